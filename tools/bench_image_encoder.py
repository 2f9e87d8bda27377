#!/usr/bin/env python3
"""What image conditioning costs on the engine (lavie_amd.image_encoder) and on the stock modules in fp16, at production size with
random weights: the CLIP ViT-L/14 vision tower (1024 wide, 24 layers, 16 heads, 224 / 14 -> 257 tokens) and the fork's 12-layer
mapper (1024 -> 768, 12 heads, 257 -> 77), B in {1, 2}.  Both arms run in ONE process in A B B A order on the same inputs; every
shape is warmed up first; a sample is a device-event time around `reps` back-to-back calls, the figure the median over the samples of
both visits of an arm.  Also: lavie_short_attention_f16 against lavie_attention_f16 (the online-softmax kernel of the UNet) at the
three shapes the two models run, and the cost of one trivial launch, from which the launch-bound share of a call is estimated as
launches x that cost / the call's time.  No speed is promised: these encoders exist for their guarantees.
Merges {"timings_us", "attention_us", "launch_us"} into --out (the error pairs of tests/test_gpu_image_encoder.py live beside them)
and prints one JSON line.
Usage: python tools/bench_image_encoder.py [--out profiles/image_encoder.json] [--reps 10] [--samples 10]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOWER = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
             hidden_act="quick_gelu", layer_norm_eps=1e-5)
MAPPER = dict(input_dim=1024, output_dim=768, num_layers=12, num_heads=12, seq_len_in=257, seq_len_out=77)
BATCHES = (1, 2)
ATT_SHAPES = {"tower 257x257, 16 heads": (257, 257, 16), "mapper self 77x77, 12 heads": (77, 77, 12), "mapper cross 77x257, 12 heads": (77, 257, 12)}


def sample(fn, reps):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0 / reps        # us per call


def abba(arms, reps, samples):
    """arms: (name_a, fn_a), (name_b, fn_b) -> name -> (median, min) over both visits"""
    (na, fa), (nb, fb) = arms
    for fn in (fa, fb):                              # warm-up: code objects, rocBLAS's choice for this M
        for _ in range(3):
            fn()
    times = {na: [], nb: []}
    for name, fn in ((na, fa), (nb, fb), (nb, fb), (na, fa)):
        times[name] += [sample(fn, reps) for _ in range(samples)]
    return {k: (round(statistics.median(v), 1), round(min(v), 1)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_encoder.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=10)
    args = ap.parse_args()
    import torch
    from transformers import CLIPVisionConfig, CLIPVisionModel
    from lavie_amd import ops
    from lavie_amd.image_encoder import HipCLIPVisionModel, HipMappingNetwork
    from lavie_amd.mapping import MappingNetwork

    tiny = torch.zeros(8, dtype=torch.float16, device="cuda")
    for _ in range(20):
        ops.relu(tiny)
    launch_us = round(statistics.median(sample(lambda: ops.relu(tiny), 200) for _ in range(args.samples)), 2)

    timings = {}
    torch.manual_seed(0)
    stock = CLIPVisionModel(CLIPVisionConfig(**TOWER)).to("cuda", torch.float16).eval()
    engine = HipCLIPVisionModel.from_stock(stock)
    feats = None
    for b in BATCHES:
        px = torch.randn(b, 3, 224, 224, generator=torch.Generator().manual_seed(b)).cuda().half()

        def run_stock():
            with torch.no_grad():
                return stock(pixel_values=px).last_hidden_state

        run_engine = lambda: engine(pixel_values=px)[0]                  # noqa: E731
        rel = float((run_engine().float() - run_stock().float()).norm() / run_stock().float().norm())
        feats = run_engine()[:1].clone()
        t = abba((("engine", run_engine), ("stock_fp16", run_stock)), args.reps, args.samples)
        launches = 2 + b + 8 * TOWER["num_hidden_layers"]
        timings[f"tower vit-l/14,B={b}"] = {"engine_us": t["engine"][0], "stock_fp16_us": t["stock_fp16"][0], "engine_min_us": t["engine"][1],
                                            "stock_fp16_min_us": t["stock_fp16"][1], "rel_l2_engine_vs_stock": rel, "engine_launches": launches,
                                            "launch_bound_share": round(launches * launch_us / t["engine"][0], 2)}
    del stock, engine
    stock = MappingNetwork(**MAPPER).to("cuda", torch.float16).eval()
    engine = HipMappingNetwork.from_stock(stock)
    for b in BATCHES:
        txt = torch.randn(b, 77, 768, generator=torch.Generator().manual_seed(b)).cuda().half()
        img = (feats / feats.float().std()).half()                        # one image for every prompt, as the pipeline calls it

        def run_stock():
            with torch.no_grad():
                return stock(img.expand(b, -1, -1), txt)

        run_engine = lambda: engine(img, txt)                            # noqa: E731
        rel = float((run_engine().float() - run_stock().float()).norm() / run_stock().float().norm())
        t = abba((("engine", run_engine), ("stock_fp16", run_stock)), args.reps, args.samples)
        launches = 1 + b + 13 * MAPPER["num_layers"]
        timings[f"mapper 12 layers,B={b}"] = {"engine_us": t["engine"][0], "stock_fp16_us": t["stock_fp16"][0], "engine_min_us": t["engine"][1],
                                              "stock_fp16_min_us": t["stock_fp16"][1], "rel_l2_engine_vs_stock": rel, "engine_launches": launches,
                                              "launch_bound_share": round(launches * launch_us / t["engine"][0], 2)}
    del stock, engine

    attention = {}
    for name, (lq, lk, heads) in ATT_SHAPES.items():
        g = torch.Generator().manual_seed(lq + lk)
        q = torch.randn(lq, heads * 64, generator=g).cuda().half()
        k, v = (torch.randn(lk, heads * 64, generator=g).cuda().half() for _ in range(2))
        o1, o2 = torch.empty_like(q), torch.empty_like(q)
        try:
            t = abba((("short", lambda: ops.short_attention(q, k, v, 1, lq, lk, heads, 64, out=o1)),
                      ("online", lambda: ops.attention(q, k, v, 1, lq, lk, heads, out=o2))), 50, args.samples)
        except (RuntimeError, ValueError) as err:                        # a shape the online-softmax entry does not take
            attention[name] = {"refused": str(err)}
            continue
        attention[name] = {"short_attention_us": t["short"][0], "attention_us": t["online"][0],
                           "max_abs_difference": float((o1.float() - o2.float()).abs().max())}

    try:
        with open(args.out) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc["timings_us"], doc["attention_us"], doc["launch_us"] = timings, attention, launch_us
    doc["timings_note"] = (f"host call to completion averaged over {args.reps} back-to-back calls; median of {2 * args.samples} samples, "
                           "A B B A in one process; launch_us: one 8-element relu launch back to back; launch_bound_share = "
                           "engine_launches x launch_us / engine_us")
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"image_encoder": {"timings_us": timings, "attention_us": attention, "launch_us": launch_us}}))


if __name__ == "__main__":
    main()
