#!/usr/bin/env python3
"""What one prompt encode costs on the engine (lavie_amd.text_encoder.HipCLIPTextModel) and on the stock transformers module in fp16,
at the two full configurations of the cascade with random weights: ViT-L/14 text (768 wide, 12 layers, 12 heads, quick_gelu) and the
x4 upscaler's encoder (1024 wide, 23 layers, 16 heads, gelu), L = 77, B in {1, 2, 8}.  Both arms run in ONE process in A B B A order
on the same ids; every shape is warmed up first; a sample is a device-event time around `reps` back-to-back calls (a single encode is
well under a millisecond), and the figure is the median over the samples of both visits of an arm.  No speed is promised: the engine
encoder exists for its guarantees, this writes down what they cost.
Merges {"timings_us": ...} into --out (the error pairs of tests/test_gpu_text_encoder.py live beside it) and prints one JSON line.
Usage: python tools/bench_text_encoder.py [--out profiles/text_encoder.json] [--reps 20] [--samples 15]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "vit-l": dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                  max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5),
    "vit-h": dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                  max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5),
}
BATCHES = (1, 2, 8)
L = 77


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=15)
    args = ap.parse_args()
    import torch
    from transformers import CLIPTextConfig, CLIPTextModel
    from lavie_amd.text_encoder import HipCLIPTextModel

    result = {}
    for name, cfg in CONFIGS.items():
        torch.manual_seed(0)
        stock = CLIPTextModel(CLIPTextConfig(bos_token_id=0, eos_token_id=2, **cfg)).to("cuda", torch.float16).eval()
        engine = HipCLIPTextModel.from_stock(stock)
        for b in BATCHES:
            ids = torch.randint(0, cfg["vocab_size"], (b, L), generator=torch.Generator().manual_seed(b)).cuda()
            ids32 = ids.to(torch.int32)

            def run_stock():
                with torch.no_grad():
                    return stock(ids)[0]

            run_engine = lambda: engine(ids32)[0]                    # noqa: E731
            rel = float((run_engine().float() - run_stock().float()).norm() / run_stock().float().norm())
            for fn in (run_engine, run_stock):                       # warm-up: code objects, rocBLAS's choice for this M
                for _ in range(5):
                    fn()
            times = {"engine": [], "stock_fp16": []}
            for arm, fn in (("engine", run_engine), ("stock_fp16", run_stock), ("stock_fp16", run_stock), ("engine", run_engine)):
                times[arm] += [sample(fn, args.reps) for _ in range(args.samples)]
            result[f"{name},B={b}"] = {"engine_us": round(statistics.median(times["engine"]), 1),
                                       "stock_fp16_us": round(statistics.median(times["stock_fp16"]), 1),
                                       "engine_min_us": round(min(times["engine"]), 1), "stock_fp16_min_us": round(min(times["stock_fp16"]), 1),
                                       "rel_l2_engine_vs_stock": rel}
        del stock, engine
    try:
        with open(args.out) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc["timings_us"] = result
    doc["timings_note"] = (f"one encode at L = {L}, host call to completion averaged over {args.reps} back-to-back calls; median of "
                           f"{2 * args.samples} samples, A B B A in one process; the engine arm includes the host-side id validation of "
                           "HipCLIPTextModel.__call__")
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"text_encoder_timings_us": result}))


if __name__ == "__main__":
    main()
