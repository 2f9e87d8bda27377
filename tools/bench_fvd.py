#!/usr/bin/env python3
"""Cost of FVD features on the engine.  COST ONLY: the guarantees are the per-element bounds and the bits.

In one process, warmed, medians of device events over windows of 10 back-to-back calls (40 for the preprocess):
  features    HipR3D18 on 1 and on 8 clips of 16 x 224 x 224 (fp32 pixels, workspace allocated per call by the wrapper), against the
              same restated module (tests/r3d_reference.py) in fp16 through stock torch.nn.Conv3d on the device, where MIOpen serves
              it (--no-stock skips that side; a failure there is recorded as text and the engine's times stand alone)
  layers      the per-layer split of one clip through the operator entries: stem, layer1 .. layer4 (two blocks each), mean_rows
  preprocess  ops.video_preprocess of uint8 [16, 320, 512, 3] (crop 270, size 224)
The engine's results are written before the stock side starts.  Prints one JSON line and writes it to --out.
Usage: python tools/bench_fvd.py [--rounds 5] [--no-stock] [--out profiles/fvd.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import r3d_reference as R  # noqa: E402
from lavie_amd import fvd, ops  # noqa: E402


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def median_ms(fn, rounds, batch=10, warm=2):
    """median over `rounds` windows of `batch` back-to-back calls each, per call"""
    for _ in range(warm):
        fn()

    def window():
        for _ in range(batch):
            fn()
    return statistics.median(event_ms(window) for _ in range(rounds)) / batch


def folded(sd, name):
    w, b = fvd.fold_batchnorm(sd[f"{name}.0.weight"], *(sd[f"{name}.1.{p}"] for p in ("weight", "bias", "running_mean", "running_var")))
    return ops.pack_conv3d(w.cuda()), b.cuda()


def layer_split(sd, x, rounds):
    """ms per stage of one forward through the operator entries, and the conv FLOPs of each"""
    out, flops = {}, {}
    wp, b = folded(sd, "stem")
    out["stem"] = median_ms(lambda: ops.conv3d_stem(x, wp, b), rounds)
    h = ops.conv3d_stem(x, wp, b)
    flops["stem"] = 2.0 * h.numel() * 441
    for level in range(1, 5):
        blocks = []
        for blk in range(2):
            p = f"layer{level}.{blk}"
            blocks.append((folded(sd, f"{p}.conv1"), folded(sd, f"{p}.conv2"), folded(sd, f"{p}.downsample") if level > 1 and blk == 0 else None))

        def run(h=h, blocks=blocks):
            for (w1, b1), (w2, b2), down in blocks:
                t = ops.conv3d(h, w1, b1, stride=2 if down else 1, relu=True)
                r = ops.conv3d(h, down[0], down[1], ksize=1, stride=2) if down else h
                h = ops.conv3d(t, w2, b2, residual=r, relu=True)
            return h
        out[f"layer{level}"] = median_ms(run, rounds)
        cin = h.shape[-1]
        h = run()
        rows, c = h.numel() // h.shape[-1], h.shape[-1]
        flops[f"layer{level}"] = 2.0 * rows * c * 27 * (cin + 3 * c) + (2.0 * rows * c * cin if level > 1 else 0.0)
    rows = h.reshape(h.shape[0], -1, h.shape[-1])
    out["mean_rows"] = median_ms(lambda: ops.mean_rows(rows), rounds)
    return out, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fvd.json"))
    args = ap.parse_args()
    module = R.make_r3d18(seed=0)
    sd = module.state_dict()
    engine = fvd.HipR3D18.from_state_dict(sd)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "clip": [16, 224, 224]}
    g = torch.Generator().manual_seed(0)
    clips = {n: torch.randn(n, 3, 16, 224, 224, generator=g).cuda() for n in (1, 8)}
    res["engine_ms"] = {str(n): median_ms(lambda x=x: engine(x), args.rounds) for n, x in clips.items()}
    split, flops = layer_split(sd, clips[1], args.rounds)
    res["layers_ms_1clip"] = split
    res["layers_gflop_1clip"] = {k: v / 1e9 for k, v in flops.items()}
    res["gflop_per_clip"] = sum(flops.values()) / 1e9
    res["engine_tflops"] = {n: res["gflop_per_clip"] * int(n) / ms for n, ms in res["engine_ms"].items()}
    frames = torch.randint(0, 256, (16, 320, 512, 3), dtype=torch.uint8, generator=g).cuda()
    out = torch.empty(16, 3, 224, 224, device="cuda")
    res["preprocess_ms"] = median_ms(lambda: ops.video_preprocess(frames, 270, 224, out=out), args.rounds, batch=40)

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    res["stock_ms"] = None
    res["stock_note"] = "skipped (--no-stock)" if args.no_stock else "did not finish"
    write()
    if not args.no_stock:
        try:
            stock = module.half().cuda()
            with torch.no_grad():
                res["stock_ms"] = {str(n): median_ms(lambda x=x: stock.features(x.half()), args.rounds) for n, x in clips.items()}
                # the two sides on the timed input: both round every activation to fp16, in different accumulation orders
                res["engine_vs_stock_max_abs_1clip"] = float((engine(clips[1]) - stock.features(clips[1].half()).float()).abs().max())
                res["features_mean_abs_1clip"] = float(engine(clips[1]).abs().mean())
            res["stock_note"] = "torch.nn.Conv3d fp16 on the device, same module, warmed"
        except Exception as exc:        # MIOpen may not serve fp16 Conv3d here: the engine's times stand alone
            res["stock_note"] = f"stock side failed: {type(exc).__name__}: {str(exc)[:200]}"
        write()
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
