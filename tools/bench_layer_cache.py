#!/usr/bin/env python3
"""What the layer cache saves per step: one UNet forward in mode off / refresh / reuse, at the base shape
(909 M-parameter base UNet, CFG batch 2, 16 frames, latent 40x64, context cached, shared CFG prefix, as the denoise loop runs it) and
at one VSR chunk (691 M-parameter VSR UNet, batch 2, 8 frames, 320x512), for depths 1 and 2.

Per model and depth the modes are timed in ONE process in blocks ordered A B B A (A = the plain forward, B = the mode under test), each
block `--iters` forwards between two device events with a synchronise behind it; a figure is the median over the forwards of both
blocks of its mode.  A reuse block follows a refresh forward.  Random-init fp16 weights; nothing here says anything about output quality.
Prints one JSON line (and writes it to --out).  Not the driver's bench; same measurement rules.
Usage: python tools/bench_layer_cache.py [--iters 5] [--models base vsr] [--out profiles/layer_cache.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lavie_amd import spec, weights  # noqa: E402


def times(fn, iters):
    """Device-event milliseconds of each of `iters` runs of `fn`."""
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def abba(plain, other, iters, before_other=None):
    """(median ms of `plain`, median ms of `other`, all samples) over blocks plain / other / other / plain."""
    a, b = [], []
    for block in "ABBA":
        if block == "A":
            a += times(plain, iters)
        else:
            if before_other:
                before_other()
            b += times(other, iters)
    return statistics.median(a), statistics.median(b), {"plain": a, "other": b}


def measure(net, forward, iters):
    """forward(mode) runs one forward of `net`; per depth: plain, refresh and reuse medians, their ratios, the cache's bytes."""
    res = {}
    forward(None)                                        # warm-up: packs the weights, sizes the workspace
    for depth in (1, 2):
        net.enable_layer_cache(depth)
        forward("refresh")
        forward("reuse")                                 # warm-up of the shallow walk's launches
        p1, refresh, s1 = abba(lambda: forward(None), lambda: forward("refresh"), iters)
        p2, reuse, s2 = abba(lambda: forward(None), lambda: forward("reuse"), iters, before_other=lambda: forward("refresh"))
        res[f"depth{depth}"] = {
            "cache_mb": round(net.layer_cache_bytes() / 1e6, 1),
            "plain_ms": round(p1, 3), "refresh_ms": round(refresh, 3), "refresh_minus_plain_ms": round(refresh - p1, 3),
            "refresh_over_plain": round(refresh / p1, 4),
            "plain_ms_beside_reuse": round(p2, 3), "reuse_ms": round(reuse, 3), "reuse_over_plain": round(reuse / p2, 4),
            # the mean forward of a loop at cache_interval N against the plain loop: (1 refresh + (N - 1) reuse) / N plain
            "step_ratio_at_interval": {str(n): round((refresh + (n - 1) * reuse) / (n * p2), 4) for n in (2, 3, 5)},
            "samples_ms": {"plain_beside_refresh": [round(v, 3) for v in s1["plain"]], "refresh": [round(v, 3) for v in s1["other"]],
                           "plain_beside_reuse": [round(v, 3) for v in s2["plain"]], "reuse": [round(v, 3) for v in s2["other"]]},
        }
        net.disable_layer_cache()
    return res


def base_model(dev, iters):
    from lavie_amd.unet import UNet3DConditionModel
    sd = bench.synth_weights(spec.param_shapes(), 0)
    net = UNet3DConditionModel(sample_size=64, cross_attention_dim=768, init_weights=False)
    for name, p in net.named_parameters():
        p.data = sd[name].to(dev, torch.float16)
    del sd
    pe, ne, lat = bench.synth_inputs(0, dev)
    ctx = torch.cat([ne, pe]).half().contiguous()
    x = torch.cat([lat, lat]).half().contiguous()
    net.prepare(2, 16, 40, 64, ctx.shape[1])
    cc = net.cache_context(ctx)
    net.set_cfg_shared_input(True)
    res = measure(net, lambda mode: net(x, 500, encoder_hidden_states=cc, layer_cache=mode), iters)
    net.set_cfg_shared_input(False)
    net.cache_context(None)
    res["shape"] = "B2 F16 40x64 ctx77, context cached, CFG shared prefix"
    return res


def vsr_model(dev, iters):
    from lavie_amd.config import VSR_CONFIG
    from lavie_amd.vsr import UNet3DVSRModel
    F, H, W = 8, 320, 512
    sd = weights.synth_state_dict(spec.param_shapes(VSR_CONFIG), 0)
    net = UNet3DVSRModel(init_weights=False, sample_size=128, down_temporal_idx=(0, 1, 2, 3), mid_temporal=True, up_temporal_idx=(0, 1, 2, 3))
    net.load_state_dict({k: v.half() for k, v in sd.items()})
    del sd
    net = net.to(dev, torch.float16)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, F, H, W, generator=g).half().to(dev)
    low = torch.randn(2, 3, F, H, W, generator=g).half().to(dev)
    ctx = torch.randn(2, bench.CTX_LEN, 1024, generator=g).half().to(dev)
    labels = torch.tensor([20, 20])
    net.prepare(2, F, H, W, ctx.shape[1])
    cc = net.cache_context(ctx)
    res = measure(net, lambda mode: net(x, 500, low, encoder_hidden_states=cc, class_labels=labels, layer_cache=mode), iters)
    net.cache_context(None)
    res["shape"] = "B2 F8 320x512 ctx77, context cached"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=["base", "vsr"], choices=["base", "vsr"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"metric": "layer_cache_forward_ms", "iters_per_block": a.iters,
           "order": "per depth: plain / refresh / refresh / plain, then plain / reuse / reuse / plain (a refresh forward in front of each "
                    "reuse block); medians over the 2 x iters forwards of a mode; device events"}
    for name in a.models:
        res[name] = (base_model if name == "base" else vsr_model)(dev, a.iters)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
