#!/usr/bin/env python3
"""Image-conditioning costs on the production model: the 909 M-parameter base UNet (random-init fp16), CFG batch 2, 16 frames,
latent 40x64, context cached as the denoise loop runs it (shared CFG prefix on).  Measures
  - the mapper (lavie_amd.mapping.MappingNetwork, production configuration, fp32 on the device) at B = 2, and per video
    (two calls at B = 1: the conditional and the unconditional prompt, as the pipeline runs it);
  - one UNet forward at a 77-token and at a 154-token context (77 text + 77 mapped image tokens);
  - the 154-token forward with fused_mask bit 2 (the fused level-0 text cross-attention, here its long variant) on and off,
    A B B A inside this process;
  - the fused kernel's launches and average time from the profile class (one instrumented forward at 77 and at 154 tokens);
  - the 50-step guided denoise loop at 154 tokens (VideoGenPipeline.denoise), for the mapper's share of a video.
Prints one JSON line (and writes it to --out).  Not the driver's bench; same measurement rules (device events, medians).
Usage: python tools/bench_image_cond.py [--iters 10] [--out profiles/image_cond.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lavie_amd import _lib, spec, weights  # noqa: E402
from lavie_amd.mapping import MappingNetwork  # noqa: E402
from lavie_amd.pipeline_videogen import VideoGenPipeline  # noqa: E402
from lavie_amd.unet import UNet3DConditionModel  # noqa: E402

KC_FUSED_CROSS = 10
MASK_ON = _lib.FUSED_DEFAULT
MASK_OFF = _lib.FUSED_DEFAULT & ~4


def timed(fn, iters):
    """Median device-event milliseconds of `fn` over `iters` runs (stream-ordered end event)."""
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out)


def fused_class(lib, fwd):
    """(launches, average us) of the fused text cross-attention class in one instrumented forward."""
    fwd()
    bench.profile_begin(lib, 1 << KC_FUSED_CROSS, 64)
    fwd()
    row = bench.profile_end(lib)[KC_FUSED_CROSS]
    return row["launches"], (row["ms"] * 1e3 / row["launches"]) if row["launches"] else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _lib.load()
    res = {"metric": "image_cond_ms", "shape": "B2 F16 40x64, context cached, CFG shared prefix", "iters": a.iters}

    # ---- the mapper (stock PyTorch on the device)
    torch.manual_seed(0)
    mshapes = {k: tuple(v.shape) for k, v in MappingNetwork().state_dict().items()}
    mapper = MappingNetwork.from_checkpoint(weights.synth_state_dict(mshapes, seed=1)).to(dev)
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 257, 1024, generator=g).to(dev)
    txt = torch.randn(2, 77, 768, generator=g).to(dev)
    with torch.no_grad():
        mapper(img, txt)
        res["mapper_b2_ms"] = timed(lambda: mapper(img, txt), a.iters)
        res["mapper_per_video_ms"] = timed(lambda: (mapper(img[:1], txt[:1]), mapper(img[1:], txt[1:])), a.iters)

    # ---- the UNet
    sd = bench.synth_weights(spec.param_shapes(), 0)
    net = UNet3DConditionModel(sample_size=64, cross_attention_dim=768, init_weights=False)
    for name, p in net.named_parameters():
        p.data = sd[name].to(dev, torch.float16)
    del sd
    pe, ne, lat = bench.synth_inputs(0, dev)
    x = torch.cat([lat, lat]).half().contiguous()
    with torch.no_grad():
        img1 = img[:1]
        ctx154 = torch.cat([torch.cat([ne, mapper(img1, ne)], 1), torch.cat([pe, mapper(img1, pe)], 1)]).half().contiguous()
    ctx77 = torch.cat([ne, pe]).half().contiguous()
    net.set_cfg_shared_input(True)
    try:
        for n, ctx in ((77, ctx77), (154, ctx154)):
            net.prepare(2, 16, 40, 64, n)
            cc = net.cache_context(ctx)
            fwd = lambda: net(x, 500, encoder_hidden_states=cc)        # noqa: E731
            fwd()
            res[f"forward_{n}_ms"] = timed(fwd, a.iters)
            res[f"fused_cross_launches_{n}"], res[f"fused_cross_avg_us_{n}"] = fused_class(lib, fwd)
            if n == 154:
                # A B B A: fused long kernel on / off in one process, the same cached context
                abba = []
                for mask in (MASK_ON, MASK_OFF, MASK_OFF, MASK_ON):
                    lib.lavie_debug_fused_mask(mask)
                    fwd()
                    abba.append(timed(fwd, a.iters))
                lib.lavie_debug_fused_mask(MASK_ON)
                res["abba_154_ms"] = {"on_1": abba[0], "off_1": abba[1], "off_2": abba[2], "on_2": abba[3]}
                on, off = (abba[0] + abba[3]) / 2, (abba[1] + abba[2]) / 2
                res["fused_long_saves_ms_per_forward"] = off - on
                lib.lavie_debug_fused_mask(MASK_OFF)
                bench.profile_begin(lib, 0x7FF, 4096)
                fwd()
                rows = bench.profile_end(lib)
                lib.lavie_debug_fused_mask(MASK_ON)
                res["unfused_154_class_ms"] = {r["name"]: round(r["ms"], 4) for r in rows if r["launches"]}
            net.cache_context(None)
    finally:
        lib.lavie_debug_fused_mask(MASK_ON)
        net.set_cfg_shared_input(False)
        net.cache_context(None)

    # ---- the 50-step guided loop at 154 tokens, and the mapper's share of a video
    pipe = VideoGenPipeline(unet=net)
    loop = lambda: pipe.denoise(lat.float(), ctx154, 50, 7.5, torch.Generator(device=dev).manual_seed(0))   # noqa: E731
    loop()
    res["denoise_50_steps_154_ms"] = timed(loop, 3)
    res["mapper_share_of_video"] = res["mapper_per_video_ms"] / (res["mapper_per_video_ms"] + res["denoise_50_steps_154_ms"])
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
