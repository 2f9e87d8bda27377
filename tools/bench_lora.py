#!/usr/bin/env python3
"""LoRA adapter costs on the production model: the 909 M-parameter base UNet (random-init fp16), rank 16 on every target
(to_q / to_k / to_v / to_out.0 of attn1 / attn2 / attn_temp), CFG batch 2, 16 frames, latent 40x64, context cached as the
denoise loop runs it.  Times lavie_unet_lora_apply after the first registration, after a re-scale and after a clear,
refresh_engine() (destroy + full re-pack, adapter registered again), and one forward with and without the adapter.
Prints one JSON line (and writes it to --out).  Not the driver's bench; same measurement rules (device events, medians).
With --adapters N [N ...] it measures the blend instead (profiles/lora_multi.json): the apply after a re-weight with N adapters of
that rank on every target against the one-adapter apply of the same build, in one process in the order one / N / N / one, and one
forward with the blend next to one without.
Usage: python tools/bench_lora.py [--rank 16] [--iters 5] [--out profiles/lora_apply.json]
       python tools/bench_lora.py --adapters 2 4 [--rank 16] [--iters 5] [--out profiles/lora_multi.json]"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lavie_amd import _lib, lora, spec  # noqa: E402
from lavie_amd.unet import UNet3DConditionModel  # noqa: E402


def timed(fn, iters):
    """Median device-event milliseconds of `fn` over `iters` runs (host work inside fn included: stream-ordered end event)."""
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--adapters", type=int, nargs="+", default=None, help="measure the blend of N adapters (one run per N)")
    a = ap.parse_args()
    if a.adapters and not all(2 <= n <= lora.MAX_ADAPTERS for n in a.adapters):
        ap.error(f"--adapters takes values in 2..{lora.MAX_ADAPTERS}")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _lib.load()
    shapes = spec.param_shapes()
    sd = bench.synth_weights(shapes, 0)
    net = UNet3DConditionModel(sample_size=64, cross_attention_dim=768, init_weights=False)
    for name, p in net.named_parameters():
        p.data = sd[name].to(dev, torch.float16)
    del sd
    g = torch.Generator().manual_seed(1)
    targets = [n for n in shapes if lora.is_target(n)]

    def make_adapter():
        ad = {}
        for n in targets:
            rows, cols = shapes[n]
            ad[f"unet.{n[:-7]}.lora_A.weight"] = torch.randn(a.rank, cols, generator=g) / cols ** 0.5
            ad[f"unet.{n[:-7]}.lora_B.weight"] = torch.randn(rows, a.rank, generator=g) * 0.01
        return ad
    ad = make_adapter()
    target_params = sum(shapes[n][0] * shapes[n][1] for n in targets)
    pe, ne, lat = bench.synth_inputs(0, dev)
    ctx = torch.cat([ne, pe]).half().contiguous()
    x = torch.cat([lat, lat]).half().contiguous()
    net.prepare(2, 16, 40, 64, 77)
    cc = net.cache_context(ctx)
    net.set_cfg_shared_input(True)
    fwd = lambda: net(x, 500, encoder_hidden_states=cc)        # noqa: E731
    fwd()
    handle = net.engine_handle()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731

    def apply():
        _lib.check(lib.lavie_unet_lora_apply(handle, stream()), "lavie_unet_lora_apply")

    res = {"metric": "lora_apply_ms", "rank": a.rank, "targets": len(targets), "target_params": target_params,
           "shape": "B2 F16 40x64 ctx77, context cached, CFG shared prefix", "iters": a.iters}
    res["forward_base_ms"] = timed(fwd, a.iters)[0]
    if a.adapters:
        res["metric"] = "lora_multi_apply_ms"
        res["order"] = "one / N / N / one adapters loaded, per N; each figure the median of `iters` set_adapters calls (re-weight + apply + sync)"
        ads = [ad] + [make_adapter() for _ in range(max(a.adapters) - 1)]
        weights = itertools.cycle([0.5, 1.0])

        def reweight():                                  # what a user does: every loaded adapter re-weighted, one apply
            names = net.get_list_adapters()
            net.set_adapters(names, [next(weights)] * len(names))
        res["blend"] = {}
        for n in a.adapters:
            runs = {1: [], n: []}
            fwd_ms = {}
            for count in (1, n, n, 1):
                have = net.get_list_adapters()
                for i in range(len(have), count):
                    net.load_lora(ads[i], adapter_name=f"a{i}")
                if len(have) > count:
                    net.delete_adapters(have[count:])
                torch.cuda.synchronize()
                reweight()                               # warm: the kernel of this term count has run
                runs[count].append(timed(reweight, a.iters)[0])
                net.set_adapters(net.get_list_adapters())
                fwd_ms[count] = timed(fwd, a.iters)[0]
            one, blend = statistics.mean(runs[1]), statistics.mean(runs[n])
            res["blend"][str(n)] = {"apply_one_ms": runs[1], "apply_blend_ms": runs[n], "blend_over_one": blend / one,
                                    "blend_over_n_single_applies": blend / (n * one), "forward_one_ms": fwd_ms[1],
                                    "forward_blend_ms": fwd_ms[n]}
            net.unload_lora()
        net.cache_context(None)
        net.set_cfg_shared_input(False)
        res["device"] = torch.cuda.get_device_name(dev)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
    # first registration (host copies -> device, lavie_unet_lora_set x targets) + apply, as load_lora does it
    t0 = time.perf_counter()
    net.load_lora(ad)
    torch.cuda.synchronize()
    res["load_lora_wall_ms"] = (time.perf_counter() - t0) * 1e3
    res["forward_lora_ms"] = timed(fwd, a.iters)[0]

    # the apply alone after a change of the global scale (every target of every block re-merged + re-derived + K / V recomputed)
    scales = iter([0.5, 1.0] * (a.iters + 1))

    def rescale():
        _lib.check(lib.lavie_unet_lora_set_scale(handle, next(scales)), "lavie_unet_lora_set_scale")
        apply()
    res["apply_rescale_ms"], res["apply_rescale_all_ms"] = timed(rescale, a.iters)
    net.set_lora_scale(1.0)
    # clear: base weights written back, blocks re-derived; re-registered between runs (outside the timed region)
    clear_ms = []
    for _ in range(a.iters):
        net.load_lora(ad)
        torch.cuda.synchronize()
        _lib.check(lib.lavie_unet_lora_clear(handle, None, stream()), "lavie_unet_lora_clear")
        clear_ms.append(timed(apply, 1)[0])
    res["apply_clear_ms"] = statistics.median(clear_ms)
    # first apply after registration on a fresh engine state: register (outside) then time the apply
    first_ms = []
    for _ in range(a.iters):
        net.unload_lora()
        net.__dict__["_lora"] = {}
        torch.cuda.synchronize()
        t = lora.normalize_lora_state_dict(ad)
        keep = []
        for n, (A, B, _) in t.items():
            w = dict(net.named_parameters())[n].data
            Ad, Bd = A.to(dev), B.to(dev)
            keep += [Ad, Bd]
            _lib.check(lib.lavie_unet_lora_set(handle, n.encode(), ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(Ad.data_ptr()),
                                               ctypes.c_void_p(Bd.data_ptr()), a.rank, 1.0, stream()), "lavie_unet_lora_set")
        torch.cuda.synchronize()
        first_ms.append(timed(apply, 1)[0])
    res["apply_first_ms"] = statistics.median(first_ms)
    _lib.check(lib.lavie_unet_lora_clear(handle, None, stream()), "lavie_unet_lora_clear")
    apply()
    net.cache_context(None)
    net.set_cfg_shared_input(False)
    net.load_lora(ad)
    torch.cuda.synchronize()

    def refresh():
        net.refresh_engine()
    res["refresh_engine_ms"] = timed(refresh, max(2, a.iters // 2))[0]
    net.prepare(2, 16, 40, 64, 77)
    cc = net.cache_context(ctx)
    res["forward_lora_after_refresh_ms"] = timed(lambda: net(x, 500, encoder_hidden_states=cc), a.iters)[0]
    net.cache_context(None)
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
