#!/usr/bin/env python3
"""Cost of FreeInit's frequency mix (ops.freq_mix, csrc/freq_mix.hip).  COST ONLY.

Two forms of one mix between two sampling iterations, guided (the fp16 model input is written twice), at two shapes:
  base   latents [1, 4, 16, 40, 64]     the base model's clip
  long   latents [1, 4, 64, 40, 64]     a 64-frame clip sampled as frame windows
  fused   ops.freq_mix: six launches of the direct fp32 DFT, the fp16 model input written by the last one
  torch   the same result composed from torch ops on the device the way diffusers does it: z_T = a x0 + s e0, fftn + fftshift of z_T
          and of r z, the blend with the shifted filter, ifftshift + ifftn, .real, then (x scale).half() into both halves.  If the
          installed torch cannot run an FFT on the device the record says so and only the fused op is timed.
in one process, A B B A, medians of device events over batches of back-to-back calls (microseconds per call in a stream of calls,
launch overhead included).  The working set is re-run in place and fits the last-level cache.  No target is set: the record states
what came out.  Prints one JSON line and writes it to --out.
Usage: python tools/bench_free_init.py [--rounds 5] [--out profiles/free_init.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import ops  # noqa: E402
from lavie_amd.free_init import FreeInit  # noqa: E402
from lavie_amd.scheduling_ddpm import DDPMScheduler  # noqa: E402

CASES = {"base": dict(shape=(1, 4, 16, 40, 64), batch=50), "long": dict(shape=(1, 4, 64, 40, 64), batch=20)}
SCALE, DIMS = 0.9, (-3, -2, -1)


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def abba(a, b, rounds):
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(event_ms(a))
        tb.append(event_ms(b))
        tb.append(event_ms(b))
        ta.append(event_ms(a))
    return ta, tb


def torch_mix(x0, e0, z, lpf_shifted, a, s, r, out, model_in):
    z_t = a * x0 + s * e0
    zf = torch.fft.fftshift(torch.fft.fftn(z_t, dim=DIMS), dim=DIMS)
    nf = torch.fft.fftshift(torch.fft.fftn(r * z, dim=DIMS), dim=DIMS)
    mixed = zf * lpf_shifted + nf * (1 - lpf_shifted)
    out.copy_(torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=DIMS), dim=DIMS).real)
    h = (out * SCALE).half()
    p = out.shape[0]
    model_in[:p] = h
    model_in[p:] = h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="A B B A rounds per shape")
    ap.add_argument("--out", default="")
    arg = ap.parse_args()
    assert torch.cuda.is_available(), "bench_free_init needs a HIP device"
    torch.cuda.set_device(0)
    sch = DDPMScheduler()
    a, s = sch.noise_level(sch.config.num_train_timesteps - 1)
    setting = FreeInit()
    res = {"metric": "free_init_mix_cost", "order": "A B B A", "filter": repr(setting), "copies_of_model_input": 2,
           "device": torch.cuda.get_device_name(0)}
    for name, case in CASES.items():
        shape, batch = case["shape"], case["batch"]
        g = torch.Generator().manual_seed(0)
        x0, e0, z = (torch.randn(shape, generator=g).cuda() for _ in range(3))
        filt = setting.filter(*shape[2:]).cuda()
        # the shifted filter of the composition: the op's filter is the even part, which for these even lengths is the filter itself
        lpf_shifted = torch.fft.fftshift(filt)
        out_f, out_t = torch.empty_like(x0), torch.empty_like(x0)
        min_f = torch.empty((2,) + shape[1:], dtype=torch.float16, device="cuda")
        min_t = torch.empty_like(min_f)
        ws = torch.empty(ops.freq_mix_workspace_bytes(shape[0] * shape[1], *shape[2:]) // 4, device="cuda")
        run_fused = lambda: [ops.freq_mix(x0, e0, z, filt, a, s, 1.0, out=out_f, model_in=min_f, input_scale=SCALE, workspace=ws)     # noqa: E731
                             for _ in range(batch)]
        run_torch = lambda: [torch_mix(x0, e0, z, lpf_shifted, a, s, 1.0, out_t, min_t) for _ in range(batch)]                     # noqa: E731
        run_fused()
        fft_error = None
        try:
            run_torch()
            torch.cuda.synchronize()
        except Exception as exc:                       # noqa: BLE001  (no device FFT in this torch build: recorded, not hidden)
            fft_error = f"{type(exc).__name__}: {exc}"[:300]
        us = lambda v: 1e3 * statistics.median(v) / batch       # noqa: E731
        rec = {"shape": list(shape), "calls_per_sample": batch, "launches_fused": 6}
        if fft_error is None:
            tf, tt = abba(run_fused, run_torch, arg.rounds)
            rec.update(fused_us=us(tf), torch_us=us(tt), torch_over_fused=us(tt) / us(tf),
                       max_abs_difference=float((out_f - out_t).abs().max()),
                       fused_us_all=[round(1e3 * v / batch, 3) for v in tf], torch_us_all=[round(1e3 * v / batch, 3) for v in tt])
        else:
            tf = [event_ms(run_fused) for _ in range(4 * arg.rounds)]
            rec.update(fused_us=us(tf), torch_us=None, torch_fft_on_device=fft_error, fused_us_all=[round(1e3 * v / batch, 3) for v in tf])
        assert torch.isfinite(out_f).all()
        res[name] = rec
    line = json.dumps(res)
    print(line)
    if arg.out:
        with open(arg.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
