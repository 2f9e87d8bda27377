#!/usr/bin/env python3
"""Cost of fusing overlapping frame windows inside the sampler step.  COST ONLY.

Times lavie_window_step (guided five-coefficient family with step noise: the most operands) against the same arithmetic composed
from torch ops (fp32 copies of the windows' predictions, guidance, a strided weighted accumulation per window, the scheduler
update, one fp16 conversion and two copies per window) at two shapes:
  base   x [1, 4, 64, 40*64],    windows of 16 frames at stride 12 (5 windows)
  vsr    x [1, 4, 61, 320*512],  windows of 8 frames at stride 6 (10 windows)
in one process, A B B A, medians of device events over batches of back-to-back launches (microseconds per step in a stream of
steps, launch overhead included, which is how the denoising loop issues them).  The record states the algorithmic bytes of the
fused step (x in and out, the noise, both guidance halves of every window's eps read and model input written), the achieved
rate and that rate as a fraction of 8 TB/s; the working set is re-run in place, so a rate may include hits in the last-level
cache.  Prints one JSON line and writes it to --out.
Usage: python tools/bench_window_fuse.py [--rounds 5] [--out profiles/window_fuse.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import ops  # noqa: E402
from lavie_amd.windows import window_profile, window_starts  # noqa: E402

CASES = {"base": dict(shape=(1, 4, 64, 40 * 64), length=16, stride=12, batch=50),
         "vsr": dict(shape=(1, 4, 61, 320 * 512), length=8, stride=6, batch=10)}
PEAK_BPS = 8e12
GUIDANCE, SCALE = 7.5, 0.9
COEFFS = (0.5, 0.1, 0.2, 0.7, 0.05)      # contractive: the state stays bounded over thousands of in-place steps


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
    return statistics.median(ta), statistics.median(tb), ta, tb


def torch_step(eps, x, noise, model_in, starts, weights, fused):
    """The same step from torch ops: weights[w] = the window's normalised profile on the device, fused = an fp32 scratch of x's shape."""
    k_x, k_e, c_x0, c_xt, sigma = COEFFS
    p, length = x.shape[0], weights[0].shape[0]
    fused.zero_()
    for s, e, wt in zip(starts, eps, weights):
        e = e.float()
        e = e[:p] + GUIDANCE * (e[p:] - e[:p])
        fused[:, :, s:s + length] += wt.view(1, 1, -1, 1) * e
    x0 = k_x * x - k_e * fused
    x.copy_(c_xt * x + c_x0 * x0 + sigma * noise)
    for s, m in zip(starts, model_in):
        h = (x[:, :, s:s + length] * SCALE).half()
        m[:p] = h
        m[p:] = h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="A B B A rounds per shape")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_window_fuse needs a HIP device"
    torch.cuda.set_device(0)
    res = {"metric": "window_fuse_step_cost", "family": "five-coefficient, guided, step noise", "order": "A B B A",
           "peak_bytes_per_s": PEAK_BPS, "device": torch.cuda.get_device_name(0)}
    for name, case in CASES.items():
        shape, length, batch = case["shape"], case["length"], case["batch"]
        p, c, frames, hw = shape
        starts = window_starts(frames, length, case["stride"])
        profile = window_profile(length, "triangle")
        g = torch.Generator().manual_seed(0)
        x = torch.randn(shape, generator=g).cuda()
        noise = torch.randn(shape, generator=g).cuda()
        eps = [torch.randn(2 * p, c, length, hw, generator=g).half().cuda() for _ in starts]
        model_in = [torch.empty_like(e) for e in eps]
        cover = torch.zeros(frames)
        for s in starts:
            cover[s:s + length] += torch.tensor(profile)
        weights = [(torch.tensor(profile) / cover[s:s + length]).cuda() for s in starts]
        fused = torch.empty_like(x)
        run_fused = lambda: [ops.window_step(eps, x, noise, model_in, starts, profile, GUIDANCE, COEFFS, SCALE)      # noqa: E731
                             for _ in range(batch)]
        run_torch = lambda: [torch_step(eps, x, noise, model_in, starts, weights, fused) for _ in range(batch)]      # noqa: E731
        run_fused(), run_torch()
        m_f, m_t, s_f, s_t = abba(run_fused, run_torch, a.rounds)
        assert torch.isfinite(x).all()
        n, nwin = p * c * frames * hw, len(starts) * p * c * length * hw
        nbytes = n * (4 + 4 + 4) + nwin * (2 * 2 + 2 * 2)          # x in, noise, x out; eps and model_in, two halves each
        us_f, us_t = 1e3 * m_f / batch, 1e3 * m_t / batch
        res[name] = {"shape": list(shape), "window_length": length, "window_stride": case["stride"], "windows": len(starts),
                     "launches_per_sample": batch, "fused_us": us_f, "torch_us": us_t, "torch_over_fused": us_t / us_f,
                     "fused_not_slower": us_f <= us_t, "algorithmic_bytes": nbytes, "fused_GBps": nbytes / (1e3 * us_f),
                     "fused_fraction_of_8TBps": nbytes / (1e-6 * us_f) / PEAK_BPS,
                     "fused_us_all": [round(1e3 * v / batch, 3) for v in s_f], "torch_us_all": [round(1e3 * v / batch, 3) for v in s_t]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    assert all(res[k]["fused_not_slower"] for k in CASES), "the fused step is slower than the torch composition"


if __name__ == "__main__":
    main()
