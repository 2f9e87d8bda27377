#!/usr/bin/env python3
"""Cost of the known-region replacement inside the sampler step.  COST ONLY.

Times the pinned against the un-pinned step kernel of each family (five-coefficient: lavie_cfg_sampler_step[_known];
multistep: lavie_cfg_multistep_step[_known], second-order form) at the base latent shape, n = 4*16*40*64 (one video, guidance
on), in one process, A B B A, medians of device events over batches of back-to-back launches (so the figure is microseconds
per launch in a stream of launches, launch overhead included, which is how the denoising loop issues them).  The pinned
kernel reads three more operands (known, noise_known: 4 bytes per element each; the mask: 4 bytes per C elements); the
record states the bytes and the achieved GB/s of both beside each other.
Prints one JSON line and writes it to --out.  Usage: python tools/bench_known_region.py [--rounds 5] [--out profiles/known_region.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import _lib  # noqa: E402

SHAPE = (1, 4, 16, 40, 64)
BATCH = 50            # launches between two events


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="A B B A rounds per family")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_known_region needs a HIP device"
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    n = int(torch.tensor(SHAPE).prod())
    eps = torch.randn(2 * n, generator=g).half().cuda()
    x = torch.randn(SHAPE, generator=g).cuda()
    hist = torch.randn(SHAPE, generator=g).cuda()
    nz = torch.randn(SHAPE, generator=g).cuda()
    known = torch.randn(SHAPE, generator=g).cuda()
    noise = torch.randn(SHAPE, generator=g).cuda()
    mask = torch.zeros(SHAPE[0], 1, *SHAPE[2:], device="cuda")
    mask[:, :, :4] = 1.0                                   # the first 4 of 16 frames pinned (clip continuation)
    min_ = torch.empty(2 * n, dtype=torch.float16, device="cuda")
    level = (0.8, 0.6)
    # contractive coefficients: the state stays bounded over thousands of in-place launches
    five, multi = (0.5, 0.1, 0.2, 0.7, 0.05), (0.5, 0.1, 0.2, 0.7, 0.45)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = _lib.KnownRegionC(ctypes.sizeof(_lib.KnownRegionC), SHAPE[1], n // (SHAPE[0] * SHAPE[1]), known.data_ptr(), mask.data_ptr(),
                          noise.data_ptr(), *level)
    # straight through the C ABI, the region struct built once: the ops wrappers' argument checks are not part of the figure
    legs = {
        "five_coefficient": (lambda: lib.lavie_cfg_sampler_step_known(p(eps), p(x), p(nz), p(min_), n, 7.5, *five, 1.0, stream, ctypes.byref(r)),
                             lambda: lib.lavie_cfg_sampler_step(p(eps), p(x), p(nz), p(min_), n, 7.5, *five, 1.0, stream),
                             n * (2 * 2 + 4 + 4 + 4 + 2 * 2)),                      # eps2, x in, noise, x out, model_in2
        "multistep": (lambda: lib.lavie_cfg_multistep_step_known(p(eps), p(x), p(hist), p(min_), n, 7.5, *multi, 1.0, stream, ctypes.byref(r)),
                      lambda: lib.lavie_cfg_multistep_step(p(eps), p(x), p(hist), p(min_), n, 7.5, *multi, 1.0, stream),
                      n * (2 * 2 + 4 + 4 + 4 + 4 + 2 * 2)),                         # eps2, x in, hist in, x out, hist out, model_in2
    }
    extra = n * (4 + 4) + mask.numel() * 4                                          # known, noise_known, mask
    res = {"metric": "known_region_step_cost", "shape": list(SHAPE), "n": n, "launches_per_sample": BATCH, "order": "A B B A",
           "pinned_frames": 4, "extra_bytes_known_noise_mask": extra, "device": torch.cuda.get_device_name(0)}
    for name, (pinned, plain, plain_bytes) in legs.items():
        run_pinned = lambda: [pinned() for _ in range(BATCH)]       # noqa: E731
        run_plain = lambda: [plain() for _ in range(BATCH)]         # noqa: E731
        assert pinned() == 0 and plain() == 0, lib.lavie_last_error()
        run_pinned(), run_plain()
        m_p, m_u, s_p, s_u = abba(run_pinned, run_plain, a.rounds)
        assert torch.isfinite(x).all()
        res[name] = {"pinned_us": 1e3 * m_p / BATCH, "unpinned_us": 1e3 * m_u / BATCH, "ratio": m_p / m_u,
                     "pinned_bytes": plain_bytes + extra, "unpinned_bytes": plain_bytes,
                     "pinned_GBps": (plain_bytes + extra) / (1e6 * m_p / BATCH), "unpinned_GBps": plain_bytes / (1e6 * m_u / BATCH),
                     "pinned_us_all": [round(1e3 * v / BATCH, 3) for v in s_p],
                     "unpinned_us_all": [round(1e3 * v / BATCH, 3) for v in s_u]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
