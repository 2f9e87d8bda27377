#!/usr/bin/env python3
"""Cost of the step's noise, three ways.  COST ONLY: the feature's guarantee is the addressing, not a speed.

At two shapes
  base   x [1, 4, 16, 40*64]:    the guided plain step (cfg_ddpm_step)
  vsr    x [1, 4, 61, 320*512]:  the guided window step, windows of 8 frames at stride 6 (10 windows)
one denoising step's noise and update are timed as
  (a) torch   noise.normal_(generator=<device torch.Generator>), then today's step reading the tensor
  (b) tensor  ops.philox_normal into the same buffer, then the same step
  (c) fused   the seeded step: the noise is made in registers, no tensor is written or read
in one process, in the order a b c c b a per round (A B B A over three variants), medians of device events over batches of
back-to-back steps (microseconds per step, launch overhead included, which is how the loop issues them).  The draw number moves
with every step, as in a loop.  The working set is re-run in place, so a time may include hits in the last-level cache.  Prints one
JSON line and writes it to --out.
Usage: python tools/bench_noise.py [--rounds 5] [--out profiles/engine_noise.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import ops  # noqa: E402
from lavie_amd.noise import NoiseKey  # noqa: E402
from lavie_amd.windows import window_profile, window_starts  # noqa: E402

CASES = {"base": dict(shape=(1, 4, 16, 40 * 64), windowed=False, batch=50),
         "vsr": dict(shape=(1, 4, 61, 320 * 512), windowed=True, length=8, stride=6, batch=10)}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="a b c c b a rounds per shape")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_noise needs a HIP device"
    torch.cuda.set_device(0)
    res = {"metric": "engine_noise_step_cost", "order": "a b c c b a", "variants": {"a": "torch normal_ + step", "b": "philox_normal + step",
                                                                                    "c": "fused seeded step"},
           "device": torch.cuda.get_device_name(0)}
    for name, case in CASES.items():
        shape, batch = case["shape"], case["batch"]
        p, c, frames, hw = shape
        g = torch.Generator().manual_seed(0)
        x = torch.randn(shape, generator=g).cuda()
        noise = torch.empty_like(x)
        gen = torch.Generator(device="cuda").manual_seed(1)
        draw = [0]

        def key():
            draw[0] += 1
            return NoiseKey([12345], draw[0])

        if case["windowed"]:
            length = case["length"]
            starts, profile = window_starts(frames, length, case["stride"]), window_profile(length, "triangle")
            eps = [torch.randn(2 * p, c, length, hw, generator=g).half().cuda() for _ in starts]
            model_in = [torch.empty_like(e) for e in eps]
            tensor_step = lambda: ops.window_step(eps, x, noise, model_in, starts, profile, GUIDANCE, COEFFS, SCALE)             # noqa: E731
            fused_step = lambda: ops.window_step_seeded(eps, x, key(), model_in, starts, profile, GUIDANCE, COEFFS, SCALE)      # noqa: E731
        else:
            eps = torch.randn((2 * p,) + shape[1:], generator=g).half().cuda()
            model_in = torch.empty_like(eps)
            tensor_step = lambda: ops.cfg_ddpm_step(eps, x, noise, model_in, GUIDANCE, COEFFS, SCALE)                            # noqa: E731
            fused_step = lambda: ops.cfg_sampler_step_seeded(eps, x, key(), model_in, GUIDANCE, COEFFS, SCALE)                  # noqa: E731
        per = c * frames * hw

        def run_a():
            for _ in range(batch):
                noise.normal_(generator=gen)
                tensor_step()

        def run_b():
            for _ in range(batch):
                k = key()
                ops.philox_normal(k.seeds, per, k.draw, out=noise)
                tensor_step()

        def run_c():
            for _ in range(batch):
                fused_step()

        runs = {"a": run_a, "b": run_b, "c": run_c}
        for fn in runs.values():            # warm-up: every code object loaded, every shape seen
            fn()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k in ("a", "b", "c", "c", "b", "a"):
                times[k].append(event_ms(runs[k]))
        assert torch.isfinite(x).all()
        us = {k: 1e3 * statistics.median(v) / batch for k, v in times.items()}
        res[name] = {"shape": list(shape), "windowed": case["windowed"], "steps_per_sample": batch,
                     "torch_us": us["a"], "tensor_us": us["b"], "fused_us": us["c"], "fused_over_torch": us["c"] / us["a"],
                     "tensor_over_torch": us["b"] / us["a"],
                     "all_us": {k: [round(1e3 * t / batch, 3) for t in v] for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
