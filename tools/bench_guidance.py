#!/usr/bin/env python3
"""Cost of guidance rescale inside the fused sampler step.  COST ONLY.

Three forms of one guided five-coefficient step (DDIM at eta = 0: no step noise), at two shapes:
  base   x [1, 4, 16, 40*64]      the base model's latents
  vsr    x [1, 4, 8, 320*512]     one 8-frame chunk of the super-resolution stage
  table   ops.guidance_table (the moments launch and the fold launch) + ops.cfg_sampler_step_scaled
  plain   ops.cfg_ddpm_step: the guided step without rescale, the code every call without the new keywords still runs
  torch   the same rescale composed from torch ops (fp32 copies, guidance, two torch.std, the scale, the scheduler update, one
          fp16 conversion and two copies); torch.std synchronises nothing, the composition stays on the device
in one process, A B B A per pair (table against plain, table against torch), medians of device events over batches of back-to-back
steps (microseconds per step in a stream of steps, launch overhead included, as the denoising loop issues them).  The working set
is re-run in place, so a rate may include hits in the last-level cache.  The fold runs as a launch of its own (the record says so);
folding in the tail of the moments launch was not built, so there is no measurement of it.  No target is set: the record states
what came out.  Prints one JSON line and writes it to --out.
Usage: python tools/bench_guidance.py [--rounds 5] [--out profiles/guidance_rescale.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import ops  # noqa: E402

CASES = {"base": dict(shape=(1, 4, 16, 40 * 64), batch=100), "vsr": dict(shape=(1, 4, 8, 320 * 512), batch=20)}
GUIDANCE, PHI, SCALE = 7.5, 0.7, 0.9
COEFFS = (0.5, 0.1, 0.2, 0.7, 0.0)      # contractive: the state stays bounded over thousands of in-place steps


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


def torch_step(eps, x, model_in):
    k_x, k_e, c_x0, c_xt, _ = COEFFS
    p = x.shape[0]
    e = eps.float()
    eu, ec = e[:p], e[p:]
    cfg = eu + GUIDANCE * (ec - eu)
    dims = list(range(1, x.dim()))
    f = PHI * (ec.std(dim=dims, keepdim=True) / cfg.std(dim=dims, keepdim=True)) + (1.0 - PHI)
    x0 = k_x * x - k_e * (f * cfg)
    x.copy_(c_xt * x + c_x0 * x0)
    h = (x * SCALE).half()
    model_in[:p] = h
    model_in[p:] = h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="A B B A rounds per pair and shape")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_guidance needs a HIP device"
    torch.cuda.set_device(0)
    res = {"metric": "guidance_rescale_step_cost", "family": "five-coefficient, guided, no step noise", "order": "A B B A",
           "fold": "own launch", "guidance": GUIDANCE, "rescale": PHI, "device": torch.cuda.get_device_name(0)}
    for name, case in CASES.items():
        shape, batch = case["shape"], case["batch"]
        p, per = shape[0], 1
        for d in shape[1:]:
            per *= d
        g = torch.Generator().manual_seed(0)
        x = torch.randn(shape, generator=g).cuda()
        eps = torch.randn((2 * p,) + shape[1:], generator=g).half().cuda()
        model_in = torch.empty_like(eps)
        table = torch.empty(p, 2, device="cuda")
        ws = torch.empty(ops.guidance_partials_floats(p, per), device="cuda")

        def run_table():
            for _ in range(batch):
                ops.guidance_table(eps, p, GUIDANCE, PHI, workspace=ws, out=table)
                ops.cfg_sampler_step_scaled(eps, x, None, model_in, table, COEFFS, SCALE)

        run_plain = lambda: [ops.cfg_ddpm_step(eps, x, None, model_in, GUIDANCE, COEFFS, SCALE) for _ in range(batch)]      # noqa: E731
        run_torch = lambda: [torch_step(eps, x, model_in) for _ in range(batch)]                                            # noqa: E731
        run_table(), run_plain(), run_torch()
        t1, pl = abba(run_table, run_plain, a.rounds)
        t2, to = abba(run_table, run_torch, a.rounds)
        assert torch.isfinite(x).all()
        us = lambda v: 1e3 * statistics.median(v) / batch       # noqa: E731
        n = p * per
        extra_bytes = 2 * n * 2                                  # the second read of both halves of eps2
        res[name] = {"shape": list(shape), "steps_per_sample": batch, "table_us": us(t1 + t2), "table_us_vs_plain": us(t1),
                     "plain_us": us(pl), "table_us_vs_torch": us(t2), "torch_us": us(to), "extra_us_over_plain": us(t1) - us(pl),
                     "torch_over_table": us(to) / us(t2), "extra_read_bytes": extra_bytes,
                     "table_us_all": [round(1e3 * v / batch, 3) for v in t1 + t2], "plain_us_all": [round(1e3 * v / batch, 3) for v in pl],
                     "torch_us_all": [round(1e3 * v / batch, 3) for v in to]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
