#!/usr/bin/env python3
"""Cost of the two ends of the denoising-loss evaluation.  COST ONLY: the feature's guarantees are the addressing
and the fixed summation order, not a speed.

At two shapes, latents [8, 4, 16, 40*64] and [2, 4, 61, 40*64], v-prediction (the target that reads both operands), each end is timed as
  (a) torch   the same end composed from torch ops on the device:
              front: ops.philox_normal into a buffer, sqrt(abar) x0 + sqrt(1 - abar) noise in fp32 (add_noise), the fp16 copy
              back:  get_velocity = a noise - s x0 from the materialised noise, mse_loss(pred.float(), target, "none").mean per latent
  (b) fused   ops.noisy_latents / ops.denoising_loss: one launch, and two small ones; no noise, fp32 noisy, target or squared-difference
              tensor exists
in one process, in the order a b b a per round, medians of device events over batches of back-to-back calls (microseconds per call,
launch overhead included).  The working set is re-run in place, so a time may include hits in the last-level cache.  Beside them, for
scale, one whole `DenoisingLoss.evaluate` at the first shape on the full base UNet with synthetic weights (--no-model leaves it out).
Prints one JSON line and writes it to --out.
Usage: python tools/bench_denoising_loss.py [--rounds 5] [--out profiles/denoising_loss.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lavie_amd import ops  # noqa: E402
from lavie_amd.denoising_loss import DenoisingLoss, noise_levels  # noqa: E402
from lavie_amd.noise import PhiloxGenerator  # noqa: E402
from lavie_amd.scheduling_ddpm import DDPMScheduler  # noqa: E402

CASES = {"base": dict(shape=(8, 4, 16, 40, 64), batch=50), "interp": dict(shape=(2, 4, 61, 40, 64), batch=50)}
KIND = "v_prediction"


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def abba(runs, rounds, batch):
    for fn in runs.values():                # warm-up: every code object loaded, every shape seen
        fn()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k in ("a", "b", "b", "a"):
            times[k].append(event_ms(runs[k]))
    us = {k: 1e3 * statistics.median(v) / batch for k, v in times.items()}
    return us, {k: [round(1e3 * t / batch, 3) for t in v] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="a b b a rounds per shape and end")
    ap.add_argument("--no-model", action="store_true", help="leave out the whole evaluate on the full UNet")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_denoising_loss needs a HIP device"
    torch.cuda.set_device(0)
    sch = DDPMScheduler()
    res = {"metric": "denoising_loss_ends_cost", "order": "a b b a", "kind": KIND,
           "variants": {"a": "torch ops on the device (philox_normal + add_noise + cast; get_velocity + mse_loss)",
                        "b": "fused (noisy_latents; denoising_loss)"},
           "device": torch.cuda.get_device_name(0)}
    for name, case in CASES.items():
        shape, batch = case["shape"], case["batch"]
        p = shape[0]
        per = 1
        for d in shape[1:]:
            per *= d
        g = torch.Generator().manual_seed(0)
        x0 = torch.randn(shape, generator=g).cuda()
        pred = torch.randn(shape, generator=g).half().cuda()
        seeds = list(range(100, 100 + p))
        ts = [(37 + 113 * i) % 1000 for i in range(p)]
        levels = noise_levels(sch, ts)
        lv = torch.tensor(levels, dtype=torch.float32, device="cuda")
        a_dev, s_dev = lv[:, 0].reshape(-1, 1, 1, 1, 1), lv[:, 1].reshape(-1, 1, 1, 1, 1)
        noise = torch.empty(shape, dtype=torch.float32, device="cuda")
        model_in = torch.empty(shape, dtype=torch.float16, device="cuda")
        out = torch.empty(p, dtype=torch.float32, device="cuda")
        ws = torch.empty(ops.denoising_loss_workspace_floats(p, per), dtype=torch.float32, device="cuda")
        draw = [0]

        def next_draw():
            draw[0] += 1
            return draw[0]

        def front_a():
            for _ in range(batch):
                ops.philox_normal(seeds, per, next_draw(), out=noise)
                (a_dev * x0 + s_dev * noise).half()

        def front_b():
            for _ in range(batch):
                ops.noisy_latents(x0, seeds, next_draw(), levels, out=model_in)

        def back_a():
            for _ in range(batch):
                target = a_dev * noise - s_dev * x0
                torch.nn.functional.mse_loss(pred.float(), target, reduction="none").mean(dim=(1, 2, 3, 4))

        def back_b():
            for _ in range(batch):
                ops.denoising_loss(pred, x0, seeds, draw[0], levels, KIND, workspace=ws, out=out)

        entry = {"shape": list(shape), "calls_per_sample": batch}
        for end, runs in (("front", {"a": front_a, "b": front_b}), ("back", {"a": back_a, "b": back_b})):
            us, every = abba(runs, a.rounds, batch)
            entry[end] = {"torch_us": us["a"], "fused_us": us["b"], "fused_over_torch": us["b"] / us["a"], "all_us": every}
        assert torch.isfinite(out).all()
        res[name] = entry
    if not a.no_model:
        from lavie_amd import spec, weights
        from lavie_amd.unet import UNet3DConditionModel
        shape = CASES["base"]["shape"]
        sd = weights.synth_state_dict(spec.param_shapes(), 0)
        net = UNet3DConditionModel(sample_size=64, cross_attention_dim=768, init_weights=False)
        net.load_state_dict({k: v.half() for k, v in sd.items()})
        del sd
        net = net.to("cuda", torch.float16)
        g = torch.Generator().manual_seed(1)
        x0 = torch.randn(shape, generator=g).cuda()
        ctx = torch.randn(shape[0], 77, 768, generator=g).half().cuda()
        scorer = DenoisingLoss(net, sch, prediction_type=KIND)
        ts = [(37 + 113 * i) % 1000 for i in range(shape[0])]
        gen = PhiloxGenerator(7)
        scorer.evaluate(x0, ctx, ts, gen)                      # warm-up: engine finalised, workspaces planned
        times = [event_ms(lambda: scorer.evaluate(x0, ctx, ts, gen)) for _ in range(3)]
        res["evaluate"] = {"shape": list(shape), "ms": statistics.median(times), "all_ms": [round(t, 3) for t in times],
                           "note": "one whole evaluate: noisy_latents, the UNet forward of 8 latents, denoising_loss, the host reduction"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
