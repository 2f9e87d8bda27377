#!/usr/bin/env python3
"""Cost of the UniPC sampler.  COST ONLY: nothing here says what step count gives what quality (random-init weights).

1. / 2. Step kernel: lavie_cfg_unipc_step (the middle step: second-order corrector and predictor, all three histories read) against
   the same update composed from torch ops on the device (guidance, x0 prediction, corrector, predictor, the three history copies,
   the fp16 model input in both halves), at the base latent size [1, 4, 16, 40 x 64] and the VSR chunk size [1, 4, 8, 320 x 512].
3. One guided forward + step at the bench shape (909 M-parameter base UNet, 16 x 40 x 64 latents, guidance 7.5): a 2-step pipeline
   call with UniPC against the same call with DPM-Solver++ 2M, per step.
Every leg runs A B B A inside one process, medians of device events.  Prints one JSON line (and writes it to --out).
Usage: python tools/bench_unipc.py [--no-forward] [--out profiles/unipc.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from bench_sampler import abba  # noqa: E402
from lavie_amd import ops, spec  # noqa: E402

SIZES = {"base_1x4x16x40x64": 4 * 16 * 40 * 64, "vsr_chunk_1x4x8x320x512": 4 * 8 * 320 * 512}
BATCH = 50            # launches between two events
# contractive coefficients: the state stays bounded over thousands of in-place launches
MIDDLE = (0.5, 0.1, True, 0.4, 0.1, 0.05, -0.01, 0.5, 0.2, -0.05)
STEPS = 2


def torch_step(eps2, x, hist, model_in2, g, c, scale):
    k_x, k_e, _, c_l, c_0, c_1, c_2, p_x, p_0, p_1 = c
    n = x.numel()
    eu, ec = eps2[:n].float(), eps2[n:].float()
    eps = eu + g * (ec - eu)
    m = k_x * x - k_e * eps
    xc = c_l * hist[0] + c_0 * m + c_1 * hist[1] + c_2 * hist[2]
    xn = p_x * xc + p_0 * m + p_1 * hist[1]
    hist[0].copy_(xc)
    hist[2].copy_(hist[1])
    hist[1].copy_(m)
    x.copy_(xn)
    h = (xn * scale).half()
    model_in2[:n].copy_(h)
    model_in2[n:].copy_(h)


def kernel_leg(rounds):
    out = {}
    for name, n in SIZES.items():
        g = torch.Generator().manual_seed(n)
        eps = torch.randn(2 * n, generator=g).half().cuda()
        x = torch.randn(n, generator=g).cuda()
        hist = tuple(torch.randn(n, generator=g).cuda() for _ in range(3))
        min_ = torch.empty(2 * n, dtype=torch.float16, device="cuda")
        fused = lambda: [ops.cfg_unipc_step(eps, x, hist, min_, 7.5, MIDDLE, 1.0) for _ in range(BATCH)]      # noqa: E731
        composed = lambda: [torch_step(eps, x, hist, min_, 7.5, MIDDLE, 1.0) for _ in range(BATCH)]            # noqa: E731
        fused(), composed()
        m_f, m_c, s_f, s_c = abba(fused, composed, rounds)
        moved = n * (2 * 2 + 4 * 4 + 4 * 4 + 2 * 2)       # eps2 read; x, x_last, m1, m2 read and written; model_in2 written
        out[name] = {"n": n, "fused_us": 1e3 * m_f / BATCH, "torch_ops_us": 1e3 * m_c / BATCH, "ratio": m_f / m_c,
                     "fused_bytes": moved, "fused_GBps": moved / (1e6 * m_f / BATCH),
                     "fused_us_all": [round(1e3 * v / BATCH, 3) for v in s_f], "torch_ops_us_all": [round(1e3 * v / BATCH, 3) for v in s_c]}
        assert torch.isfinite(x).all()
    return out


def forward_leg(rounds):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from lavie_amd.scheduling_unipc_multistep import UniPCMultistepScheduler
    from lavie_amd.unet import UNet3DConditionModel
    dev = torch.device("cuda:0")
    sd = bench.synth_weights(spec.param_shapes(), 0)
    net = UNet3DConditionModel(sample_size=64, cross_attention_dim=768, init_weights=False)
    for name, prm in net.named_parameters():
        prm.data = sd[name].to(dev, torch.float16)
    del sd
    pe, ne, lat = bench.synth_inputs(0, dev)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=320, width=512, video_length=16, guidance_scale=7.5,
              output_type="latent", num_inference_steps=STEPS)
    uni = VideoGenPipeline(unet=net, scheduler=UniPCMultistepScheduler())
    dpm = VideoGenPipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
    a, b = (lambda: uni(**kw)), (lambda: dpm(**kw))
    ok = bool(torch.isfinite(a().video).all() and torch.isfinite(b().video).all())
    a(), b()
    m_a, m_b, s_a, s_b = abba(a, b, rounds)
    return {"steps_per_call": STEPS, "unipc_ms_per_step": m_a / STEPS, "dpmsolver_ms_per_step": m_b / STEPS, "ratio": m_a / m_b,
            "outputs_finite": ok, "unipc_ms_all": s_a, "dpmsolver_ms_all": s_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="A B B A rounds of each leg")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_unipc needs a HIP device"
    torch.cuda.set_device(0)
    res = {"metric": "unipc_cost", "note": "cost only: no quality at a given step count is claimed (random-init weights)",
           "launches_per_sample": BATCH, "step_kernel": kernel_leg(a.rounds)}
    if not a.no_forward:
        res["forward_plus_step"] = forward_leg(a.rounds)
        fwd = res["forward_plus_step"]["unipc_ms_per_step"]
        res["step_share_of_forward_plus_step"] = res["step_kernel"]["base_1x4x16x40x64"]["fused_us"] / (1e3 * fwd)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
