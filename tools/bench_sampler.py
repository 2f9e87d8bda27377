#!/usr/bin/env python3
"""Cost of the DPM-Solver++ multistep sampler.  COST ONLY: nothing here says that 20 steps give the quality of 50 (random-init
weights).

1. Step kernel: lavie_cfg_multistep_step (second-order form, history read) against lavie_cfg_sampler_step, at the base latent
   size (n = 4*16*40*64) and the VSR chunk size (n = 4*8*320*512), A B B A in one process, medians of device events over
   batches of launches.  `--parent-lib PATH` takes the five-coefficient kernel from another build of the library (the
   parent commit's); without it both kernels come from the library in use.
2. End to end at the bench shape (909 M-parameter base UNet, 16 x 40 x 64 latents, guidance 7.5): 50-step DDIM against
   20-step DPM-Solver++ 2M per video, A B B A.  `--vsr`: one 8-frame VSR chunk (320 x 512 latents) 50 against 20 steps.
Prints one JSON line (and writes it to --out).  Usage: python tools/bench_sampler.py [--parent-lib PATH] [--vsr] [--out profiles/dpmsolver.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lavie_amd import _lib, ops, spec  # noqa: E402

SIZES = {"base_4x16x40x64": 4 * 16 * 40 * 64, "vsr_chunk_4x8x320x512": 4 * 8 * 320 * 512}
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
    """Runs a b b a `rounds` times; returns the medians and all samples of each."""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(event_ms(a))
        tb.append(event_ms(b))
        tb.append(event_ms(b))
        ta.append(event_ms(a))
    return statistics.median(ta), statistics.median(tb), ta, tb


def kernel_leg(parent_path, rounds):
    lib = _lib.load()
    old = lib
    if parent_path:
        old = ctypes.CDLL(parent_path)
        sig = _lib.SIGNATURES["lavie_cfg_sampler_step"]
        old.lavie_cfg_sampler_step.restype, old.lavie_cfg_sampler_step.argtypes = sig
    out = {}
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, n in SIZES.items():
        g = torch.Generator().manual_seed(n)
        eps = torch.randn(2 * n, generator=g).half().cuda()
        x = torch.randn(n, generator=g).cuda()
        hist = torch.randn(n, generator=g).cuda()
        min_ = torch.empty(2 * n, dtype=torch.float16, device="cuda")
        # contractive coefficients: the state stays bounded over thousands of in-place launches
        new = lambda: [lib.lavie_cfg_multistep_step(p(eps), p(x), p(hist), p(min_), n, 7.5, 0.5, 0.1, 0.2, 0.7, 0.45, 1.0, stream)  # noqa: E731
                       for _ in range(BATCH)]
        ref = lambda: [old.lavie_cfg_sampler_step(p(eps), p(x), None, p(min_), n, 7.5, 0.5, 0.1, 0.2, 0.7, 0.0, 1.0, stream)  # noqa: E731
                       for _ in range(BATCH)]
        new(), ref()
        m_new, m_ref, s_new, s_ref = abba(new, ref, rounds)
        bytes_new, bytes_ref = n * (2 * 2 + 4 + 4 + 4 + 4 + 2 * 2), n * (2 * 2 + 4 + 4 + 2 * 2)
        out[name] = {"n": n, "multistep_us": 1e3 * m_new / BATCH, "five_coefficient_us": 1e3 * m_ref / BATCH,
                     "ratio": m_new / m_ref, "multistep_bytes": bytes_new, "five_coefficient_bytes": bytes_ref,
                     "multistep_GBps": bytes_new / (1e6 * m_new / BATCH), "five_coefficient_GBps": bytes_ref / (1e6 * m_ref / BATCH),
                     "multistep_us_all": [round(1e3 * v / BATCH, 3) for v in s_new],
                     "five_coefficient_us_all": [round(1e3 * v / BATCH, 3) for v in s_ref]}
        assert torch.isfinite(x).all()
    return out


def base_leg(rounds):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from lavie_amd.unet import UNet3DConditionModel
    dev = torch.device("cuda:0")
    sd = bench.synth_weights(spec.param_shapes(), 0)
    net = UNet3DConditionModel(sample_size=64, cross_attention_dim=768, init_weights=False)
    for name, prm in net.named_parameters():
        prm.data = sd[name].to(dev, torch.float16)
    del sd
    pe, ne, lat = bench.synth_inputs(0, dev)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=320, width=512, video_length=16, guidance_scale=7.5,
              output_type="latent")
    ddim = VideoGenPipeline(unet=net, scheduler=DDIMScheduler())
    dpm = VideoGenPipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
    a = lambda: ddim(num_inference_steps=50, **kw)      # noqa: E731
    b = lambda: dpm(num_inference_steps=20, **kw)       # noqa: E731
    ok = bool(torch.isfinite(a().video).all() and torch.isfinite(b().video).all())
    m_a, m_b, s_a, s_b = abba(a, b, rounds)
    del net
    torch.cuda.empty_cache()
    return {"ddim_50_steps_ms": m_a, "dpmsolver_20_steps_ms": m_b, "ratio": m_b / m_a, "steps_ratio": 20 / 50, "outputs_finite": ok,
            "ddim_50_steps_ms_all": s_a, "dpmsolver_20_steps_ms_all": s_b}


def vsr_leg(rounds):
    from lavie_amd import weights
    from lavie_amd.config import VSR_CONFIG
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from lavie_amd.vsr import UNet3DVSRModel, VideoUpscalePipeline
    dev = torch.device("cuda:0")
    sd = weights.synth_state_dict(spec.param_shapes(VSR_CONFIG), 0)
    net = UNet3DVSRModel(init_weights=False, sample_size=128, down_temporal_idx=(0, 1, 2, 3), mid_temporal=True,
                         up_temporal_idx=(0, 1, 2, 3))
    net.load_state_dict({k: v.half() for k, v in sd.items()})
    del sd
    net = net.to(dev, torch.float16)
    g = torch.Generator().manual_seed(0)
    frames = torch.randn(1, 3, 8, 320, 512, generator=g).clamp(-1, 1)
    pe, ne = torch.randn(1, 77, 1024, generator=g), torch.randn(1, 77, 1024, generator=g)
    lat = torch.randn(1, 4, 8, 320, 512, generator=g)
    kw = dict(image=frames, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=7.5, noise_level=150)
    ddim = VideoUpscalePipeline(unet=net, scheduler=DDIMScheduler())
    dpm = VideoUpscalePipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
    a = lambda: ddim(num_inference_steps=50, **kw)      # noqa: E731
    b = lambda: dpm(num_inference_steps=20, **kw)       # noqa: E731
    ok = bool(torch.isfinite(dpm(num_inference_steps=2, **kw).images).all())
    m_a, m_b, s_a, s_b = abba(a, b, rounds)
    return {"ddim_50_steps_ms": m_a, "dpmsolver_20_steps_ms": m_b, "ratio": m_b / m_a, "steps_ratio": 20 / 50, "outputs_finite": ok,
            "ddim_50_steps_ms_all": s_a, "dpmsolver_20_steps_ms_all": s_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="another build of liblavie_hip.so to take lavie_cfg_sampler_step from")
    ap.add_argument("--rounds", type=int, default=5, help="A B B A rounds of the kernel leg")
    ap.add_argument("--e2e-rounds", type=int, default=1)
    ap.add_argument("--vsr", action="store_true", help="also time one VSR chunk, 50 against 20 steps (about a minute)")
    ap.add_argument("--no-base", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sampler needs a HIP device"
    torch.cuda.set_device(0)
    res = {"metric": "dpmsolver_cost", "note": "cost only: equal quality at fewer steps is not claimed (random-init weights)",
           "five_coefficient_kernel_from": "parent library" if a.parent_lib else "library in use",
           "launches_per_sample": BATCH, "step_kernel": kernel_leg(a.parent_lib, a.rounds)}
    if not a.no_base:
        res["base_video"] = base_leg(a.e2e_rounds)
    if a.vsr:
        res["vsr_chunk"] = vsr_leg(a.e2e_rounds)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
