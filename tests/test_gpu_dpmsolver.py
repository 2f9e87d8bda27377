"""DPM-Solver++ multistep sampler on the GPU: the fused step kernel against its fp32 / float64 forms, and the two pipelines with
the new scheduler against test-side loops around the fp32 oracles."""
import pytest
import torch

import dpm_reference as R
import golden_util as G
from gpu_util import rel_l2
from test_gpu_engine import SMALL_KW, build, ocfg_small

pytestmark = pytest.mark.gpu

# tolerance of the existing multi-step pipeline tests on the same small models, DDIM through the fused step kernel against the
# fp32 oracle loop: tests/test_gpu_engine.py::test_pipeline_ddim_scheduler and tests/test_gpu_vsr.py::test_vsr_pipeline_loop_vs_oracle
TOL_PIPELINE = 3e-2

COEFFS = {"second order": (1.0206, 0.2041, 0.1234, 0.8803, 0.4712), "first order": (1.0206, 0.2041, 0.1234, 0.8803, 0.0),
          "final": (1.0001, 0.0100, 1.0, 0.0, 0.0), "v_prediction": (0.7071, 0.7071, 0.3000, 0.7200, 0.6500),
          "sample": (0.0, -1.0, 0.2500, 0.7400, 0.3000)}
# vector body + ragged tail (unguided), whole blocks, one lane, the one-element-per-lane form under guidance (n % 8 != 0)
SIZES = (1, 7, 8, 1000, 2048, 2049, 4 * 4 * 8 * 8, 8 * 2051 + 5, 4 * 16 * 40 * 64)


def _inputs(n, seed, guided):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((2 if guided else 1) * n, generator=g).half()
    x = torch.randn(n, generator=g) * 3.0
    hist = torch.randn(n, generator=g)
    return eps, x, hist


def _run(eps, x, hist, guided, coeffs, scale, guidance=7.5):
    from lavie_amd import ops
    n = x.numel()
    e, xd, hd = eps.cuda(), x.cuda().clone(), hist.cuda().clone()
    min_ = torch.full(((2 if guided else 1) * n,), float("nan"), dtype=torch.float16, device="cuda")
    if guided:
        ops.cfg_multistep_step(e, xd, hd, min_, guidance, coeffs, scale)
    else:
        ops.multistep_step(e, xd, hd, min_, coeffs, scale)
    torch.cuda.synchronize()
    return xd, hd, min_


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("name", list(COEFFS))
def test_step_kernel_vs_fp32_and_float64_forms(name, guided):
    """Kernel against the update evaluated in float64 from the kernel's own inputs, per element:
        |x0_kernel - x0_f64| <= 8 * 2^-24 * M0,   |x'_kernel - x'_f64| <= 16 * 2^-24 * M
    where M0 / M are the sums of the magnitudes of the terms of x0 / x' (dpm_reference.kernel_form_f64).  Derivation
    (dpm_reference.py): any fp32 evaluation of the update is a chain of at most 6 (x0) / 12 (x') roundings of relative size
    2^-24, each acting on an intermediate no larger than those sums; 8 / 16 leave room for second-order terms and for the
    final rounding.  Fusing a multiply-add only removes roundings, so the kernel's fused form and torch's unfused fp32 form
    both obey it; the torch form is held to the same bound here, which checks the bound against the reference's own error.
    In units of the fp32 spacing of M this is 'a few ulp'.  model_in is exactly fp16(x' * scale) of the kernel's own x', and
    its two halves are bit-equal under guidance."""
    coeffs, scale, guidance = COEFFS[name], 0.8125 if name != "final" else 1.0, 7.5
    worst = {}
    for n in SIZES:
        eps, x, hist = _inputs(n, n, guided)
        xd, hd, min_ = _run(eps, x, hist, guided, coeffs, scale, guidance)
        eu, ec = (eps[:n], eps[n:]) if guided else (eps, None)
        x0_64, xn_64, m0, m = R.kernel_form_f64(eu, ec, x, hist, guidance, coeffs)
        x0_32, xn_32 = R.torch_form_f32(eu, ec, x, hist, guidance, coeffs)
        for what, got, ref, mag, k in (("x0 kernel", hd.cpu(), x0_64, m0, R.X0_ROUNDINGS), ("x' kernel", xd.cpu(), xn_64, m, R.XN_ROUNDINGS),
                                       ("x0 torch", x0_32, x0_64, m0, R.X0_ROUNDINGS), ("x' torch", xn_32, xn_64, m, R.XN_ROUNDINGS)):
            ratio = ((got.double() - ref).abs() / (R.U32 * mag).clamp_min(1e-300)).max().item()
            worst[what] = max(worst.get(what, 0.0), ratio)
            assert ratio <= k, (what, n, ratio)
        want = (xd * scale).half()
        assert torch.equal(min_[:n], want), n
        if guided:
            assert torch.equal(min_[n:], want), n
    print(name, "guided" if guided else "unguided", "max error in units of 2^-24 M:", {k: f"{v:.2f}" for k, v in worst.items()})


@pytest.mark.parametrize("guided", [True, False])
def test_poisoned_history_is_never_read_when_c_prev_is_zero(guided):
    """c_prev = 0 (first step, final step, order 1): a history full of NaN gives finite output bit-equal to a zero history,
    and the history comes back holding x0.  With c_prev != 0 the same poison does reach the output (the test can see it)."""
    for n in (8 * 2051 + 5, 4096):
        eps, x, hist = _inputs(n, 3, guided)
        nan = torch.full_like(hist, float("nan"))
        for name in ("first order", "final"):
            a = _run(eps, x, nan, guided, COEFFS[name], 0.9)
            b = _run(eps, x, torch.zeros_like(hist), guided, COEFFS[name], 0.9)
            assert all(torch.isfinite(t.float()).all() for t in a)
            assert all(torch.equal(p, q) for p, q in zip(a, b))
        seen = _run(eps, x, nan, guided, COEFFS["second order"], 0.9)
        assert torch.isnan(seen[0]).all() and torch.isfinite(seen[1]).all()


def test_first_order_is_bit_equal_to_the_five_coefficient_kernel():
    """With c_prev = 0 and the same coefficients the new kernel's x is bit-equal to lavie_cfg_sampler_step with sigma = 0 (the
    multistep kernel spells out the rounding points that kernel compiles to, elementwise.hip), and so is model_in at
    next_input_scale = 1, the scale of every scheduler that reaches this kernel.
    At a scale != 1 bit-equality of model_in is impossible by construction: the five-coefficient kernel's scale-and-convert
    compiles to one v_fma_mixlo_f16, which rounds the exact product x' * scale once, to fp16; the new kernel is held to
    fp16(fp32(x' * scale)) exactly (the test above), which rounds twice.  The two differ where the fp32 rounding moves the
    product across an fp16 rounding boundary: there, by one fp16 ulp.  So at scale != 1: x bit-equal, model_in within one fp16
    spacing of the value, on every element."""
    from lavie_amd import ops
    for n in (4 * 4 * 8 * 8, 8 * 2051 + 5, 4 * 16 * 40 * 64):
        for name in ("first order", "final", "v_prediction", "sample"):
            for scale in (1.0, 0.8125):
                coeffs = COEFFS[name][:4] + (0.0,)
                eps, x, hist = _inputs(n, 17, True)
                xd, _, min_ = _run(eps, x, hist, True, coeffs, scale)
                xo = x.cuda().clone()
                mo = torch.empty(2 * n, dtype=torch.float16, device="cuda")
                ops.cfg_ddpm_step(eps.cuda(), xo, None, mo, 7.5, coeffs, scale)
                assert torch.equal(xd, xo), (n, name, scale)
                if scale == 1.0:
                    assert torch.equal(min_, mo), (n, name)
                else:
                    differ = int((min_ != mo).sum())
                    spacing = torch.maximum(mo.float().abs(), torch.tensor(2.0 ** -14, device="cuda")) * 2.0 ** -10
                    print(f"n={n} {name}: model_in differs from the five-coefficient kernel on {differ} of {2 * n} elements")
                    assert ((min_.float() - mo.float()).abs() <= spacing).all(), (n, name)


def test_step_kernel_two_runs_bit_identical():
    for guided in (True, False):
        eps, x, hist = _inputs(4 * 16 * 40 * 64, 5, guided)
        a = _run(eps, x, hist, guided, COEFFS["second order"], 0.9)
        b = _run(eps, x, hist, guided, COEFFS["second order"], 0.9)
        assert all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------ VideoGenPipeline
@pytest.fixture(scope="module")
def small():
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    cfg = UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    sd = G.synth16(spec.param_shapes(cfg), 11)
    return build(sd, **SMALL_KW), sd


def _oracle_loop(sd, lat, pe, ne, steps, guidance):
    """Test-side fp32 loop: oracle UNet + the scheduler's own plain-torch step()."""
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from oracle import unet_fp32 as O
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(steps)
    x = lat.clone()
    for t in [int(v) for v in sch.timesteps]:
        if guidance > 1.0:
            ctx = torch.cat([ne, pe]).half().float()
            eps = O.unet_forward(sd, torch.cat([x, x]).half().float(), t, ctx, ocfg_small())
            p = x.shape[0]
            eps = eps[:p] + guidance * (eps[p:] - eps[:p])
        else:
            eps = O.unet_forward(sd, x.half().float(), t, pe.half().float(), ocfg_small())
        x = sch.step(eps, t, x).prev_sample
    return x


def test_pipeline_20_guided_steps_vs_oracle_loop(small):
    """20 guided steps through VideoGenPipeline(sample_method = dpmsolver++) against the fp32 loop, under the tolerance of the
    DDIM pipeline test on the same model; a callback sees the scheduler's timesteps; the run is deterministic."""
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, sd = small
    pipe, _, _ = VideoGenPipeline.from_sample_yaml(dict(sample_method="dpmsolver++"), unet=net)
    g = torch.Generator().manual_seed(19)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    seen = []
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4,
              num_inference_steps=20, guidance_scale=7.5, output_type="latent")
    out = pipe(callback=lambda i, t, x: seen.append(t), **kw).video.float().cpu()
    assert seen == [951 - 50 * i for i in range(20)]
    ref = _oracle_loop(sd, lat, pe, ne, 20, 7.5)
    err = rel_l2(out, ref)
    print(f"20 guided steps: rel-L2 vs oracle loop {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL_PIPELINE
    assert torch.equal(pipe(**kw).video.float().cpu(), out)
    # a CPU generator changes nothing: the solver draws no noise
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(1), **kw).video.float().cpu(), out)


def test_pipeline_without_guidance_and_generator_list(small):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    net, sd = small
    pipe = VideoGenPipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
    g = torch.Generator().manual_seed(23)
    pe = torch.randn(2, 77, 128, generator=g)
    lat = torch.randn(2, 4, 4, 8, 8, generator=g)
    kw = dict(prompt_embeds=pe, height=64, width=64, video_length=4, num_inference_steps=20, guidance_scale=1.0, output_type="latent")
    out = pipe(latents=lat, **kw).video.float().cpu()
    err = rel_l2(out, _oracle_loop(sd, lat, pe, None, 20, 1.0))
    print(f"20 unguided steps: rel-L2 vs oracle loop {err:.3e}")
    assert err < TOL_PIPELINE
    # a list of generators, one per latent: the initial latents come from them, each latent from its own
    gl = lambda: [torch.Generator().manual_seed(31), torch.Generator().manual_seed(32)]
    o2 = pipe(generator=gl(), **kw).video.float().cpu()
    lat2 = torch.cat([torch.randn(1, 4, 4, 8, 8, generator=q) for q in gl()])
    assert torch.equal(o2, pipe(latents=lat2, **kw).video.float().cpu())
    with pytest.raises(ValueError):
        pipe(generator=[torch.Generator()], **kw)


def test_pipeline_with_graph_is_bit_equal_to_eager(small):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    net, _ = small
    g = torch.Generator().manual_seed(44)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)

    def run():
        pipe = VideoGenPipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), num_inference_steps=20, guidance_scale=7.5,
                    output_type="latent", video_length=4, height=64, width=64).video.clone()

    eager = run()
    net.enable_graph(True)
    try:
        graphed = run()
    finally:
        net.enable_graph(False)
    assert torch.equal(eager, graphed)


# ------------------------------------------------------------------ VideoUpscalePipeline
def test_vsr_pipeline_two_chunks_vs_oracle_loop_and_fresh_history():
    """VideoUpscalePipeline on the small VSR model, 12 frames = two chunks (8 + 4), DPM-Solver++: each chunk against the
    test-side fp32 loop (oracle VSR UNet + the scheduler's step()) under the VSR pipeline test's tolerance, and chunk 2 bit-equal
    to the same frames through a fresh pipeline and scheduler, i.e. it saw nothing of chunk 1's history."""
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from lavie_amd.vsr import VideoUpscalePipeline, upscale_in_chunks
    from oracle import vsr_blocks as V
    from oracle.vsr_loop import add_low_res_noise
    from test_gpu_vsr import SMALL_VSR, build_vsr
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    cfg = UNetConfig(in_channels=7, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(False, True),
                     layers_per_block=1, vsr_blocks=True, only_cross_attention=(True, False), vsr_temporal_modules=True,
                     num_class_embeds=1000)
    sd = G.synth16(spec.param_shapes(cfg), 31)
    net = build_vsr(sd, **SMALL_VSR)
    steps, guidance, level = 6, 9.0, 20
    g = torch.Generator().manual_seed(77)
    pe, ne = torch.randn(1, 77, 128, generator=g).half().float(), torch.randn(1, 77, 128, generator=g).half().float()
    frames = torch.randn(1, 3, 12, 8, 8, generator=g).clamp(-1, 1)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=steps, guidance_scale=guidance, noise_level=level)
    pipe = VideoUpscalePipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
    up = upscale_in_chunks(pipe, frames, short_seq=8, generator=torch.Generator().manual_seed(5), **kw).float().cpu()
    assert up.shape == (1, 4, 12, 8, 8) and torch.isfinite(up).all()

    # the same host draws, chunk by chunk: low-res noise, then the initial latents (VideoUpscalePipeline.__call__)
    gen = torch.Generator().manual_seed(5)
    unet = lambda x, low, t, ctx, labels: V.vsr_unet_forward(sd, x, low, t, ctx, labels, block_out_channels=(256, 512),
                                                            attn_levels=(False, True), only_cross_attention=(True, False),
                                                            layers_per_block=1, heads=8)
    chunk_inputs = []
    for lo, hi in ((0, 8), (8, 12)):
        part = frames[:, :, lo:hi]
        noise = torch.randn(part.shape, generator=gen)
        lat = torch.randn(1, 4, hi - lo, 8, 8, generator=gen)
        chunk_inputs.append((part, lat))
        img = add_low_res_noise(part, noise, level)
        sch = DPMSolverMultistepScheduler()
        sch.set_timesteps(steps)
        ctx, low = torch.cat([ne, pe]), torch.cat([img, img])
        labels = torch.full((2,), level, dtype=torch.long)
        x = lat
        for t in [int(v) for v in sch.timesteps]:
            eps = unet(torch.cat([x, x]).half().float(), low.half().float(), t, ctx, labels)
            x = sch.step(eps[:1] + guidance * (eps[1:] - eps[:1]), t, x).prev_sample
        err = rel_l2(up[:, :, lo:hi], x)
        print(f"VSR chunk frames {lo}:{hi}: rel-L2 vs oracle loop {err:.3e}")
        assert err < TOL_PIPELINE, (lo, hi)
    # chunk 2 alone through a fresh pipeline, same draws: bit-equal, so no history crossed the chunk boundary
    gen = torch.Generator().manual_seed(5)
    torch.randn(chunk_inputs[0][0].shape, generator=gen)
    torch.randn(chunk_inputs[0][1].shape, generator=gen)
    fresh = VideoUpscalePipeline(unet=net, scheduler=DPMSolverMultistepScheduler())
    alone = fresh(image=chunk_inputs[1][0], generator=gen, **kw).images.float().cpu()
    assert torch.equal(alone, up[:, :, 8:12])
