"""Sampling long clips as overlapping frame windows on the GPU: lavie_window_step (csrc/sampler_window.hip) per element against its
float64 form, its exact properties (one window is the plain kernel, a frame under one window has the plain kernel's bits, all
windows that share a frame receive one fp16 value), and the windowed pipelines against plain runs and a test-side fp32 loop
around the oracle UNet."""
import pytest
import torch

import golden_util as G
import window_reference as W
from gpu_util import rel_l2
from test_gpu_dpmsolver import TOL_PIPELINE
from test_gpu_engine import SMALL_KW, build, ocfg_small

pytestmark = pytest.mark.gpu

# (P, C, hw): one element; the one-element form across videos and channels; the smallest eight-element form; more than one block
# per plane; ragged, more than one block
SHAPES = ((1, 1, 1), (2, 3, 7), (2, 4, 8), (2, 4, 8 * 33), (1, 4, 2051))
# (F, L, starts): one window; two windows overlapping in 3 frames; cover count 3; three windows that only touch
SCHEDULES = ((4, 4, (0,)), (13, 8, (0, 5)), (10, 6, (0, 2, 4)), (9, 3, (0, 3, 6)))
ENTRIES = {"cfg_five": ("five", True), "five": ("five", False), "cfg_multistep": ("multistep", True), "multistep": ("multistep", False)}
# fifth coefficient: sigma of the step's own noise (five-coefficient family) / c_prev (multistep family), both non-zero and zero
COEFFS = {"five": ((1.0206, 0.2041, 0.1234, 0.8803, 0.35), (1.0206, 0.2041, 0.1234, 0.8803, 0.0)),
          "multistep": ((1.0206, 0.2041, 0.1234, 0.8803, 0.4712), (1.0206, 0.2041, 0.1234, 0.8803, 0.0))}
GUIDANCE, SCALE = 7.5, 0.8125


def make_inputs(pchw, sched, seed, guided):
    p, c, hw = pchw
    frames, length, starts = sched
    g = torch.Generator().manual_seed(seed)
    nb = 2 * p if guided else p
    return dict(eps=[torch.randn(nb, c, length, hw, generator=g).half() for _ in starts],
                x=torch.randn(p, c, frames, hw, generator=g) * 3.0, hist=torch.randn(p, c, frames, hw, generator=g),
                nz=torch.randn(p, c, frames, hw, generator=g))


def run(entry, d, sched, profile, coeffs, scale):
    """One launch on NaN-filled outputs.  Returns (x, x0_prev or None, [model_in per window]) on the device."""
    from lavie_amd import ops
    family, guided = ENTRIES[entry]
    x = d["x"].cuda().clone()
    min_ = [torch.full(e.shape, float("nan"), dtype=torch.float16, device="cuda") for e in d["eps"]]
    if family == "five":
        aux, hist = (d["nz"].cuda() if coeffs[4] != 0.0 else None), None
    else:
        aux = hist = d["hist"].cuda().clone() if coeffs[4] != 0.0 else torch.full_like(x, float("nan"))   # c_prev = 0 never reads it
    ops.window_step([e.cuda() for e in d["eps"]], x, aux, min_, sched[2], profile, GUIDANCE if guided else None, coeffs, scale,
                    multistep=family == "multistep")
    torch.cuda.synchronize()
    return x, hist, min_


def run_plain(entry, eps, x, aux, coeffs, scale):
    """The plain kernel of the family on one tensor [P, C, F, hw] (cfg_ddpm_step, sampler_step, cfg_multistep_step, multistep_step)."""
    from lavie_amd import ops
    family, guided = ENTRIES[entry]
    x = x.cuda().contiguous().clone()
    min_ = torch.full(eps.shape, float("nan"), dtype=torch.float16, device="cuda")
    hist = None
    if family == "five":
        nz = aux.cuda().contiguous() if coeffs[4] != 0.0 else None
        if guided:
            ops.cfg_ddpm_step(eps.cuda(), x, nz, min_, GUIDANCE, coeffs, scale)
        else:
            ops.sampler_step(eps.cuda(), x, nz, min_, coeffs, scale)
    else:
        hist = aux.cuda().contiguous().clone() if coeffs[4] != 0.0 else torch.full_like(x, float("nan"))
        if guided:
            ops.cfg_multistep_step(eps.cuda(), x, hist, min_, GUIDANCE, coeffs, scale)
        else:
            ops.multistep_step(eps.cuda(), x, hist, min_, coeffs, scale)
    torch.cuda.synchronize()
    return x, hist, min_


def profile_of(kind, length):
    from lavie_amd.windows import window_profile
    return window_profile(length, kind)


# ------------------------------------------------------------------ 1. per element
@pytest.mark.parametrize("kind", ["uniform", "triangle"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_window_step_per_element_vs_float64(entry, kind):
    """Both families with and without guidance, fifth coefficient non-zero and zero, on every shape and schedule, every output
    pre-filled with NaN (the multistep history too when c_prev = 0) and fully finite afterwards, against the step evaluated in
    float64 from the kernel's own inputs: |got - f64| <= K * 2^-24 * M with M the sum of term magnitudes and K twice the number of
    fp32 roundings of the spelled-out form for the frame's cover count (window_reference.py).  The unfused torch fp32 form is held
    to the same bound.  Every window's model_in is exactly fp16 of the kernel's own x' times the scale, rounded as the family's
    plain kernel rounds it, in both guidance halves."""
    family, guided = ENTRIES[entry]
    worst = {}
    for pchw in SHAPES:
        for sched in SCHEDULES:
            frames, length, starts = sched
            profile = profile_of(kind, length)
            for ci, coeffs in enumerate(COEFFS[family]):
                d = make_inputs(pchw, sched, 1000 * pchw[2] + 10 * frames + ci, guided)
                aux = d["nz"] if family == "five" else d["hist"]
                g = GUIDANCE if guided else None
                x, hist, min_ = run(entry, d, sched, profile, coeffs, SCALE)
                xn64, mag, h64, hmag = W.window_form_f64(family, d["eps"], d["x"], aux, starts, profile, g, coeffs)
                xn32, h32 = W.torch_form_f32(family, d["eps"], d["x"], aux, starts, profile, g, coeffs)
                k = W.bound_k(family, frames, length, starts)
                checks = [("x' kernel", x.cpu(), xn64, mag, k), ("x' torch", xn32, xn64, mag, k)]
                if family == "multistep":
                    kh = W.bound_k("history", frames, length, starts)
                    checks += [("x0 kernel", hist.cpu(), h64, hmag, kh), ("x0 torch", h32, h64, hmag, kh)]
                for what, got, ref, m, kk in checks:
                    assert torch.isfinite(got).all(), (what, pchw, sched)
                    ratio = (got.double() - ref).abs() / (W.U32 * m).clamp_min(1e-300)
                    worst[what] = max(worst.get(what, 0.0), (ratio / kk).max().item())
                    assert (ratio <= kk).all(), (what, pchw, sched, coeffs, ratio.max().item())
                rounded = W.twice_rounded_f16 if family == "multistep" else W.once_rounded_f16
                p = pchw[0]
                for w, s in enumerate(starts):
                    want = rounded(x[:, :, s:s + length], SCALE)
                    assert torch.isfinite(min_[w].float()).all(), (pchw, sched, w)
                    assert torch.equal(min_[w][:p].cpu(), want), (pchw, sched, coeffs, w)
                    if guided:
                        assert torch.equal(min_[w][p:], min_[w][:p]), (pchw, sched, coeffs, w)
    print(entry, kind, "max error as a fraction of the bound K 2^-24 M:", {k: f"{v:.3f}" for k, v in worst.items()})


# ------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_one_window_is_the_plain_kernel_bit_for_bit(entry):
    """One window with s = 0, L = F: x, aux and model_in are bit-equal to the plain kernel of the family."""
    family, _ = ENTRIES[entry]
    for pchw in SHAPES:
        for frames in (4, 7):
            sched = (frames, frames, (0,))
            for kind in ("uniform", "triangle"):
                for coeffs in COEFFS[family]:
                    d = make_inputs(pchw, sched, 31 + pchw[2] + frames, ENTRIES[entry][1])
                    got = run(entry, d, sched, profile_of(kind, frames), coeffs, SCALE)
                    ref = run_plain(entry, d["eps"][0], d["x"], d["nz"] if family == "five" else d["hist"], coeffs, SCALE)
                    for name, a, b in zip(("x", "x0_prev", "model_in"), (got[0], got[1], got[2][0]), ref):
                        if a is not None:
                            assert torch.isfinite(a.float()).all() and torch.equal(a, b), (name, pchw, frames, kind, coeffs)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_frames_under_one_window_have_the_plain_kernels_bits(entry):
    """In an overlapped schedule the frames covered once are bit-equal to the plain kernel run on that window alone; the windows
    that share a frame hold bit-equal fp16; the guidance halves are bit-equal."""
    family, guided = ENTRIES[entry]
    for pchw in SHAPES[1:]:
        for sched in ((13, 8, (0, 5)), (10, 6, (0, 2, 4))):
            frames, length, starts = sched
            cover = W.cover_count(frames, length, starts)
            for coeffs in COEFFS[family]:
                d = make_inputs(pchw, sched, 77 + pchw[2], guided)
                aux = d["nz"] if family == "five" else d["hist"]
                x, hist, min_ = run(entry, d, sched, profile_of("triangle", length), coeffs, SCALE)
                p = pchw[0]
                for w, s in enumerate(starts):
                    px, ph, pm = run_plain(entry, d["eps"][w], d["x"][:, :, s:s + length], aux[:, :, s:s + length], coeffs, SCALE)
                    once = [f for f in range(s, s + length) if cover[f] == 1]
                    assert once or sched[0] == 10                        # (10, 6, [0, 2, 4]): the middle window has no frame of its own
                    for f in once:
                        assert torch.equal(x[:, :, f], px[:, :, f - s]), (pchw, sched, w, f)
                        assert torch.equal(min_[w][:, :, f - s], pm[:, :, f - s]), (pchw, sched, w, f)
                        if hist is not None:
                            assert torch.equal(hist[:, :, f], ph[:, :, f - s]), (pchw, sched, w, f)
                    if guided:
                        assert torch.equal(min_[w][:p], min_[w][p:])
                    for v in range(w + 1, len(starts)):                  # frames shared with a later window
                        for f in range(starts[v], min(s + length, starts[v] + length)):
                            assert torch.equal(min_[w][:, :, f - s], min_[v][:, :, f - starts[v]]), (pchw, sched, w, v, f)


def test_two_runs_are_bit_identical():
    sched = (13, 8, (0, 5))
    for entry in ENTRIES:
        d = make_inputs((2, 4, 8 * 33), sched, 3, ENTRIES[entry][1])
        coeffs = COEFFS[ENTRIES[entry][0]][0]
        a = run(entry, d, sched, profile_of("triangle", 8), coeffs, SCALE)
        b = run(entry, d, sched, profile_of("triangle", 8), coeffs, SCALE)
        assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2])), entry
        assert a[1] is None or torch.equal(a[1], b[1]), entry


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_poisoned_window_poisons_exactly_the_frames_it_covers(entry):
    """A window's eps has no frames outside [s_w, s_w + L) by construction; what can be checked is that NaN in ALL of one window's
    eps reaches exactly the frames that window covers, in x and in every window's model_in, and no others."""
    family, guided = ENTRIES[entry]
    for pchw in ((2, 3, 7), (2, 4, 8 * 33)):
        for sched, bad in (((13, 8, (0, 5)), 1), ((10, 6, (0, 2, 4)), 0), ((9, 3, (0, 3, 6)), 1)):
            frames, length, starts = sched
            d = make_inputs(pchw, sched, 5 + pchw[2], guided)
            d["eps"][bad] = torch.full_like(d["eps"][bad], float("nan"))
            x, hist, min_ = run(entry, d, sched, profile_of("uniform", length), COEFFS[family][0], SCALE)
            hit = torch.tensor([starts[bad] <= f < starts[bad] + length for f in range(frames)], device="cuda")
            nan_frames = torch.isnan(x).all(dim=3).all(dim=1).all(dim=0)
            assert torch.equal(nan_frames, hit) and torch.isfinite(x[:, :, ~hit]).all(), (pchw, sched)
            if hist is not None:
                assert torch.equal(torch.isnan(hist).all(dim=3).all(dim=1).all(dim=0), hit)
            for w, s in enumerate(starts):
                got = torch.isnan(min_[w]).all(dim=3).all(dim=1).all(dim=0)
                assert torch.equal(got, hit[s:s + length]) and torch.isfinite(min_[w][:, :, ~hit[s:s + length]].float()).all(), (pchw, sched, w)


def test_wrapper_refusals():
    from lavie_amd import ops
    sched = (13, 8, (0, 5))
    d = make_inputs((2, 4, 8), sched, 1, True)
    x, eps = d["x"].cuda(), [e.cuda() for e in d["eps"]]
    min_ = [torch.empty_like(e) for e in eps]
    prof, co = profile_of("triangle", 8), COEFFS["five"][1]
    with pytest.raises(ValueError, match="model_in"):
        ops.window_step(eps, x, None, min_[:1], sched[2], prof, 7.5, co)
    with pytest.raises(ValueError, match="eps"):
        ops.window_step([eps[0], eps[1][:2]], x, None, min_, sched[2], prof, 7.5, co)
    with pytest.raises(ValueError, match="fp16"):
        ops.window_step([eps[0], eps[1].float()], x, None, min_, sched[2], prof, 7.5, co)
    with pytest.raises(ValueError, match="aux"):
        ops.window_step(eps, x, x[:1].contiguous(), min_, sched[2], prof, 7.5, COEFFS["five"][0])
    with pytest.raises(RuntimeError, match="aux is null"):
        ops.window_step(eps, x, None, min_, sched[2], prof, 7.5, COEFFS["five"][0])
    with pytest.raises(RuntimeError, match="overlap"):
        ops.window_step(eps, x, None, [min_[0], eps[0]], sched[2], prof, 7.5, co)
    short = lambda ts: [t[:, :, :4].contiguous() for t in ts]      # noqa: E731   windows of 4 frames leave frame 4 uncovered
    with pytest.raises(RuntimeError, match="uncovered"):
        ops.window_step(short(eps), x, None, short(min_), (0, 5), prof[:4], 7.5, co)


# ------------------------------------------------------------------ 3. the pipelines
STEPS = 4


@pytest.fixture(scope="module")
def small():
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    cfg = UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    sd = G.synth16(spec.param_shapes(cfg), 11)
    return build(sd, **SMALL_KW), sd


@pytest.fixture(scope="module")
def small_vsr():
    from test_gpu_vsr import build_small_vsr
    return build_small_vsr()[0]


def make_pipe(net, method):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    return VideoGenPipeline.from_sample_yaml(dict(sample_method=method), unet=net)[0]


def base_case(seed, frames):
    g = torch.Generator().manual_seed(seed)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    return pe, ne, torch.randn(1, 4, frames, 8, 8, generator=g)


@pytest.mark.parametrize("method", ["ddim", "dpmsolver++"])
def test_windows_that_only_touch_are_two_plain_runs_bit_for_bit(small, method):
    """denoise(window_length=8, window_stride=8) on 16 frames is bit-equal to two plain denoise calls on the two halves of the same
    latents (DDIM at eta = 0 and DPM-Solver++: no step noise); window_length >= video_length is the plain call."""
    net, _ = small
    pipe = make_pipe(net, method)
    pe, ne, lat = base_case(61, 16)
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    x_t = (lat * pipe.scheduler.init_noise_sigma).cuda()
    out = pipe.denoise(x_t, ctx, STEPS, 7.5, window_length=8, window_stride=8)
    halves = [pipe.denoise(x_t[:, :, s:s + 8].contiguous(), ctx, STEPS, 7.5) for s in (0, 8)]
    assert torch.isfinite(out).all() and torch.equal(out, torch.cat(halves, dim=2))
    plain = pipe.denoise(x_t, ctx, STEPS, 7.5)
    for length in (16, 24):
        assert torch.equal(pipe.denoise(x_t, ctx, STEPS, 7.5, window_length=length, window_stride=4), plain)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=64, video_length=16, num_inference_steps=STEPS,
              guidance_scale=7.5, output_type="latent", latents=lat)
    assert torch.equal(pipe(window_length=8, window_stride=8, **kw).video, out)        # the same through __call__
    assert torch.equal(pipe(window_length=16, **kw).video, plain)


def vsr_case(seed, frames):
    g = torch.Generator().manual_seed(seed)
    pe, ne = torch.randn(1, 77, 128, generator=g).half().float(), torch.randn(1, 77, 128, generator=g).half().float()
    return pe, ne, torch.randn(1, 3, frames, 8, 8, generator=g).clamp(-1, 1), torch.randn(1, 4, frames, 8, 8, generator=g)


@pytest.mark.parametrize("method", ["ddim", "dpmsolver++"])
def test_vsr_windows_that_only_touch_are_two_plain_runs_bit_for_bit(small_vsr, method):
    """The VSR denoise with the same noised low-res frames: two touching windows = two plain calls on the halves."""
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from lavie_amd.vsr import VideoUpscalePipeline
    pipe = VideoUpscalePipeline(unet=small_vsr, scheduler=DDIMScheduler() if method == "ddim" else DPMSolverMultistepScheduler())
    pe, ne, low, lat = vsr_case(71, 16)
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    low, lat = low.cuda(), lat.cuda()            # `denoise` takes the low-res frames already noised: any fixed tensor serves
    out = pipe.denoise(lat, low, ctx, 20, 3, 9.0, window_length=8, window_stride=8)
    halves = [pipe.denoise(lat[:, :, s:s + 8].contiguous(), low[:, :, s:s + 8].contiguous(), ctx, 20, 3, 9.0) for s in (0, 8)]
    assert torch.isfinite(out).all() and torch.equal(out, torch.cat(halves, dim=2))
    assert torch.equal(pipe.denoise(lat, low, ctx, 20, 3, 9.0, window_length=16), pipe.denoise(lat, low, ctx, 20, 3, 9.0))


def oracle_windowed_loop(sd, method, lat, pe, ne, length, stride, kind, gen):
    """Test-side fp32 loop: per step the oracle UNet on every window of the latents, guidance, the windows' predictions averaged per
    frame with the normalised profile weights (float64 weights, applied in fp32), then the scheduler update written out from
    `coefficients` on the whole clip."""
    from lavie_amd.windows import window_profile, window_starts
    from oracle import unet_fp32 as O
    sch = make_pipe(object(), method).scheduler
    sch.set_timesteps(STEPS)
    frac = bool(getattr(sch, "fractional_timesteps", False))
    ts = [float(t) if frac else int(t) for t in sch.timesteps]
    scale = getattr(sch, "model_input_scale", lambda t: 1.0)
    ctx = torch.cat([ne, pe]).half().float()
    frames = lat.shape[2]
    starts, profile = window_starts(frames, length, stride), window_profile(length, kind)
    weights = W.exact_weights(frames, starts, profile)
    x = lat * sch.init_noise_sigma
    x0_prev = None
    for i, t in enumerate(ts):
        fused = torch.zeros_like(x)
        for w, s in enumerate(starts):
            xin = (x[:, :, s:s + length] * scale(t)).half().float()
            e = O.unet_forward(sd, torch.cat([xin, xin]), t, ctx, ocfg_small())
            e = e[:1] + 7.5 * (e[1:] - e[:1])
            for f in range(s, s + length):
                fused[:, :, f] += weights[(w, f)] * e[:, :, f - s]
        k_x, k_e, c_x0, c_xt, c4 = sch.coefficients(t)
        x0 = k_x * x - k_e * fused
        if getattr(sch, "multistep", False):
            d = x0 + c4 * (x0 - x0_prev) if (c4 != 0.0 and i > 0) else x0
            x, x0_prev = c_xt * x + c_x0 * d, x0
        else:
            x = c_xt * x + c_x0 * x0
            if c4 != 0.0:
                x = x + c4 * torch.randn(x.shape, generator=gen)
    return x


@pytest.mark.parametrize("method", ["ddpm", "ddim", "eulerdiscrete", "dpmsolver++"])
def test_windowed_pipeline_vs_oracle_loop(small, method):
    """13 frames as two 8-frame windows at stride 6 (frames 5..7 shared), 4 guided steps, each sampler: within the project's
    pipeline bound of the test-side fp32 loop; the shared frames and their neighbours differ from two independent 8-frame runs."""
    net, sd = small
    pipe = make_pipe(net, method)
    pe, ne, lat = base_case(83, 13)
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    x_t = (lat * pipe.scheduler.init_noise_sigma).cuda()
    seen = []
    out = pipe.denoise(x_t, ctx, STEPS, 7.5, torch.Generator().manual_seed(3), callback=lambda i, t, x: seen.append(i),
                       window_length=8, window_stride=6).float().cpu()
    assert seen == list(range(STEPS)) and out.shape == lat.shape
    ref = oracle_windowed_loop(sd, method, lat, pe, ne, 8, 6, "triangle", torch.Generator().manual_seed(3))
    err = rel_l2(out, ref)
    print(f"{method}: 13 frames, windows of 8 at stride 6, {STEPS} steps: rel-L2 vs oracle loop {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL_PIPELINE


def test_upscale_in_chunks_with_overlap(small_vsr):
    """overlap = 2: [P, 4, F, h, w], finite, bit-reproducible across two calls; overlap = 0 is the chunk loop as it was (restated
    here: the pipeline on 8 frames at a time with one generator, concatenated) bit for bit."""
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.vsr import VideoUpscalePipeline, upscale_in_chunks
    pipe = VideoUpscalePipeline(unet=small_vsr, scheduler=DDIMScheduler())
    pe, ne, low, _ = vsr_case(91, 13)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=2, guidance_scale=9.0, noise_level=20)
    a = upscale_in_chunks(pipe, low, short_seq=8, overlap=2, generator=torch.Generator().manual_seed(1), **kw)
    b = upscale_in_chunks(pipe, low, short_seq=8, overlap=2, generator=torch.Generator().manual_seed(1), **kw)
    assert a.shape == (1, 4, 13, 8, 8) and torch.isfinite(a).all() and torch.equal(a, b)
    c = upscale_in_chunks(pipe, low, short_seq=8, overlap=0, generator=torch.Generator().manual_seed(1), **kw)
    gen = torch.Generator().manual_seed(1)
    chunks = torch.cat([pipe(image=low[:, :, s:min(13, s + 8)], generator=gen, **kw).images for s in range(0, 13, 8)], dim=2)
    assert torch.equal(c, chunks) and not torch.equal(a, c)
