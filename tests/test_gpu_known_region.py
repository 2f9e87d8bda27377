"""Sampling around known latents on the GPU: the five entry points of sampler_known.hip per element against their float64 form,
their exact properties (m = 0 is the plain kernel, m = 1 is the re-noised known latents, the end of a run), and the pipeline and
the clip continuation against test-side fp32 loops around the oracle UNet."""
import pytest
import torch

import golden_util as G
import known_reference as K
from gpu_util import rel_l2
from test_gpu_dpmsolver import TOL_PIPELINE
from test_gpu_engine import SMALL_KW, build, ocfg_small

pytestmark = pytest.mark.gpu

# (P, C, inner): one element; the one-element form across videos and channels; the smallest eight-element form; whole blocks with
# mask edges off the 8-boundaries; ragged; a typical small latent shape
SHAPES = ((1, 1, 1), (2, 3, 7), (2, 4, 8), (2, 4, 8 * 33), (1, 4, 2051), (2, 4, 4 * 8 * 8))
MASKS = ("zeros", "ones", "prefix", "binary", "soft")
ENTRIES = ("cfg_sampler", "sampler", "cfg_multistep", "multistep", "blend2", "blend1")
FAMILY = {"cfg_sampler": "five", "sampler": "five", "cfg_multistep": "multistep", "multistep": "multistep", "blend2": "blend",
          "blend1": "blend"}
GUIDED = {"cfg_sampler": True, "sampler": False, "cfg_multistep": True, "multistep": False, "blend2": True, "blend1": False}
# fifth coefficient: sigma of the step's own noise (five-coefficient family) / c_prev (multistep family), both zero and non-zero
COEFFS = {"five": ((1.0206, 0.2041, 0.1234, 0.8803, 0.35), (1.0206, 0.2041, 0.1234, 0.8803, 0.0)),
          "multistep": ((1.0206, 0.2041, 0.1234, 0.8803, 0.4712), (1.0206, 0.2041, 0.1234, 0.8803, 0.0)),
          "blend": ((0.0, 0.0, 0.0, 0.0, 0.0),)}
LEVEL, END = (0.8, 0.6), (1.0, 0.0)
GUIDANCE, SCALE = 7.5, 0.8125


def make_mask(kind, p, inner, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "zeros":
        return torch.zeros(p, 1, inner)
    if kind == "ones":
        return torch.ones(p, 1, inner)
    if kind == "prefix":                                     # the first frames pinned: an edge that is no multiple of 8
        m = torch.zeros(p, 1, inner)
        m[:, :, :min(inner, (inner * 3) // 8 + 3)] = 1.0
        return m
    if kind == "binary":
        return (torch.rand(p, 1, inner, generator=g) < 0.5).float()
    return torch.rand(p, 1, inner, generator=g) * 0.998 + 0.001          # soft: strictly inside (0, 1)


def make_inputs(shape, seed, guided):
    g = torch.Generator().manual_seed(seed)
    n = shape[0] * shape[1] * shape[2]
    return dict(eps=torch.randn((2 if guided else 1) * n, generator=g).half(), x=torch.randn(shape, generator=g) * 3.0,
                hist=torch.randn(shape, generator=g), nz=torch.randn(shape, generator=g), known=torch.randn(shape, generator=g) * 2.0,
                nk=torch.randn(shape, generator=g))


def run(entry, d, mask, coeffs, level, scale, known=None, nk="given"):
    """One launch on NaN-filled outputs.  Returns (x, x0_prev or None, model_in) on the device."""
    from lavie_amd import ops
    family, guided = FAMILY[entry], GUIDED[entry]
    x, n = d["x"].cuda().clone(), d["x"].numel()
    known = (d["known"] if known is None else known).cuda()
    nk = d["nk"].cuda() if isinstance(nk, str) else (None if nk is None else nk.cuda())
    mask = None if mask is None else mask.cuda()
    min_ = torch.full(((2 if guided else 1) * n,), float("nan"), dtype=torch.float16, device="cuda")
    hist = None
    if family == "blend":
        ops.known_blend(x, min_, known, mask, nk, level, scale)
    elif family == "five":
        nz = d["nz"].cuda() if coeffs[4] != 0.0 else None
        if guided:
            ops.cfg_sampler_step_known(d["eps"].cuda(), x, nz, min_, GUIDANCE, coeffs, scale, known, mask, nk, level)
        else:
            ops.sampler_step_known(d["eps"].cuda(), x, nz, min_, coeffs, scale, known, mask, nk, level)
    else:
        hist = d["hist"].cuda().clone() if coeffs[4] != 0.0 else torch.full_like(x, float("nan"))   # c_prev = 0 never reads it
        if guided:
            ops.cfg_multistep_step_known(d["eps"].cuda(), x, hist, min_, GUIDANCE, coeffs, scale, known, mask, nk, level)
        else:
            ops.multistep_step_known(d["eps"].cuda(), x, hist, min_, coeffs, scale, known, mask, nk, level)
    torch.cuda.synchronize()
    return x, hist, min_


def run_plain(entry, d, coeffs, scale):
    """The existing un-pinned kernel of the same family."""
    from lavie_amd import ops
    guided = GUIDED[entry]
    x, n = d["x"].cuda().clone(), d["x"].numel()
    min_ = torch.full(((2 if guided else 1) * n,), float("nan"), dtype=torch.float16, device="cuda")
    hist = None
    if FAMILY[entry] == "blend":
        (ops.latents_to_model_input if guided else ops.latents_to_model_input1)(x, min_, scale)
    elif FAMILY[entry] == "five":
        nz = d["nz"].cuda() if coeffs[4] != 0.0 else None
        if guided:
            ops.cfg_ddpm_step(d["eps"].cuda(), x, nz, min_, GUIDANCE, coeffs, scale)
        else:
            ops.sampler_step(d["eps"].cuda(), x, nz, min_, coeffs, scale)
    else:
        hist = d["hist"].cuda().clone() if coeffs[4] != 0.0 else torch.full_like(x, float("nan"))
        if guided:
            ops.cfg_multistep_step(d["eps"].cuda(), x, hist, min_, GUIDANCE, coeffs, scale)
        else:
            ops.multistep_step(d["eps"].cuda(), x, hist, min_, coeffs, scale)
    torch.cuda.synchronize()
    return x, hist, min_


def halves(d, guided):
    n = d["x"].numel()
    shape = d["x"].shape
    return (d["eps"][:n].reshape(shape), d["eps"][n:].reshape(shape)) if guided else (d["eps"].reshape(shape), None)


# ------------------------------------------------------------------ 1. per element
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_per_element_vs_float64(entry, kind):
    """Every entry point on every shape and mask, outputs pre-filled with NaN, against the step evaluated in float64 from the
    kernel's own inputs: |got - f64| <= K * 2^-24 * M with M the sum of term magnitudes and K twice the number of fp32 roundings of
    the spelled-out form (known_reference.py: 24 five-coefficient family, 26 multistep family, 12 its history, 8 blend).  The
    unfused torch fp32 form is held to the same bound.  model_in is exactly fp16 of the kernel's own x' times the scale, rounded
    as the family's plain kernel rounds it, and its halves are bit-equal under guidance."""
    family, guided = FAMILY[entry], GUIDED[entry]
    worst = {}
    for shape in SHAPES:
        for ci, coeffs in enumerate(COEFFS[family]):
            for level in (LEVEL, END):
                d = make_inputs(shape, 100 * shape[2] + ci, guided)
                mask = make_mask(kind, shape[0], shape[2], shape[2] + 7)
                aux = d["nz"] if family == "five" else d["hist"]
                x, hist, min_ = run(entry, d, mask, coeffs, level, SCALE)
                eu, ec = halves(d, guided) if family != "blend" else (None, None)
                mfull = K.expand_mask(mask, shape)
                xn64, mag, h64, hmag = K.known_form_f64(family, eu, ec, d["x"], aux, GUIDANCE, coeffs, d["known"], mfull, d["nk"], level)
                xn32, h32 = K.torch_form_f32(family, eu, ec, d["x"], aux, GUIDANCE, coeffs, d["known"], mfull, d["nk"], level)
                checks = [("x' kernel", x.cpu(), xn64, mag, K.K[family]), ("x' torch", xn32, xn64, mag, K.K[family])]
                if family == "multistep":
                    checks += [("x0' kernel", hist.cpu(), h64, hmag, K.K["history"]), ("x0' torch", h32, h64, hmag, K.K["history"])]
                for what, got, ref, m, k in checks:
                    assert torch.isfinite(got).all(), (what, shape)
                    ratio = ((got.double() - ref).abs() / (K.U32 * m).clamp_min(1e-300)).max().item()
                    worst[what] = max(worst.get(what, 0.0), ratio)
                    assert ratio <= k, (what, shape, coeffs, level, ratio)
                n = x.numel()
                want = (K.twice_rounded_f16 if family == "multistep" else K.once_rounded_f16)(x.reshape(-1), SCALE)
                assert torch.equal(min_[:n].cpu(), want), (shape, coeffs, level)
                if guided:
                    assert torch.equal(min_[n:], min_[:n]), (shape, coeffs, level)
    print(entry, kind, "max error in units of 2^-24 M:", {k: f"{v:.2f}" for k, v in worst.items()})


# ------------------------------------------------------------------ 2. the two exact ends of the mask
@pytest.mark.parametrize("entry", ENTRIES)
def test_mask_zero_is_the_plain_kernel_bit_for_bit(entry):
    """m = 0 everywhere: x, x0_prev and model_in are bit-equal to the existing un-pinned kernel of the same family (for the blend:
    x untouched and the model input of lavie_latents_to_scaled_model_input), at a scale != 1 too, and whatever known /
    noise_known hold: they are NaN here."""
    family = FAMILY[entry]
    for shape in SHAPES:
        for coeffs in COEFFS[family]:
            d = make_inputs(shape, 31 + shape[2], GUIDED[entry])
            nan = torch.full(shape, float("nan"))
            got = run(entry, d, torch.zeros(shape[0], 1, shape[2]), coeffs, LEVEL, SCALE, known=nan, nk=nan)
            ref = run_plain(entry, d, coeffs, SCALE)
            for name, a, b in zip(("x", "x0_prev", "model_in"), got, ref):
                if a is not None:
                    assert torch.isfinite(a.float()).all() and torch.equal(a, b), (name, shape, coeffs)


@pytest.mark.parametrize("entry", ENTRIES)
def test_mask_one_is_the_renoised_known_latents_bit_for_bit(entry):
    """m = 1 everywhere: x is xk = fma(s, noise_known, a known) bit for bit, whatever the model predicted (eps is NaN here), and
    the history of the multistep family is `known`.  xk is formed in float64 (the fp32 product a known, the exact product
    s noise_known, one sum) and rounded to fp32 once."""
    family = FAMILY[entry]
    for shape in SHAPES:
        d = make_inputs(shape, 57 + shape[2], GUIDED[entry])
        d["eps"] = torch.full_like(d["eps"], float("nan"))
        x, hist, min_ = run(entry, d, torch.ones(shape[0], 1, shape[2]), COEFFS[family][0], LEVEL, SCALE)
        a, s = K.f32s(LEVEL[0]), K.f32s(LEVEL[1])
        xk = ((a * d["known"]).double() + s * d["nk"].double()).float()
        assert torch.equal(x.cpu(), xk), shape
        assert torch.isfinite(min_.float()).all()
        if family == "multistep":
            assert torch.equal(hist.cpu(), d["known"]), shape
    if family == "blend":           # no mask at all is m = 1: the scheduler's add_noise
        x, _, _ = run(entry, d, None, COEFFS[family][0], LEVEL, SCALE)
        assert torch.equal(x.cpu(), xk)


# ------------------------------------------------------------------ 3. the end of a run
@pytest.mark.parametrize("entry", ENTRIES)
def test_end_of_run_ignores_the_noise_and_lands_on_known(entry):
    """s_next = 0: noise_known is not read, NaN-filled or absent (NULL) alike give the same finite output; with a = 1 the
    pinned elements are `known` bit for bit."""
    family = FAMILY[entry]
    for shape in SHAPES:
        d = make_inputs(shape, 77 + shape[2], GUIDED[entry])
        mask = make_mask("binary", shape[0], shape[2], 5)
        a = run(entry, d, mask, COEFFS[family][0], END, 1.0, nk=torch.full(shape, float("nan")))
        b = run(entry, d, mask, COEFFS[family][0], END, 1.0, nk=None)
        for p, q in zip(a, b):
            if p is not None:
                assert torch.isfinite(p.float()).all() and torch.equal(p, q), shape
        pinned = K.expand_mask(mask, shape) == 1
        assert torch.equal(a[0].cpu()[pinned], d["known"][pinned]), shape


# ------------------------------------------------------------------ 4. reproducibility
def test_two_runs_are_bit_identical():
    shape = (2, 4, 16 * 8 * 8)
    for entry in ENTRIES:
        d = make_inputs(shape, 3, GUIDED[entry])
        mask = make_mask("soft", shape[0], shape[2], 9)
        a = run(entry, d, mask, COEFFS[FAMILY[entry]][0], LEVEL, SCALE)
        b = run(entry, d, mask, COEFFS[FAMILY[entry]][0], LEVEL, SCALE)
        assert all(torch.equal(p, q) for p, q in zip(a, b) if p is not None), entry


def test_refused_calls_name_the_argument():
    from lavie_amd import ops
    d = make_inputs((2, 4, 8), 1, True)
    x, known, nk, mask = d["x"].cuda(), d["known"].cuda(), d["nk"].cuda(), torch.ones(2, 1, 8, device="cuda")
    min_ = torch.empty(2 * x.numel(), dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="noise_known"):
        ops.known_blend(x, min_, known, mask, None, LEVEL)
    with pytest.raises(RuntimeError, match="mask"):
        ops.cfg_sampler_step_known(d["eps"].cuda(), x, None, min_, 7.5, COEFFS["five"][1], 1.0, known, None, nk, LEVEL)
    with pytest.raises(RuntimeError, match="finite"):
        ops.known_blend(x, min_, known, mask, nk, LEVEL, float("nan"))
    with pytest.raises(ValueError, match="mask"):
        ops.known_blend(x, min_, known, torch.ones(2, 4, 8, device="cuda"), nk, LEVEL)


# ------------------------------------------------------------------ 5. the pipeline
SAMPLERS = ("ddpm", "ddim", "eulerdiscrete", "dpmsolver++")
STEPS, FRAMES = 4, 4


@pytest.fixture(scope="module")
def small():
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    cfg = UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    sd = G.synth16(spec.param_shapes(cfg), 11)
    return build(sd, **SMALL_KW), sd


def make_pipe(net, method):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    return VideoGenPipeline.from_sample_yaml(dict(sample_method=method), unet=net)[0]


def case(seed):
    g = torch.Generator().manual_seed(seed)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, FRAMES, 8, 8, generator=g)
    known = torch.randn(1, 4, FRAMES, 8, 8, generator=g) * 0.8
    noise = torch.randn(1, 4, FRAMES, 8, 8, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, height=64, width=64, video_length=FRAMES, num_inference_steps=STEPS,
              guidance_scale=7.5, output_type="latent")
    return pe, ne, lat, known, noise, kw


def first_frames_mask(k):
    m = torch.zeros(1, 1, FRAMES, 8, 8)
    m[:, :, :k] = 1.0
    return m


def oracle_loop(sd, method, lat, pe, ne, known, mask, noise, start, gen):
    """Test-side fp32 loop: the oracle UNet, the scheduler update written out from `coefficients` in torch, the replacement after
    every step in torch (known_reference.replace_known).  mask None: nothing pinned during the steps."""
    from oracle import unet_fp32 as O
    sch = make_pipe(object(), method).scheduler          # a scheduler of its own, configured as the pipeline configures it
    sch.set_timesteps(STEPS)
    frac = bool(getattr(sch, "fractional_timesteps", False))
    ts = [float(t) if frac else int(t) for t in sch.timesteps]
    scale = getattr(sch, "model_input_scale", lambda t: 1.0)
    ctx = torch.cat([ne, pe]).half().float()
    a, s = sch.noise_level(ts[start])
    xk = a * known + s * noise
    x = xk if (start > 0 or mask is None) else (1.0 - mask) * lat * sch.init_noise_sigma + mask * xk
    x0_prev = None
    for i in range(start, STEPS):
        t = ts[i]
        xin = (x * scale(t)).half().float()
        eps = O.unet_forward(sd, torch.cat([xin, xin]), t, ctx, ocfg_small())
        eps = eps[:1] + 7.5 * (eps[1:] - eps[:1])
        k_x, k_e, c_x0, c_xt, c4 = sch.coefficients(t)
        x0 = k_x * x - k_e * eps
        if getattr(sch, "multistep", False):
            d = x0 + c4 * (x0 - x0_prev) if (c4 != 0.0 and i > start) else x0
            x = c_xt * x + c_x0 * d
            x0_prev = x0 if mask is None else (1.0 - mask) * x0 + mask * known
        else:
            x = c_xt * x + c_x0 * x0
            if c4 != 0.0:
                x = x + c4 * torch.randn(x.shape, generator=gen)
        if mask is not None:
            level = sch.noise_level(ts[i + 1] if i + 1 < STEPS else None)
            x = K.replace_known(x, known, mask, noise, level)
    return x


@pytest.mark.parametrize("method", SAMPLERS)
def test_pipeline_pinned_everywhere_returns_known_and_mask_zero_is_the_plain_run(small, method):
    net, _ = small
    pipe = make_pipe(net, method)
    pe, ne, lat, known, noise, kw = case(41)
    full = pipe(latents=lat, known_latents=known, known_mask=torch.ones(1, 1, FRAMES, 8, 8), generator=torch.Generator().manual_seed(3),
                **kw).video
    assert torch.equal(full.float().cpu(), known)
    plain = pipe(latents=lat, generator=torch.Generator().manual_seed(3), **kw).video.clone()
    # `denoise` takes the explicit noise tensor; through __call__ the same run draws it from the generator
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    x_t = (lat * pipe.scheduler.init_noise_sigma).cuda()
    free = pipe.denoise(x_t, ctx, STEPS, 7.5, torch.Generator().manual_seed(3), known=known.cuda(),
                        mask=torch.zeros(1, 1, FRAMES, 8, 8), known_noise=noise.cuda())
    assert torch.equal(free, plain)


@pytest.mark.parametrize("method", SAMPLERS)
def test_pipeline_pinned_frames_vs_oracle_loop(small, method):
    """The first 2 frames pinned: they come back as `known`, the free frames differ from the plain run (temporal attention
    carries the known frames to them), and the whole loop stays within the project's bound of the test-side fp32 loop."""
    net, sd = small
    pipe = make_pipe(net, method)
    pe, ne, lat, known, noise, kw = case(43)
    mask = first_frames_mask(2)
    ctx = torch.cat([ne, pe]).to("cuda", torch.float16).contiguous()
    x_t = (lat * pipe.scheduler.init_noise_sigma).cuda()
    out = pipe.denoise(x_t, ctx, STEPS, 7.5, torch.Generator().manual_seed(3), known=known.cuda(), mask=mask,
                       known_noise=noise.cuda()).float().cpu()
    plain = pipe(latents=lat, generator=torch.Generator().manual_seed(3), **kw).video.float().cpu()
    assert torch.equal(out[:, :, :2], known[:, :, :2])
    moved = rel_l2(out[:, :, 2:], plain[:, :, 2:])
    ref = oracle_loop(sd, method, lat, pe, ne, known, mask, noise, 0, torch.Generator().manual_seed(3))
    err = rel_l2(out, ref)
    print(f"{method}: pinned 2 of {FRAMES} frames, {STEPS} steps: rel-L2 vs oracle loop {err:.3e}; free frames moved {moved:.3e} from the plain run")
    assert moved > 1e-2
    assert torch.isfinite(out).all() and err < TOL_PIPELINE


@pytest.mark.parametrize("method", SAMPLERS)
def test_pipeline_strength_half_vs_oracle_loop(small, method):
    """strength = 0.5 through __call__: the loop runs the last 2 of 4 timesteps from add_noise(known, noise, timesteps[2])."""
    net, sd = small
    pipe = make_pipe(net, method)
    pe, ne, lat, known, noise, kw = case(47)
    seen = []
    # the generator's first draw of the call is the run's noise tensor (latents are given): the same tensor the loop gets
    gen = torch.Generator().manual_seed(9)
    out = pipe(latents=lat, known_latents=known, strength=0.5, generator=gen, callback=lambda i, t, x: seen.append(i), **kw).video.float().cpu()
    assert seen == [2, 3]
    gen = torch.Generator().manual_seed(9)
    drawn = torch.randn(lat.shape, generator=gen)
    ref = oracle_loop(sd, method, lat, pe, ne, known, None, drawn, 2, gen)
    err = rel_l2(out, ref)
    print(f"{method}: strength 0.5, {STEPS} steps: rel-L2 vs oracle loop {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL_PIPELINE


# ------------------------------------------------------------------ 6. clip continuation
def test_continue_clip_pins_the_overlap_bit_for_bit(small):
    from lavie_amd.cascade import continue_clip, text_to_long_video
    net, _ = small
    pipe = make_pipe(net, "ddim")
    pe, ne, _, _, _, kw = case(53)
    kw.update(video_length=8, num_inference_steps=4)
    kw.pop("output_type")
    clip1 = pipe(generator=torch.Generator().manual_seed(1), output_type="latent", **kw).video
    clip2 = continue_clip(pipe, clip1, overlap=3, generator=torch.Generator().manual_seed(2), **kw)
    assert clip2.shape == clip1.shape
    assert torch.equal(clip2[:, :, :3], clip1[:, :, -3:])
    assert not torch.equal(clip2[:, :, 3:], clip1[:, :, 3:])
    long = text_to_long_video(pipe, None, 3, overlap=3, generator=torch.Generator().manual_seed(1), **kw)
    assert long.shape[2] == 8 + 2 * (8 - 3)
    assert torch.equal(long[:, :, :8], clip1) and torch.isfinite(long).all()
