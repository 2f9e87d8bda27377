"""-m gpu: the UniPC sampler.  The fused step kernel (csrc/sampler_unipc.hip) per element against its float64 and
plain-fp32 forms (tests/unipc_reference.py) on guarded, poisoned operands, its bit guarantees, and the two pipelines with the new
scheduler against test-side loops around the fp32 oracles driven by unipc_reference.trajectory."""
import pytest
import torch

import guidance_reference as GR
import golden_util as G
import opcheck as OC
import unipc_reference as R
from gpu_util import rel_l2
from test_gpu_dpmsolver import TOL_PIPELINE
from test_gpu_engine import SMALL_KW, build, ocfg_small

pytestmark = pytest.mark.gpu

# (k_x, k_eps, corr, c_l, c_0, c_1, c_2, p_x, p_0, p_1): the four kinds of step a run takes (10 steps, positions 0, 1, 5, 9)
COEFFS = {"first": (1.0206, 0.2041, False, 0.0, 0.0, 0.0, 0.0, 0.8803, 0.1234, 0.0),
          "after first": (1.0911, 0.4364, True, 0.8612, 0.0661, 0.0661, 0.0, 0.7924, 0.2671, -0.0713),
          "middle": (1.3416, 0.8944, True, 0.7831, 0.1342, 0.0519, -0.0107, 0.6934, 0.3605, -0.0921),
          "final": (1.0001, 0.0100, True, 0.0447, 0.7013, 0.3122, -0.0574, 0.0, 1.0, 0.0)}
# vector body with a partial last block; one element per lane (n % 8 != 0), more than one block
SIZES = (8 * 256 * 2 + 8, 4 * 3 * 5 * 7)
SCALE = 0.8125


def _inputs(p, per, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(eps=torch.randn(2, p, per, generator=g).half(), x=torch.randn(p, per, generator=g) * 3.0,
                x_last=torch.randn(p, per, generator=g) * 3.0, m1=torch.randn(p, per, generator=g), m2=torch.randn(p, per, generator=g))


def _run(t, mode, coeffs, scale=SCALE, guidance=7.5, table=None, guard=False):
    """mode: "none" (eps = the first half only), "cfg", "table".  -> (x, x_last, m1, m2, model_in) on the device."""
    from lavie_amd import ops
    eps = t["eps"] if mode != "none" else t["eps"][0]
    bufs = {k: OC.Guarded(v.shape, v.dtype, data=v.contiguous()) for k, v in dict(t, eps=eps.contiguous()).items()}
    out = OC.guarded(eps.shape, torch.float16)
    hist = (bufs["x_last"].t, bufs["m1"].t, bufs["m2"].t)
    if mode == "none":
        ops.unipc_step(bufs["eps"].t, bufs["x"].t, hist, out.t, coeffs, scale)
    elif mode == "cfg":
        ops.cfg_unipc_step(bufs["eps"].t, bufs["x"].t, hist, out.t, guidance, coeffs, scale)
    else:
        ops.cfg_unipc_step_scaled(bufs["eps"].t, bufs["x"].t, hist, out.t, table.cuda(), coeffs, scale)
    torch.cuda.synchronize()
    if guard:
        bufs["eps"].check_unchanged("eps")
        for name, b in bufs.items():
            b.check_bands(name)
        out.check_written("model_in")
        out.check_bands("model_in")
    return bufs["x"].t.clone(), hist[0].clone(), hist[1].clone(), hist[2].clone(), out.t.clone()


@pytest.mark.parametrize("mode", ["cfg", "none", "table"])
@pytest.mark.parametrize("name", list(COEFFS))
def test_step_kernel_vs_fp32_and_float64_forms(name, mode):
    """Kernel against the update in float64 from the kernel's own inputs, per element, in units of 2^-24 M (M: the sum of the
    magnitudes of the terms of m, x^c, x').  The allowance is not a constant: the plain fp32 torch form's worst error in those
    units is measured on the same inputs, and the kernel is allowed twice that (fused multiply-adds reorder roundings).  model_in
    is bit-equal to fp16(fp32(x' scale)) of the kernel's own x', and is held to fp16(x'_f64 * scale), the reference value rounded
    once, within one fp16 spacing PLUS what x' itself was just allowed (2 * torch's error * 2^-24 M * scale).  One bare fp16
    spacing cannot hold for any fp32 evaluation: where the terms cancel (guidance 7.5: M ~ 20 |x'| and more) the allowed fp32 error
    of x' is larger than the fp16 spacing of the small x' (first seen on an MI355X: middle / cfg, n = 4104); the count of such
    elements is printed.  Operands sit between guard bands and model_in starts as NaN: every element written, nothing outside.
    Measured: DESIGN.md 7.22."""
    coeffs = COEFFS[name]
    table = torch.tensor([[7.5, 0.8], [3.0, 1.1]])
    worst, beyond = {}, 0
    for per in SIZES:
        p = 2 if mode == "table" else 1
        t = _inputs(p, per, per + len(name))
        xd, xl, m1, m2, mi = _run(t, mode, coeffs, table=table, guard=True)
        eu, ec = t["eps"][0], (None if mode == "none" else t["eps"][1])
        g = table[:, :1] if mode == "table" else 7.5
        f = table[:, 1:] if mode == "table" else 1.0
        if mode == "table":      # per-latent scalars: the reference forms take one pair at a time
            parts = [(R.kernel_form_f64(eu[j], ec[j], t["x"][j], t["x_last"][j], t["m1"][j], t["m2"][j], float(g[j]), float(f[j]), coeffs),
                      R.torch_form_f32(eu[j], ec[j], t["x"][j], t["x_last"][j], t["m1"][j], t["m2"][j], float(g[j]), float(f[j]), coeffs))
                     for j in range(p)]
            ref = [torch.stack([q[0][0][k] for q in parts]) for k in range(3)]
            mags = [torch.stack([q[0][1][k] for q in parts]) for k in range(3)]
            t32 = [torch.stack([q[1][k] for q in parts]) for k in range(3)]
        else:
            ref, mags = R.kernel_form_f64(eu, ec, t["x"], t["x_last"], t["m1"], t["m2"], g, f, coeffs)
            t32 = R.torch_form_f32(eu, ec, t["x"], t["x_last"], t["m1"], t["m2"], g, f, coeffs)
        for what, got, r64, r32, mag in (("m", m1, *[v[0] for v in (ref, t32, mags)]), ("xc", xl, *[v[1] for v in (ref, t32, mags)]),
                                         ("x'", xd, *[v[2] for v in (ref, t32, mags)])):
            unit = (R.U32 * mag).clamp_min(1e-300)
            allowed = ((r32.double() - r64).abs() / unit).max().item()
            ratio = ((got.cpu().double() - r64).abs() / unit).max().item()
            worst[what] = (max(worst.get(what, (0.0, 0.0))[0], ratio), max(worst.get(what, (0.0, 0.0))[1], allowed))
            assert ratio <= 2.0 * allowed, (what, per, ratio, allowed)
        want = (ref[2] * SCALE).half()
        spacing = torch.maximum(want.float().abs(), torch.tensor(2.0 ** -14)) * 2.0 ** -10
        slack = (2.0 * allowed * R.U32 * mags[2] * SCALE).float()          # what x' itself was just allowed (`allowed` is x''s here)
        halves = (mi.cpu().reshape(2, p, per) if mode != "none" else mi.cpu().reshape(1, p, per))
        for hlf in halves:
            off = (hlf.float() - want.float().reshape(p, per)).abs()
            beyond += int((off > spacing.reshape(p, per)).sum())
            assert (off <= (spacing + slack).reshape(p, per)).all(), per
        assert torch.equal(halves[0], halves[-1])
        assert torch.equal(mi.reshape(halves.shape)[0].cpu(), (xd.cpu().reshape(p, per) * SCALE).half())      # fp16(fp32(x' s)) of its own x'
        # the history moved on: m2 <- the m1 the call was given (read here in every kind but "first", which writes m)
        assert torch.equal(m2.cpu().reshape(p, per), t["m1"] if name != "first" else m1.cpu().reshape(p, per))
    print(name, mode, "kernel / torch-fp32 worst error in units of 2^-24 M:", {k: f"{a:.2f} / {b:.2f}" for k, (a, b) in worst.items()},
          f"; model_in elements beyond one bare fp16 spacing of the reference: {beyond}")


@pytest.mark.parametrize("mode", ["cfg", "none"])
def test_poisoned_history_is_never_read_when_its_coefficients_are_zero(mode):
    """x_last / m1 / m2 full of NaN: whichever buffer has no non-zero coefficient in force cannot reach an output, which is then
    bit-equal to the run with zeros there; with a coefficient in force the same poison does reach the output (the test can see)."""
    nan = float("nan")
    for per in SIZES:
        t = _inputs(1, per, 3)
        cases = {"first": ("x_last", "m1", "m2"), "after first": ("m2",),
                 "order 1 predictor": ("m2",)}
        cs = dict(COEFFS, **{"order 1 predictor": COEFFS["after first"][:9] + (0.0,)})
        for name, unread in cases.items():
            poisoned = dict(t, **{k: torch.full_like(t[k], nan) for k in unread})
            zeroed = dict(t, **{k: torch.zeros_like(t[k]) for k in unread})
            a, b = _run(poisoned, mode, cs[name]), _run(zeroed, mode, cs[name])
            assert all(torch.isfinite(v.float()).all() for v in a), name
            assert all(torch.equal(u, v) for u, v in zip(a, b)), name
        for k in ("x_last", "m1", "m2"):
            seen = _run(dict(t, **{k: torch.full_like(t[k], nan)}), mode, COEFFS["middle"])
            assert torch.isnan(seen[0]).all(), k


def test_degenerate_form_is_bit_equal_to_the_multistep_step():
    """corr = 0, p_1 = 0 and (p_x, p_0) = DPM-Solver++ order 1's (c_xt, c_x0): x and model_in have the bits of lavie_multistep_step /
    lavie_cfg_multistep_step with c_prev = 0, and m1 the bits of its x0_prev, at scale 1 and at another scale."""
    from lavie_amd import ops
    k_x, k_e, c_x0, c_xt = 1.0206, 0.2041, 0.1234, 0.8803
    uni = (k_x, k_e, False, 0.3, 0.2, 0.1, 0.4, c_xt, c_x0, 0.0)         # the corrector's coefficients are not in force
    for per in SIZES + (4 * 16 * 8 * 8,):
        for mode in ("cfg", "none"):
            for scale in (1.0, SCALE):
                t = _inputs(1, per, 17)
                xd, _, m1, _, mi = _run(t, mode, uni, scale)
                eps = (t["eps"] if mode == "cfg" else t["eps"][0]).contiguous().cuda()
                xo, hist, mo = t["x"].cuda().clone(), torch.empty(1, per, device="cuda"), torch.empty_like(eps)
                if mode == "cfg":
                    ops.cfg_multistep_step(eps, xo, hist, mo, 7.5, (k_x, k_e, c_x0, c_xt, 0.0), scale)
                else:
                    ops.multistep_step(eps, xo, hist, mo, (k_x, k_e, c_x0, c_xt, 0.0), scale)
                assert torch.equal(xd, xo) and torch.equal(mi, mo) and torch.equal(m1, hist), (per, mode, scale)


def test_two_runs_are_bit_identical_and_a_latent_of_a_batch_has_the_bits_of_its_single_call():
    table = torch.tensor([[7.5, 0.8], [3.0, 1.1]])
    for per in SIZES:
        t = _inputs(2, per, 5)
        a = _run(t, "table", COEFFS["middle"], table=table)
        b = _run(t, "table", COEFFS["middle"], table=table)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        for j in range(2):
            one = {k: (v[:, j:j + 1] if k == "eps" else v[j:j + 1]) for k, v in t.items()}
            c = _run(one, "table", COEFFS["middle"], table=table[j:j + 1])
            for u, v in zip(a[:4], c[:4]):
                assert torch.equal(u[j:j + 1], v)
            assert torch.equal(a[4].reshape(2, 2, per)[:, j], c[4].reshape(2, per))
        for mode in ("cfg", "none"):
            one = {k: (v[:, :1] if k == "eps" else v[:1]) for k, v in t.items()}
            assert all(torch.equal(u, v) for u, v in zip(_run(one, mode, COEFFS["middle"]), _run(one, mode, COEFFS["middle"])))
        # a table of (g, 1) gives the scalar-guidance kernel's bits
        one = {k: (v[:, :1] if k == "eps" else v[:1]) for k, v in t.items()}
        assert all(torch.equal(u, v) for u, v in zip(_run(one, "table", COEFFS["middle"], table=torch.tensor([[7.5, 1.0]])),
                                                      _run(one, "cfg", COEFFS["middle"])))


# ------------------------------------------------------------------ VideoGenPipeline
@pytest.fixture(scope="module")
def small():
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    cfg = UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    sd = G.synth16(spec.param_shapes(cfg), 11)
    return build(sd, **SMALL_KW), sd


def _timesteps(steps):
    return R.leading_timesteps(steps)


def _oracle_loop(sd, lat, pe, ne, steps, guidance, phi=0.0):
    """Test-side fp32 loop: the oracle UNet (fp16-rounded input, as the engine sees it), guidance and rescale per latent, and the
    whole-trajectory UniPC of unipc_reference.  guidance: a number (<= 1: none) or one value per latent."""
    from oracle import unet_fp32 as O
    p = lat.shape[0]
    scales = guidance if isinstance(guidance, (list, tuple)) else [guidance] * p

    def model(x, t):
        if scales[0] <= 1.0:
            return O.unet_forward(sd, x.half().float(), t, pe.half().float(), ocfg_small())
        ctx = torch.cat([ne, pe]).half().float()
        e = O.unet_forward(sd, torch.cat([x, x]).half().float(), t, ctx, ocfg_small())
        out = [GR.rescale_noise_cfg(e[j:j + 1] + scales[j] * (e[p + j:p + j + 1] - e[j:j + 1]), e[p + j:p + j + 1], phi) for j in range(p)]
        return torch.cat(out)

    return R.trajectory(model, lat.clone(), _timesteps(steps), R.abar_table())


def _unipc_pipe(net):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_unipc_multistep import UniPCMultistepScheduler
    return VideoGenPipeline(unet=net, scheduler=UniPCMultistepScheduler())


def test_pipeline_10_guided_steps_vs_oracle_loop(small):
    """10 guided steps through VideoGenPipeline(scheduler=UniPCMultistepScheduler()) against the fp32 loop, under the rel-L2 the
    DPM-Solver++ pipeline test is granted; a callback sees the scheduler's timesteps; the run is deterministic and a generator
    changes nothing (the solver draws no step noise)."""
    net, sd = small
    pipe = _unipc_pipe(net)
    g = torch.Generator().manual_seed(19)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    seen = []
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4,
              num_inference_steps=10, guidance_scale=7.5, output_type="latent")
    out = pipe(callback=lambda i, t, x: seen.append(t), **kw).video.float().cpu()
    assert seen == [901 - 100 * i for i in range(10)]
    err = rel_l2(out, _oracle_loop(sd, lat, pe, ne, 10, 7.5))
    print(f"10 guided UniPC steps: rel-L2 vs oracle loop {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL_PIPELINE
    assert torch.equal(pipe(**kw).video.float().cpu(), out)
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(1), **kw).video.float().cpu(), out)
    from lavie_amd.noise import PhiloxGenerator
    assert torch.equal(pipe(generator=PhiloxGenerator(7), **kw).video.float().cpu(), out)


def test_pipeline_without_guidance_and_generator_list(small):
    net, sd = small
    pipe = _unipc_pipe(net)
    g = torch.Generator().manual_seed(23)
    pe = torch.randn(2, 77, 128, generator=g)
    lat = torch.randn(2, 4, 4, 8, 8, generator=g)
    kw = dict(prompt_embeds=pe, height=64, width=64, video_length=4, num_inference_steps=10, guidance_scale=1.0, output_type="latent")
    out = pipe(latents=lat, **kw).video.float().cpu()
    err = rel_l2(out, _oracle_loop(sd, lat, pe, None, 10, 1.0))
    print(f"10 unguided UniPC steps: rel-L2 vs oracle loop {err:.3e}")
    assert err < TOL_PIPELINE
    gl = lambda: [torch.Generator().manual_seed(31), torch.Generator().manual_seed(32)]      # noqa: E731
    o2 = pipe(generator=gl(), **kw).video.float().cpu()
    lat2 = torch.cat([torch.randn(1, 4, 4, 8, 8, generator=q) for q in gl()])
    assert torch.equal(o2, pipe(latents=lat2, **kw).video.float().cpu())
    with pytest.raises(ValueError):
        pipe(generator=[torch.Generator()], **kw)


def test_pipeline_with_rescale_and_a_scale_per_prompt_vs_oracle_loop(small):
    """guidance_rescale = 0.7 with two prompts at different scales (the table form of the step) against the reference loop with
    rescale_noise_cfg written from its published formula (tests/guidance_reference.py)."""
    net, sd = small
    pipe = _unipc_pipe(net)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(2, 77, 128, generator=g), torch.randn(2, 77, 128, generator=g)
    lat = torch.randn(2, 4, 4, 8, 8, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4, num_inference_steps=6,
              output_type="latent")
    out = pipe(guidance_scale=[5.0, 9.0], guidance_rescale=0.7, **kw).video.float().cpu()
    err = rel_l2(out, _oracle_loop(sd, lat, pe, ne, 6, [5.0, 9.0], 0.7))
    plain = pipe(guidance_scale=[5.0, 9.0], **kw).video.float().cpu()
    print(f"6 UniPC steps, rescale 0.7, scales 5 / 9: rel-L2 vs oracle loop {err:.3e}; moved {rel_l2(out, plain):.3e} from the run without rescale")
    assert torch.isfinite(out).all() and err < TOL_PIPELINE and rel_l2(out, plain) > 0.0


def test_pipeline_with_graph_is_bit_equal_to_eager(small):
    net, _ = small
    g = torch.Generator().manual_seed(44)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)

    def run():
        return _unipc_pipe(net)(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat.clone(), num_inference_steps=10, guidance_scale=7.5,
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
    """VideoUpscalePipeline on the small VSR model, 12 frames = two chunks (8 + 4), UniPC: each chunk against the test-side fp32 loop
    (oracle VSR UNet + unipc_reference.trajectory), and chunk 2 bit-equal to the same frames through a fresh pipeline and
    scheduler, i.e. it saw nothing of chunk 1's history."""
    from lavie_amd.scheduling_unipc_multistep import UniPCMultistepScheduler
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
    pipe = VideoUpscalePipeline(unet=net, scheduler=UniPCMultistepScheduler())
    up = upscale_in_chunks(pipe, frames, short_seq=8, generator=torch.Generator().manual_seed(5), **kw).float().cpu()
    assert up.shape == (1, 4, 12, 8, 8) and torch.isfinite(up).all()

    gen = torch.Generator().manual_seed(5)
    unet = lambda x, low, t, ctx, labels: V.vsr_unet_forward(sd, x, low, t, ctx, labels, block_out_channels=(256, 512),      # noqa: E731
                                                            attn_levels=(False, True), only_cross_attention=(True, False),
                                                            layers_per_block=1, heads=8)
    chunk_inputs = []
    for lo, hi in ((0, 8), (8, 12)):
        part = frames[:, :, lo:hi]
        noise = torch.randn(part.shape, generator=gen)
        lat = torch.randn(1, 4, hi - lo, 8, 8, generator=gen)
        chunk_inputs.append((part, lat))
        img = add_low_res_noise(part, noise, level)
        ctx, low = torch.cat([ne, pe]), torch.cat([img, img])
        labels = torch.full((2,), level, dtype=torch.long)

        def model(x, t):
            eps = unet(torch.cat([x, x]).half().float(), low.half().float(), t, ctx, labels)
            return eps[:1] + guidance * (eps[1:] - eps[:1])

        x = R.trajectory(model, lat, _timesteps(steps), R.abar_table())
        err = rel_l2(up[:, :, lo:hi], x)
        print(f"VSR chunk frames {lo}:{hi}, UniPC: rel-L2 vs oracle loop {err:.3e}")
        assert err < TOL_PIPELINE, (lo, hi)
    gen = torch.Generator().manual_seed(5)
    torch.randn(chunk_inputs[0][0].shape, generator=gen)
    torch.randn(chunk_inputs[0][1].shape, generator=gen)
    fresh = VideoUpscalePipeline(unet=net, scheduler=UniPCMultistepScheduler())
    alone = fresh(image=chunk_inputs[1][0], generator=gen, **kw).images.float().cpu()
    assert torch.equal(alone, up[:, :, 8:12])
