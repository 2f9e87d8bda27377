"""-m gpu: the denoising objective evaluated forward (csrc/denoise_loss.hip, lavie_amd/denoising_loss.py).  The two
operators per element / per latent against the float64 restatement from the same Philox words (tests/denoise_loss_reference.py), with
poisoned outputs and guard bands around every output and the workspace; position and batch independence bit for bit; consistency with
`ops.philox_normal`; and `DenoisingLoss` on the smallest UNet the GPU tests build.

The bound of the loss is derived from the kernel's structure, not measured (`loss_tolerance`)."""
import numpy as np
import pytest
import torch

import denoise_loss_reference as D
import opcheck as oc

pytestmark = pytest.mark.gpu

f16, f32 = torch.float16, torch.float32
DRAW, DRAW_OFFSET = 6, 7
# name -> (per, hw): the vector path; the scalar path; a per that ends inside a block (257 lanes of 8); several blocks per latent
SHAPES = {"vector": (4 * 2 * 8 * 8, 8 * 8), "scalar": (4 * 3 * 5 * 7, 5 * 7), "ends_in_block": (8 * 256 + 8, 8),
          "several_blocks": (4 * 2 * 48 * 64, 48 * 64)}
# more chunks than the fold kernel has lanes (256 chunks of 2048 elements): its lanes add a second partial
PAST_ONE_FOLD_PASS = (2048 * 257 + 8, 8)


def ops():
    from lavie_amd import ops as o
    return o


def levels_of(P):
    """t = 0, t = 999 and one level in between, cycled over the latents"""
    from lavie_amd.denoising_loss import noise_levels
    from lavie_amd.scheduling_ddpm import DDPMScheduler
    three = noise_levels(DDPMScheduler(), (0, 999, 500))
    return [three[p % 3] for p in range(P)]


def seeds_of(P):
    return [0x0123456789ABCDEF, 7, 2 ** 64 - 1][:P] if P <= 3 else [1000 + 3 * p for p in range(P)]


def latents(P, per, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * P + per + seed)
    return torch.randn(P, per, generator=g).to(dtype)


def offset_of(with_offset, hw):
    return (0.1, DRAW_OFFSET, hw) if with_offset else None


def ordered(bits16):
    """fp16 bit patterns as integers in the order of their values (neighbours differ by 1; +0 and -0 coincide)"""
    b = bits16.astype(np.int32) & 0xFFFF
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


NOT_NEAREST = {}          # case -> (elements that are the neighbour of the nearest fp16, elements): reported, never read by an assertion


def check_model_in(got, ref64, label):
    """every element is the fp16 nearest to the float64 value, or its neighbour"""
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), label
    nearest = ref64.astype(np.float16)
    steps = np.abs(ordered(got.view(np.uint16)) - ordered(nearest.view(np.uint16)))
    NOT_NEAREST[label] = (int((steps != 0).sum()), steps.size)
    print(f"{label}: {NOT_NEAREST[label][0]} of {steps.size} elements are not the nearest fp16")
    bad = np.flatnonzero(steps.reshape(-1) > 1)
    assert bad.size == 0, (label, bad.size, int(bad[0]), got.reshape(-1)[bad[0]], ref64.reshape(-1)[bad[0]])


# ------------------------------------------------------------------ noisy_latents
@pytest.mark.parametrize("with_offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("dtype", [f32, f16], ids=["x0f32", "x0f16"])
@pytest.mark.parametrize("P", [1, 3, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_noisy_latents_per_element(shape, P, dtype, with_offset):
    per, hw = SHAPES[shape]
    x0, seeds, lv, off = latents(P, per, dtype), seeds_of(P), levels_of(P), offset_of(with_offset, hw)
    got = oc.run_guarded(lambda i, o: ops().noisy_latents(i["x0"], seeds, DRAW, lv, offset=off, out=o["model_in"]), {"x0": x0},
                         {"model_in": ((P, per), f16)}, sync=torch.cuda.synchronize)["model_in"]
    check_model_in(got, D.noisy(x0.numpy(), seeds, DRAW, lv, off), f"noisy[{shape},P{P},{'f32' if dtype == f32 else 'f16'},{'offset' if with_offset else 'plain'}]")


@pytest.mark.parametrize("dtype", [f32, f16], ids=["x0f32", "x0f16"])
@pytest.mark.parametrize("which", ["x0", "model_in"])
def test_noisy_latents_on_a_view_offset_by_one_element_has_the_aligned_bits(which, dtype):
    """per % 8 == 0 and one tensor a view that starts one element past a 16-byte boundary: every lane takes one element, the bits of the
    aligned call, and nothing outside the view is stored to."""
    P, (per, hw) = 3, SHAPES["ends_in_block"]
    x0, seeds, lv, off = latents(P, per, dtype), seeds_of(P), levels_of(P), offset_of(True, hw)
    aligned = ops().noisy_latents(x0.cuda(), seeds, DRAW, lv, offset=off).cpu()
    gx, gm = oc.guarded((P * per + 1,), dtype), oc.guarded((P * per + 1,), f16)
    ox, om = int(which == "x0"), int(which == "model_in")
    xv, mv = gx.t[ox:ox + P * per].view(P, per), gm.t[om:om + P * per].view(P, per)
    xv.copy_(x0)
    assert (xv.data_ptr() % 16 != 0) == (which == "x0") and (mv.data_ptr() % 16 != 0) == (which == "model_in")
    ops().noisy_latents(xv, seeds, DRAW, lv, offset=off, out=mv)
    torch.cuda.synchronize()
    gx.check_bands("x0")
    gm.check_bands("model_in")
    oc.assert_bits(mv, aligned, label="model_in")
    assert gm.unwritten().tolist() == [P * per if om == 0 else 0]


def test_noisy_latents_identities():
    """coef = 0 has the bits of the call without offset; s = 0 gives fp16(x0) exactly; a = 0, s = 1 gives fp16 of `ops.philox_normal` at
    the same key."""
    o = ops()
    for shape in ("vector", "scalar"):
        per, hw = SHAPES[shape]
        P = 3
        seeds, lv = seeds_of(P), levels_of(P)
        for dtype in (f32, f16):
            x0 = latents(P, per, dtype).cuda()
            plain = o.noisy_latents(x0, seeds, DRAW, lv)
            oc.assert_bits(o.noisy_latents(x0, seeds, DRAW, lv, offset=(0.0, DRAW_OFFSET, hw)), plain.cpu(), label="coef 0")
            assert not torch.equal(o.noisy_latents(x0, seeds, DRAW, lv, offset=(0.1, DRAW_OFFSET, hw)), plain)
            oc.assert_bits(o.noisy_latents(x0, seeds, DRAW, [(1.0, 0.0)] * P), x0.cpu().to(f16), label="s 0")
            normal = o.philox_normal(seeds, per, DRAW)
            oc.assert_bits(o.noisy_latents(x0, seeds, DRAW, [(0.0, 1.0)] * P), normal.cpu().to(f16), label="a 0, s 1")


# ------------------------------------------------------------------ denoising_loss
# The kernel's own structure (csrc/denoise_loss.hip): a lane adds 8 squares (one fma each), a 6-level butterfly in the wave, 3 adds
# over the four waves: summation depth 17 in fp32; the fold over the chunks and the division run in double, then ONE rounding to fp32.
DEPTH = 8 + 6 + 3
# Roundings of a target element before it meets pred, in units of 2^-24 of the magnitudes added up into it (target_scale): the normal
# is sqrt(-2 log u1) * sincospi(2 u2): log within 3 ulp and sincospi within 4 ulp of fp32 (the OpenCL bounds the device library
# states), halved by the correctly rounded sqrt (+ 0.5), one product (0.5): 1.5 + 0.5 + 0.5 + 4 + 0.5 = 7 ulp = 14 units; the offset
# fma and the v-prediction fma one unit each.
TARGET_UNITS = 16


def loss_tolerance(mse_ref, scale_sq_mean):
    """Relative bound of |mse - mse_ref|, all terms being non-negative: (depth + the final rounding + the rounding of d, which enters
    d^2 twice) 2^-24, plus the target's own error e_i <= TARGET_UNITS 2^-24 T_i in 2 |d_i| e_i, summed by Cauchy-Schwarz:
    sum |d| T <= sqrt(sum d^2 sum T^2)."""
    return (DEPTH + 1 + 2 + 2 * TARGET_UNITS * np.sqrt(scale_sq_mean / mse_ref)) * 2.0 ** -24


def run_loss(pred, x0, seeds, lv, kind, off):
    P, per = x0.shape
    need = ops().denoising_loss_workspace_floats(P, per)
    assert need == P * ((per + 2047) // 2048)
    got = oc.run_guarded(lambda i, o: ops().denoising_loss(i["pred"], i["x0"], seeds, DRAW, lv, kind, offset=off, workspace=o["ws"], out=o["out"]),
                         {"pred": pred, "x0": x0}, {"out": ((P,), f32), "ws": ((need,), f32)}, sync=torch.cuda.synchronize)
    return got["out"].numpy().astype(np.float64)


def check_loss(got, pred, tgt, scale, label):
    ref = D.mse(pred.numpy(), tgt)
    tol = loss_tolerance(ref, (scale * scale).mean(axis=1))
    err = np.abs(got - ref) / ref
    print(f"{label}: worst |err| / bound {float((err / tol).max()):.3f}")
    assert np.all(err <= tol), (label, got, ref, err, tol)


CASES = [(s, P) for s in SHAPES for P in (1, 3, 16)]


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("shape,P", CASES + [("past_one_fold_pass", 1)])
def test_denoising_loss_random_pred(shape, P, kind):
    per, hw = SHAPES.get(shape, PAST_ONE_FOLD_PASS)
    for dtype, with_offset in ((f32, True), (f16, False)):
        x0, seeds, lv, off = latents(P, per, dtype), seeds_of(P), levels_of(P), offset_of(with_offset, hw)
        pred = latents(P, per, f16, seed=1)
        got = run_loss(pred, x0, seeds, lv, kind, off)
        check_loss(got, pred, D.target(x0.numpy(), seeds, DRAW, lv, kind, off), D.target_scale(x0.numpy(), seeds, DRAW, lv, kind, off),
                   f"loss[{shape},P{P},{kind},{'f32' if dtype == f32 else 'f16'}]")


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("shape,P", CASES)
def test_denoising_loss_of_the_rounded_target_and_of_a_constant_shift(shape, P, kind):
    """pred = fp16(target): mse at the size of fp16 rounding, <= 2^-22 mean(target^2) + the square of the smallest subnormal (the
    rounding of an element is within 2^-12 of its magnitude or within half the smallest subnormal; the fp32 target's own error is 2^-8
    of that).  pred = fp16(target) + 0.5: against the float64 loss of that pred within the kernel's bound, and that within
    2 delta E + E^2 of delta^2, E = 2^-11 (max |target| + delta) covering the two fp16 roundings of pred."""
    per, hw = SHAPES[shape]
    delta = 0.5
    x0, seeds, lv, off = latents(P, per, f32), seeds_of(P), levels_of(P), offset_of(True, hw)
    tgt = D.target(x0.numpy(), seeds, DRAW, lv, kind, off)
    scale = D.target_scale(x0.numpy(), seeds, DRAW, lv, kind, off)
    rounded = torch.from_numpy(tgt.astype(np.float16))
    got = run_loss(rounded, x0, seeds, lv, kind, off)
    assert np.all(got <= 2.0 ** -22 * (tgt * tgt).mean(axis=1) + 2.0 ** -48), (got, (tgt * tgt).mean(axis=1))
    shifted = (rounded.float() + delta).to(f16)
    got = run_loss(shifted, x0, seeds, lv, kind, off)
    check_loss(got, shifted, tgt, scale, f"shift[{shape},P{P},{kind}]")
    E = 2.0 ** -11 * (np.abs(tgt).max() + delta)
    assert np.all(np.abs(D.mse(shifted.numpy(), tgt) - delta * delta) <= 2 * delta * E + E * E)
    assert np.all(np.abs(got - delta * delta) <= 2 * delta * E + E * E + loss_tolerance(delta * delta, (scale * scale).mean(axis=1)) * delta * delta)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sample_loss_of_an_exact_shift_is_exact(shape):
    """kind "sample" with fp16 x0 on a grid of 2^-6 and pred = x0 + 0.5: every difference is 0.5 exactly, every partial sum of 0.25s
    is exact in fp32, so mse == 0.25 bit for bit."""
    per, _ = SHAPES[shape]
    P = 3
    x0 = (torch.round(latents(P, per, f32).clamp(-3, 3) * 64) / 64).to(f16)
    pred = (x0.float() + 0.5).to(f16)
    assert torch.equal(pred.float() - x0.float(), torch.full((P, per), 0.5))
    got = run_loss(pred, x0, seeds_of(P), levels_of(P), "sample", None)
    assert got.tolist() == [0.25] * P


# ------------------------------------------------------------------ position and batch
@pytest.mark.parametrize("shape", ["vector", "scalar", "several_blocks"])
def test_a_latent_has_the_bits_of_its_single_call_at_every_position(shape):
    """latent 2 of P = 16 against its P = 1 call, and every P in 1..16 with the latent last, for both operators; two calls agree"""
    o = ops()
    per, hw = SHAPES[shape]
    seeds, lv, off = seeds_of(16), levels_of(16), offset_of(True, hw)
    x0, pred = latents(16, per, f32).cuda(), latents(16, per, f16, seed=1).cuda()
    whole_in = o.noisy_latents(x0, seeds, DRAW, lv, offset=off)
    whole = {k: o.denoising_loss(pred, x0, seeds, DRAW, lv, k, offset=off) for k in D.KINDS}
    oc.assert_bits(o.noisy_latents(x0, seeds, DRAW, lv, offset=off), whole_in.cpu(), label="second call")
    for p in (2, 15):
        one = slice(p, p + 1)
        oc.assert_bits(o.noisy_latents(x0[one], seeds[one], DRAW, lv[one], offset=off), whole_in[one].cpu(), label=f"model_in of latent {p}")
        for k in D.KINDS:
            oc.assert_bits(o.denoising_loss(pred[one], x0[one], seeds[one], DRAW, lv[one], k, offset=off), whole[k][one].cpu(), label=f"{k} of latent {p}")
            oc.assert_bits(o.denoising_loss(pred, x0, seeds, DRAW, lv, k, offset=off), whole[k].cpu(), label="second call")
    for P in range(1, 17):
        part = slice(16 - P, 16)
        oc.assert_bits(o.noisy_latents(x0[part], seeds[part], DRAW, lv[part], offset=off)[-1:], whole_in[15:].cpu(), label=f"P={P}")
        oc.assert_bits(o.denoising_loss(pred[part], x0[part], seeds[part], DRAW, lv[part], "v_prediction", offset=off)[-1:],
                       whole["v_prediction"][15:].cpu(), label=f"P={P}")


def test_loss_on_a_view_offset_by_one_element_has_the_aligned_bits():
    o = ops()
    P, (per, hw) = 3, SHAPES["ends_in_block"]
    seeds, lv, off = seeds_of(P), levels_of(P), offset_of(True, hw)
    x0, pred = latents(P, per, f32).cuda(), latents(P, per, f16, seed=1)
    aligned = o.denoising_loss(pred.cuda(), x0, seeds, DRAW, lv, "v_prediction", offset=off).cpu()
    g = oc.guarded((P * per + 1,), f16)
    view = g.t[1:1 + P * per].view(P, per)
    view.copy_(pred)
    oc.assert_bits(o.denoising_loss(view, x0, seeds, DRAW, lv, "v_prediction", offset=off), aligned, label="offset pred")
    g.check_bands("pred")


def test_wrappers_refuse_by_name():
    o = ops()
    x0 = torch.zeros(2, 24, device="cuda")
    h = torch.zeros(2, 24, dtype=f16, device="cuda")
    lv = [(1.0, 0.0)] * 2
    with pytest.raises(ValueError, match="3 seeds for 2 latents"):
        o.noisy_latents(x0, [1, 2, 3], 0, lv)
    with pytest.raises(ValueError, match="1 noise levels for 2"):
        o.noisy_latents(x0, [1, 2], 0, lv[:1])
    with pytest.raises(ValueError, match="hw=5 must divide per=24"):
        o.noisy_latents(x0, [1, 2], 0, lv, offset=(0.1, 1, 5))
    with pytest.raises(ValueError, match="kind 'velocity'"):
        o.denoising_loss(h, x0, [1, 2], 0, lv, "velocity")
    with pytest.raises(ValueError, match="pred must be"):
        o.denoising_loss(h[:1], x0, [1, 2], 0, lv, "epsilon")
    with pytest.raises(ValueError, match="workspace has 1 elements, 2 needed"):
        o.denoising_loss(h, x0, [1, 2], 0, lv, "epsilon", workspace=torch.zeros(1, device="cuda"))
    with pytest.raises(ValueError, match="at most 16"):
        o.noisy_latents(torch.zeros(17, 8, device="cuda"), list(range(17)), 0, [(1.0, 0.0)] * 17)


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def small():
    from test_gpu_lora import SMALL_KW, build, synth
    sd = synth(11, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    return build(sd, **SMALL_KW), sd


@pytest.fixture(scope="module")
def clip():
    g = torch.Generator().manual_seed(77)
    return torch.randn(2, 4, 4, 8, 8, generator=g).cuda(), torch.randn(2, 77, 128, generator=g).to(f16).cuda()


TS = [800, 150]


def scorer(net, **kw):
    from lavie_amd.denoising_loss import DenoisingLoss
    from lavie_amd.scheduling_ddpm import DDPMScheduler
    return DenoisingLoss(net, DDPMScheduler(), **kw)


def test_evaluate_is_the_operators_around_the_same_forward(small, clip):
    """model_in from the operator, the same unet on it, the float64 loss of that prediction against the regenerated target:
    `evaluate` matches it to the operator-level bound (the engine does the same forward, so no model tolerance enters); a second
    evaluate has the same bits; min-SNR weights and the host reduction on top."""
    from lavie_amd.denoising_loss import min_snr_weights, noise_levels, snr
    from lavie_amd.noise import PhiloxGenerator
    from lavie_amd.scheduling_ddpm import DDPMScheduler
    net, _ = small
    x0, ctx = clip
    P, per, hw = 2, x0[0].numel(), 64
    for kind, coef in (("epsilon", 0.0), ("v_prediction", 0.1)):
        gen = PhiloxGenerator([40, 41], draw=3)
        seeds, lv = gen.seeds(2), noise_levels(DDPMScheduler(), TS)
        off = (coef, 4, hw) if coef else None
        model_in = ops().noisy_latents(x0, seeds, 3, lv, offset=off)
        pred = net(model_in, torch.tensor(TS, dtype=f32, device="cuda"), encoder_hidden_states=ctx).sample
        flat = x0.reshape(P, per).cpu().numpy()
        tgt, scale = D.target(flat, seeds, 3, lv, kind, off), D.target_scale(flat, seeds, 3, lv, kind, off)
        ref = D.mse(pred.reshape(P, per).cpu().numpy(), tgt)
        s = scorer(net, prediction_type=kind, noise_offset=coef, snr_gamma=5.0)
        out = s.evaluate(x0, ctx, TS, gen)
        got = out.mse.cpu().numpy().astype(np.float64)
        assert out.mse.dtype == f32 and np.isfinite(got).all() and gen.draw == (5 if coef else 4)
        assert np.all(np.abs(got - ref) <= loss_tolerance(ref, (scale * scale).mean(axis=1)) * ref), (kind, got, ref)
        w = min_snr_weights(snr(DDPMScheduler(), TS), 5.0, kind)
        assert torch.equal(out.weights, w) and out.loss == float((out.mse.cpu().double() * w).mean())
        again = s.evaluate(x0, ctx, TS, PhiloxGenerator([40, 41], draw=3))
        oc.assert_bits(again.mse, out.mse.cpu(), label=f"second evaluate ({kind})")
        assert not torch.equal(s.evaluate(x0, ctx, TS, PhiloxGenerator([40, 42], draw=3)).mse[1], out.mse[1])


def test_a_lora_adapter_at_scale_0_is_the_base_and_at_scale_1_is_not(small, clip):
    from lavie_amd.noise import PhiloxGenerator
    from test_gpu_lora import adapter
    net, sd = small
    x0, ctx = clip
    s = scorer(net)
    base = s.evaluate(x0, ctx, TS, PhiloxGenerator(5)).mse.cpu()
    try:
        net.load_lora(adapter(sd, 16, 9))
        with_adapter = s.evaluate(x0, ctx, TS, PhiloxGenerator(5)).mse.cpu()
        assert not torch.equal(with_adapter, base)
        net.set_lora_scale(0.0)
        oc.assert_bits(s.evaluate(x0, ctx, TS, PhiloxGenerator(5)).mse, base, label="scale 0")
    finally:
        net.unload_lora()
    oc.assert_bits(s.evaluate(x0, ctx, TS, PhiloxGenerator(5)).mse, base, label="unloaded")


def test_sweep_returns_the_evaluate_columns(small, clip):
    from lavie_amd.noise import PhiloxGenerator
    net, _ = small
    x0, ctx = clip
    s = scorer(net)
    ts = (900, 500, 100)
    curve = s.sweep(x0, ctx, timesteps=ts, generator=PhiloxGenerator(8))
    assert curve.shape == (2, 3) and curve.dtype == torch.float64
    for k, t in enumerate(ts):
        col = s.evaluate(x0, ctx, t, PhiloxGenerator(8, draw=k)).mse.cpu().double()
        assert torch.equal(curve[:, k], col), (k, curve[:, k], col)
    assert curve[:, 0].mean() != curve[:, 2].mean()


def test_pipeline_denoising_loss_is_evaluate_on_its_own_parts(small, clip):
    from lavie_amd.noise import PhiloxGenerator
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, _ = small
    x0, ctx = clip
    pipe = VideoGenPipeline(unet=net)
    out = pipe.denoising_loss(latents=x0, prompt_embeds=ctx, timesteps=TS, seed=[40, 41])
    ref = scorer(net).evaluate(x0, ctx, TS, PhiloxGenerator([40, 41]))
    oc.assert_bits(out.mse, ref.mse.cpu(), label="pipeline")
    assert out.loss == ref.loss
