"""Seeded engine noise on the device (csrc/philox.h, csrc/sampler_noise.hip, csrc/sampler_window.hip): the materialised tensor
against the float64 reference from the same words, its addressing (rows, slices, alignment, draws, seeds), the fused seeded steps
against the materialised noise followed by today's steps, bit for bit, and the pipelines with a `PhiloxGenerator`."""
import numpy as np
import pytest
import torch

import noise_reference as R
import opcheck as oc

pytestmark = pytest.mark.gpu

f16, f32 = torch.float16, torch.float32
SEEDS3 = [0x0123456789ABCDEF, 7, 2 ** 64 - 1]
BIG = 2 ** 34 - 3                  # + 3 crosses the low counter word: block 2^32 - 1 -> 2^32


def ops():
    from lavie_amd import ops as o
    return o


# ------------------------------------------------------------------ 4. accuracy
_REF = {}


def reference(seed, draw, first, per):
    """(float64 reference, max |error| of the same formula evaluated in fp32 by torch on the CPU), computed once per case."""
    k = (seed, draw, first, per)
    if k not in _REF:
        ref = R.normal(seed, draw, first, per)
        _REF[k] = (ref, float(np.abs(R.normal_fp32_formula(seed, draw, first, per).astype(np.float64) - ref).max()))
    return _REF[k]


def test_accuracy_against_float64_from_the_same_words():
    """max |device - float64| <= 2 x max |fp32 formula on the CPU - float64| over all cases together (same precision, another libm; the
    CPU figure is taken over the union of the cases so that a case of one element does not set a bound of its own luck).  Measured:
    DESIGN 7.18."""
    worst_dev = worst_cpu = 0.0
    for per in (1, 7, 8, 4099):
        for first in (0, 5, BIG):
            got = ops().philox_normal(SEEDS3, per, 3, first_element=first).cpu().numpy()
            assert got.shape == (3, per) and np.isfinite(got).all()
            for p, seed in enumerate(SEEDS3):
                ref, cpu_err = reference(seed, 3, first, per)
                worst_dev = max(worst_dev, float(np.abs(got[p].astype(np.float64) - ref).max()))
                worst_cpu = max(worst_cpu, cpu_err)
    print(f"max |error| vs float64: device {worst_dev:.3e}, fp32 formula on the CPU {worst_cpu:.3e}")
    assert worst_cpu > 0 and worst_dev <= 2 * worst_cpu, (worst_dev, worst_cpu)


@pytest.mark.parametrize("first", [0, 5, BIG])
def test_accuracy_case_by_case_at_4099_elements(first):
    """The same yardstick without pooling: for each seed at per = 4099 (enough elements for the CPU figure to be a maximum and not
    one element's luck) the device's max |error| is within twice the fp32 formula's ON THAT CASE."""
    got = ops().philox_normal(SEEDS3, 4099, 3, first_element=first).cpu().numpy().astype(np.float64)
    for p, seed in enumerate(SEEDS3):
        ref, cpu_err = reference(seed, 3, first, 4099)
        dev_err = float(np.abs(got[p] - ref).max())
        print(f"first={first} seed={seed:#x}: device {dev_err:.3e}, fp32 formula on the CPU {cpu_err:.3e}")
        assert cpu_err > 0 and dev_err <= 2 * cpu_err, (first, seed, dev_err, cpu_err)


def test_u1_equal_to_one_gives_a_zero():
    """ln 1 = 0: r = -0 and the value is +-0 exactly.  Element 49975720 of (seed 99, draw 0) is the first such element of that latent
    (found once by searching the words on the host; that it is one is asserted here)."""
    seed, e = 99, 49975720
    a, b, second = R.words(seed, 0, e, 2)
    assert int(a[0]) >> 8 == 0xFFFFFF and int(a[1]) >> 8 == 0xFFFFFF          # the pair's two values share u1
    for first, per in ((e - e % 4, 16), (e - 1, 5)):                   # the eight-element form and the scalar one
        got = ops().philox_normal([seed], per, 0, first_element=first).cpu().numpy()[0]
        assert got[e - first] == 0.0 and got[e + 1 - first] == 0.0 and np.isfinite(got).all(), (first, per, got)


# ------------------------------------------------------------------ 5. addressing
@pytest.mark.parametrize("P", [1, 2, 16])
def test_a_row_is_the_single_latent_call(P):
    seeds = [1000 + 3 * p for p in range(P)]
    for per, first in ((4099, 0), (64, 8), (24, 6)):                     # scalar form, eight-element form, first % 4 != 0
        both = ops().philox_normal(seeds, per, 5, first_element=first)
        for p, s in enumerate(seeds):
            oc.assert_bits(both[p:p + 1], ops().philox_normal([s], per, 5, first_element=first).cpu(), label=f"P={P} row {p} per={per}")


def test_more_than_sixteen_rows_take_several_launches():
    seeds = list(range(50, 69))
    both = ops().philox_normal(seeds, 40, 2)
    oc.assert_bits(both[17:18], ops().philox_normal([67], 40, 2).cpu(), label="row 17 of 19")


def test_a_slice_is_that_range_of_the_whole():
    whole = ops().philox_normal([77], 4096, 9).cpu()
    for first, per in ((0, 4096), (8, 64), (4, 24), (5, 24), (6, 7), (1, 1), (4095, 1), (3, 4093)):
        oc.assert_bits(ops().philox_normal([77], per, 9, first_element=first), whole[:, first:first + per], label=f"[{first}, {first + per})")
    # an unaligned output pointer takes the scalar form: the same bits, and nothing around it is written
    g = oc.guarded((1 + 64 + 3,), f32)
    ops().philox_normal([77], 64, 9, first_element=8, out=g.t[1:65])
    torch.cuda.synchronize()
    g.check_bands("out")
    oc.assert_bits(g.t[1:65].reshape(1, 64), whole[:, 8:72], label="unaligned out")
    assert g.unwritten().tolist() == [0, 65, 66, 67]
    # across the low counter word
    hi = ops().philox_normal([77], 16, 9, first_element=BIG - 1).cpu()
    oc.assert_bits(ops().philox_normal([77], 8, 9, first_element=BIG + 3), hi[:, 4:12], label="across 2^34")


def test_draw_and_seed_change_the_tensor():
    base = ops().philox_normal([77], 256, 9)
    assert not torch.equal(base, ops().philox_normal([77], 256, 10))
    assert not torch.equal(base, ops().philox_normal([78], 256, 9))
    assert not torch.equal(base, ops().philox_normal([77], 256, 9 + 2 ** 32))        # the draw's high word is used
    assert not torch.equal(base, ops().philox_normal([77 + 2 ** 32], 256, 9))        # and the seed's
    assert torch.equal(base, ops().philox_normal([77], 256, 9))


# ------------------------------------------------------------------ 6. fused = materialised, bit for bit
K = (1.0078, 0.1254, 0.0351, 0.9612, 0.0421)        # k_x, k_eps, c_x0, c_xt, sigma
SCALE = 0.8125


def step_inputs(P, per, guided, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, per, generator=g)
    eps = torch.randn((2 if guided else 1) * P, per, generator=g).to(f16)
    return x, eps


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("per", [24, 27, 2048 + 16, 2048 + 19])
@pytest.mark.parametrize("sigma", [K[4], 0.0])
def test_seeded_step_is_the_materialised_noise_and_todays_step(guided, P, per, sigma):
    """n = P per with per in {8 k, 8 k + 3}: k = 3 (one workgroup) and k = 258 (more than one: 2064 / 8 lanes > 256)."""
    from lavie_amd.noise import NoiseKey
    o = ops()
    key = NoiseKey([31 + 5 * p for p in range(P)], 6)
    co = K[:4] + (sigma,)
    x, eps = step_inputs(P, per, guided, 17 * P + per)
    nb = eps.shape[0]

    def plain(i, out):
        noise = o.philox_normal(key.seeds, per, key.draw) if sigma != 0.0 else None
        if guided:
            o.cfg_ddpm_step(i["eps"], i["x"], noise, out["model_in"], 7.5, co, SCALE)
        else:
            o.sampler_step(i["eps"], i["x"], noise, out["model_in"], co, SCALE)

    def seeded(i, out):
        if guided:
            o.cfg_sampler_step_seeded(i["eps"], i["x"], key, out["model_in"], 7.5, co, SCALE)
        else:
            o.sampler_step_seeded(i["eps"], i["x"], key, out["model_in"], co, SCALE)

    runs = [oc.run_guarded(fn, {"eps": eps, "x": x}, {"model_in": ((nb, per), f16), "x": ((P, per), f32)}, alias={"x": "x"},
                           sync=torch.cuda.synchronize) for fn in (plain, seeded)]
    oc.assert_bits(runs[1]["x"], runs[0]["x"], label="x")
    oc.assert_bits(runs[1]["model_in"], runs[0]["model_in"], label="model_in")
    assert torch.isfinite(runs[1]["x"]).all() and not torch.equal(runs[1]["x"], x)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("hw", [24, 21])
@pytest.mark.parametrize("sigma", [K[4], 0.0])
def test_seeded_window_step_is_window_step_on_the_materialised_clip_noise(guided, hw, sigma):
    """[2, 4, 11, hw] with windows of 4 at stride 3 (starts 0, 3, 6, 7): hw = 24 the eight-element form, 21 the scalar one."""
    from lavie_amd.noise import NoiseKey
    from lavie_amd.windows import window_profile, window_starts
    o = ops()
    P, C, F, L = 2, 4, 11, 4
    starts, profile = window_starts(F, L, 3), window_profile(L, "triangle")
    key = NoiseKey([901, 17], 4)
    co = K[:4] + (sigma,)
    g = torch.Generator().manual_seed(5 + hw)
    x = torch.randn(P, C, F, hw, generator=g)
    nb = 2 * P if guided else P
    eps = {f"eps{w}": torch.randn(nb, C, L, hw, generator=g).to(f16) for w in range(len(starts))}
    outs = {f"model_in{w}": ((nb, C, L, hw), f16) for w in range(len(starts))}
    outs["x"] = ((P, C, F, hw), f32)
    guidance = 7.5 if guided else None

    def lists(i, out):
        return [i[f"eps{w}"] for w in range(len(starts))], [out[f"model_in{w}"] for w in range(len(starts))]

    def plain(i, out):
        e, m = lists(i, out)
        noise = o.philox_normal(key.seeds, C * F * hw, key.draw).view(P, C, F, hw) if sigma != 0.0 else None
        o.window_step(e, i["x"], noise, m, starts, profile, guidance, co, SCALE)

    def seeded(i, out):
        e, m = lists(i, out)
        o.window_step_seeded(e, i["x"], key, m, starts, profile, guidance, co, SCALE)

    runs = [oc.run_guarded(fn, dict(eps, x=x), outs, alias={"x": "x"}, sync=torch.cuda.synchronize) for fn in (plain, seeded)]
    for name in outs:
        oc.assert_bits(runs[1][name], runs[0][name], label=name)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("which", ["eps", "x", "model_in"])
def test_seeded_step_on_offset_views_has_the_aligned_calls_bits(guided, which):
    """Like the plain step the seeded one has no alignment rule: with per % 8 == 0 and one tensor a view that starts 4 (fp32) or 2
    (fp16) bytes past a 16-byte boundary every lane takes one element: the bits of the aligned call, and nothing outside is stored to."""
    from lavie_amd.noise import NoiseKey
    o = ops()
    P, per = 2, 2048 + 16
    key = NoiseKey([8, 9], 2)
    x, eps = step_inputs(P, per, guided, 3)
    nb = eps.shape[0]
    call = (lambda e, xx, m: o.cfg_sampler_step_seeded(e, xx, key, m, 7.5, K, SCALE)) if guided else \
        (lambda e, xx, m: o.sampler_step_seeded(e, xx, key, m, K, SCALE))
    xa, ea, ma = x.cuda(), eps.cuda(), torch.empty(nb, per, dtype=f16, device="cuda")
    call(ea, xa, ma)
    gx, ge, gm = oc.guarded((P * per + 1,), f32), oc.guarded((nb * per + 1,), f16), oc.guarded((nb * per + 1,), f16)
    off = {name: int(name == which) for name in ("eps", "x", "model_in")}
    xv = gx.t[off["x"]:off["x"] + P * per].view(P, per)
    ev = ge.t[off["eps"]:off["eps"] + nb * per].view(nb, per)
    mv = gm.t[off["model_in"]:off["model_in"] + nb * per].view(nb, per)
    xv.copy_(x)
    ev.copy_(eps)
    assert (xv.data_ptr() % 16 != 0) == (which == "x") and (mv.data_ptr() % 16 != 0) == (which == "model_in")
    call(ev, xv, mv)
    torch.cuda.synchronize()
    for g, name in ((gx, "x"), (ge, "eps"), (gm, "model_in")):
        g.check_bands(name)
    oc.assert_bits(xv, xa.cpu(), label="x")
    oc.assert_bits(mv, ma.cpu(), label="model_in")
    spare = nb * per if off["model_in"] == 0 else 0                      # the one element of the buffer outside the view
    assert gm.unwritten().tolist() == [spare]


def test_seeded_steps_take_their_scalars_as_they_come():
    """as sampler_step / cfg_ddpm_step: a non-finite coefficient is not refused (it poisons x, as in the plain entry)"""
    from lavie_amd.noise import NoiseKey
    o = ops()
    x, eps = step_inputs(1, 24, False, 4)
    xa, xb, e = x.cuda(), x.cuda(), eps.cuda()
    co = (float("nan"),) + K[1:]
    o.sampler_step_seeded(e, xa, NoiseKey([5], 1), torch.empty_like(e), co)
    o.sampler_step(e, xb, o.philox_normal([5], 24, 1), torch.empty_like(e), co)
    assert torch.isnan(xa).all() and torch.isnan(xb).all()


def test_wrappers_refuse_by_name():
    from lavie_amd.noise import NoiseKey
    o = ops()
    x = torch.zeros(2, 24, device="cuda")
    h = torch.zeros(2, 24, dtype=f16, device="cuda")
    with pytest.raises(ValueError, match="3 seeds for 2 latents"):
        o.sampler_step_seeded(h, x, NoiseKey([1, 2, 3], 0), h, K)
    with pytest.raises(ValueError, match="twice"):
        o.cfg_sampler_step_seeded(h, x, NoiseKey([1, 2], 0), h, 7.5, K)
    x17 = torch.zeros(17, 8, device="cuda")
    h17 = torch.zeros(17, 8, dtype=f16, device="cuda")
    with pytest.raises(ValueError, match="at most 16"):
        o.sampler_step_seeded(h17, x17, NoiseKey(list(range(17)), 0), h17, K)


# ------------------------------------------------------------------ 7. the pipelines
STEPS = 4


@pytest.fixture(scope="module")
def small():
    import golden_util as G
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    from test_gpu_engine import SMALL_KW, build
    cfg = UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    return build(G.synth16(spec.param_shapes(cfg), 11), **SMALL_KW)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(77)
    return torch.randn(2, 77, 128, generator=g), torch.randn(2, 77, 128, generator=g)


def pipe_of(net):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    return VideoGenPipeline(unet=net)                  # DDPM: noise at every step but the last


def call(pipe, pe, ne, generator, frames=8, **more):
    kw = dict(height=64, width=64, video_length=frames, num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent")
    kw.update(more)
    return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, generator=generator, **kw).video.float().cpu()


def test_a_prompt_in_a_batch_gets_the_noise_of_its_single_call(small, prompts):
    """Initial latents and every step's noise come from the generator.  The NOISE of latent j in the batch has the bits of the single
    call's (asserted on the draws themselves); the videos agree to rel-L2 5e-3, the tolerance of
    test_gpu_engine.test_prompts_batched_per_forward_match_single_prompt_runs, which shows that the UNet itself is not bit-invariant
    to the batch at this configuration (other GEMM tiles at twice the rows)."""
    from gpu_util import rel_l2
    from lavie_amd.noise import PhiloxGenerator
    from lavie_amd.scheduling_ddpm import randn_tensor
    pe, ne = prompts
    pipe = pipe_of(small)
    sa, sb = 4100, 93
    both = call(pipe, pe, ne, PhiloxGenerator([sa, sb]))
    for j, s in enumerate((sa, sb)):
        one = call(pipe, pe[j:j + 1], ne[j:j + 1], PhiloxGenerator(s))
        assert torch.isfinite(one).all() and rel_l2(both[j:j + 1], one) < 5e-3, j
    assert rel_l2(both[0], both[1]) > 0.1
    gb, ga = PhiloxGenerator([sa, sb]), PhiloxGenerator(sb)
    for shape in ((4, 8, 8, 8), (4, 8, 8, 8), (3, 5, 7, 9)):
        b = randn_tensor((2,) + shape, generator=gb, device="cuda")
        oc.assert_bits(b[1:2], randn_tensor((1,) + shape, generator=ga, device="cuda").cpu(), label=str(shape))
    sliced = PhiloxGenerator([sa, sb])[1:2]
    oc.assert_bits(randn_tensor((1, 4, 8, 8, 8), generator=sliced, device="cuda"),
                   randn_tensor((1, 4, 8, 8, 8), generator=PhiloxGenerator(sb), device="cuda").cpu(), label="slice")


def test_equal_seeds_agree_bit_for_bit_plain_windowed_and_around_known_latents(small, prompts):
    """A windowed call and a call around known latents are two cases: frame windows are not combined with known latents
    (sampling.REFUSED["window_length", "known"]), whatever the generator."""
    from lavie_amd.noise import PhiloxGenerator
    pe, ne = prompts
    pipe = pipe_of(small)
    known = torch.randn(1, 4, 8, 8, 8, generator=torch.Generator().manual_seed(3))
    mask = torch.zeros(1, 1, 8, 1, 1)
    mask[:, :, :2] = 1
    cases = {"plain": dict(), "windowed": dict(frames=11, window_length=8, window_stride=3),
             "known": dict(known_latents=known, known_mask=mask), "no guidance": dict(guidance_scale=1.0)}
    outs = {}
    for name, more in cases.items():
        a = call(pipe, pe[:1], ne[:1], PhiloxGenerator(12), **more)
        b = call(pipe, pe[:1], ne[:1], PhiloxGenerator(12), **more)
        assert torch.isfinite(a).all() and torch.equal(a, b), name
        assert not torch.equal(a, call(pipe, pe[:1], ne[:1], PhiloxGenerator(13), **more)), name
        outs[name] = a
    assert not torch.equal(outs["plain"], outs["known"])


def test_a_torch_generator_launches_what_it_launched(small, prompts, monkeypatch):
    """No seeded entry and no philox_normal is reached with a torch.Generator or with none (the launch trace of those calls, op by op,
    is held by tests/test_denoise_trace_host.py against its golden file); two runs agree."""
    from lavie_amd import ops as o
    pe, ne = prompts
    pipe = pipe_of(small)
    reached = []
    for name in ("philox_normal", "sampler_step_seeded", "cfg_sampler_step_seeded", "window_step_seeded"):
        monkeypatch.setattr(o, name, lambda *a, _n=name, **k: reached.append(_n))
    a = call(pipe, pe[:1], ne[:1], torch.Generator().manual_seed(5))
    b = call(pipe, pe[:1], ne[:1], torch.Generator().manual_seed(5))
    w = call(pipe, pe[:1], ne[:1], torch.Generator().manual_seed(5), frames=11, window_length=8, window_stride=3)
    torch.manual_seed(5)
    call(pipe, pe[:1], ne[:1], None)
    assert reached == [] and torch.equal(a, b) and torch.isfinite(w).all()


def test_free_init_with_a_philox_generator_runs_and_reproduces(small, prompts):
    from lavie_amd.noise import PhiloxGenerator
    pe, ne = prompts
    pipe = pipe_of(small)
    a = call(pipe, pe[:1], ne[:1], PhiloxGenerator(21), free_init=dict(num_iters=2))
    b = call(pipe, pe[:1], ne[:1], PhiloxGenerator(21), free_init=dict(num_iters=2))
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, call(pipe, pe[:1], ne[:1], PhiloxGenerator(21)))
