"""-m gpu: FreeInit.  The fused frequency mix (lavie_freq_mix_f32, csrc/freq_mix.hip) per element against the
float64 model of tests/freeinit_reference.py, which evaluates the published two-transform formula literally; its structure
(all-stop and all-pass filters, the DC mode, single cosines under the ideal filter); its bit guarantees; the refusals of the C ABI;
and the pipeline's iterations against a loop written here around plain pipeline calls.

The bound on the op's fp32 output is set per case by an independent fp32 implementation: the same formula through torch's
float32 torch.fft on the CPU, whose largest error against float64 the kernel may exceed 4 times (a straight N-term fp32 sum
against an FFT's log N growth).  Both numbers are printed; the figures measured on an MI355X are in DESIGN.md 7.15."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import freeinit_cases as C
import freeinit_reference as R
import layercache_cases as LC
import opcheck as oc
from gpu_util import TOL_UNET, rel_l2

pytestmark = pytest.mark.gpu
f16, f32t = torch.float16, torch.float32
MARGIN = 4.0


def sync():
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ops():
    from lavie_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def reference(shape, method, r):
    """(inputs, filter for the kernel, float64 result, largest error of the float32 torch.fft evaluation), computed once per case."""
    from lavie_amd.free_init import freq_filter
    x0, e0, z = C.op_inputs(shape)
    a, s = C.noise_level()
    lpf = R.published_filter(*shape[1:], method, C.ORDER, C.DS, C.DT)
    ref = R.mix(x0, e0, z, a, s, r, lpf).real
    err32 = float((R.mix(x0, e0, z, a, s, r, lpf, torch.float32).real.double() - ref).abs().max())
    return (x0, e0, z), freq_filter(*shape[1:], method, C.ORDER, C.DS, C.DT), ref, err32


def run_mix(ops, ins, filt, a, s, r, dup=2, in_scale=C.IN_SCALE, alias=False):
    """ops.freq_mix on guarded operands (opcheck.run_guarded: bands, poison, two runs bit for bit) -> {"out", "model_in"}."""
    x0, e0, z = ins
    inputs = {"x0": x0, "e0": e0, "z": z, "filt": filt}
    shape = tuple(x0.shape)
    outs = {"out": (shape, f32t)}
    if dup:
        outs["model_in"] = ((dup * shape[0],) + shape[1:], f16)

    def run(i, o):
        ops.freq_mix(i["x0"], i["e0"], i["z"], i["filt"], a, s, r, out=o["out"], model_in=o.get("model_in"), input_scale=in_scale)

    return oc.run_guarded(run, inputs, outs, alias={"out": "x0"} if alias else None, sync=sync)


def fp16_of_product(out, scale):
    """fp16(out * scale) rounded once: the product of two fp32 values is exact in float64, numpy rounds float64 -> float16 directly."""
    return torch.from_numpy((out.double().numpy() * np.float64(np.float32(scale))).astype(np.float16))


# ------------------------------------------------------------------ 1. per element against float64
OP_IDS = ["x".join(map(str, shape)) + "-" + m for shape, m in C.OP_CASES]


@pytest.mark.parametrize("r", C.R_VALUES, ids=["r1", "r1.7"])
@pytest.mark.parametrize("shape,method", C.OP_CASES, ids=OP_IDS)
def test_mix_per_element_vs_float64(ops, shape, method, r):
    ins, filt, ref, err32 = reference(shape, method, r)
    a, s = C.noise_level()
    res = run_mix(ops, ins, filt, a, s, r, dup=2)
    err = float((res["out"].double() - ref).abs().max())
    print(f"freq_mix {shape} {method} r={r}: kernel max |err| {err:.3e}, torch fp32 fft max |err| {err32:.3e}, ratio {err / err32:.2f}")
    assert torch.isfinite(res["out"]).all()
    assert err <= MARGIN * err32, (shape, method, r, err, err32)
    want = fp16_of_product(res["out"], C.IN_SCALE)
    for j, part in enumerate(res["model_in"].reshape(2, -1)):
        oc.assert_bits(part, want.reshape(-1), label=f"model_in copy {j} vs fp16(input_scale out)")


# ------------------------------------------------------------------ 2. structure
STRUCT_SHAPES = [(3, 5, 6, 8), (2, 61, 10, 12), (4, 16, 40, 64)]


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_all_stop_filter_is_the_fresh_noise_bit_for_bit(ops, shape):
    ins = C.op_inputs(shape, seed=1)
    a, s = C.noise_level()
    for r in C.R_VALUES:
        res = run_mix(ops, ins, torch.zeros(shape[1:]), a, s, r, dup=1)
        want = torch.from_numpy(ins[2].numpy() * np.float32(r))
        oc.assert_bits(res["out"], want, label=f"filter = 0, r = {r}")
        oc.assert_bits(res["model_in"], fp16_of_product(want, C.IN_SCALE), label="model_in at filter = 0")


@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_all_pass_filter_is_the_renoised_result(ops, shape):
    x0, e0, z = C.op_inputs(shape, seed=2)
    a, s = C.noise_level()
    ones = torch.ones(shape[1:], dtype=torch.float64)
    ref = R.mix(x0, e0, z, a, s, 1.7, ones).real
    assert float((ref - (a * x0.double() + s * e0.double())).abs().max()) < 1e-12          # the model itself: z_T
    err32 = float((R.mix(x0, e0, z, a, s, 1.7, ones, torch.float32).real.double() - ref).abs().max())
    res = run_mix(ops, (x0, e0, z), ones.float(), a, s, 1.7, dup=0)
    err = float((res["out"].double() - ref).abs().max())
    print(f"all-pass {shape}: kernel {err:.3e}, torch fp32 {err32:.3e}")
    assert err <= MARGIN * err32


def test_dc_filter_returns_the_constant(ops):
    """x0 constant per image, e0 = z = 0, a = 1 and a filter that keeps only frequency 0: the constant comes back.  Bound: the three
    forward sums add W, H, F equal terms one after the other (relative error <= (W + H + F) u), every other product is by an exact
    1 or 0 but the final 1 / (F H W): (W + H + F + 8) 2^-23 |c|."""
    shape = (3, 5, 6, 8)
    consts = torch.tensor([0.7310585, -2.5, 1e-3])
    x0 = consts.view(3, 1, 1, 1).expand(shape).contiguous()
    zero = torch.zeros(shape)
    filt = torch.zeros(shape[1:])
    filt[0, 0, 0] = 1.0
    res = run_mix(ops, (x0, zero, zero.clone()), filt, 1.0, 0.5, 1.0, dup=0)
    bound = (sum(shape[1:]) + 8) * oc.U32 * consts.abs().double().view(3, 1, 1, 1)
    assert bool(((res["out"].double() - x0.double()).abs() <= bound).all())


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["F", "H", "W"])
def test_single_cosines_under_the_ideal_filter(ops, axis):
    """One cosine of frequency m along one axis (e0 = z = 0, a = 1): kept when the ideal filter passes (+m, -m), otherwise replaced by
    the (zero) fresh noise; what the filter does at +-m is read off the published filter.  Bound: amplitude 1, sums of up to
    W + H + F terms forward and as many inverse, 2 (W + H + F + 8) 2^-23."""
    from lavie_amd.free_init import freq_filter
    shape = (16, 12, 20)
    n = shape[axis]
    lpf = R.published_filter(*shape, "ideal", C.ORDER, C.DS, C.DT)
    centre = [v // 2 for v in shape]
    seen = set()
    for m in range(1, n // 2):
        plus, minus = list(centre), list(centre)
        plus[axis] += m
        minus[axis] -= m
        keep = float(lpf[tuple(plus)] + lpf[tuple(minus)]) / 2
        assert keep in (0.0, 1.0)
        seen.add(keep)
        view = [1, 1, 1]
        view[axis] = n
        wave = torch.cos(2 * torch.pi * m * torch.arange(n, dtype=torch.float64) / n).view(view).expand(shape)
        x0 = wave.float().unsqueeze(0).contiguous()
        zero = torch.zeros_like(x0)
        out = ops.freq_mix(x0.cuda(), zero.cuda(), zero.cuda(), freq_filter(*shape, "ideal", C.ORDER, C.DS, C.DT).cuda(), 1.0, 0.0, 1.0)
        err = float((out.cpu().double() - keep * x0.double()).abs().max())
        assert err <= 2 * (sum(shape) + 8) * oc.U32, (axis, m, keep, err)
    assert seen == {0.0, 1.0}                    # both outcomes occur along every axis


# ------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("shape", [(3, 5, 6, 8), (2, 61, 10, 12), (2, 8, 65, 33)], ids=lambda s: "x".join(map(str, s)))
def test_bit_guarantees(ops, shape):
    ins, filt, _, _ = reference(shape, "butterworth", 1.7)
    a, s = C.noise_level()
    dev = [t.cuda() for t in ins]
    fd = filt.cuda()
    first = ops.freq_mix(*dev, fd, a, s, 1.7)
    assert torch.equal(ops.freq_mix(*dev, fd, a, s, 1.7), first)                       # two calls
    for j in range(shape[0]):                                                          # image j alone
        single = ops.freq_mix(*(t[j:j + 1].contiguous() for t in dev), fd, a, s, 1.7)
        assert torch.equal(single[0], first[j]), j
    aliased = run_mix(ops, ins, filt, a, s, 1.7, dup=1, alias=True)                    # out = x0
    oc.assert_bits(aliased["out"], first.cpu(), label="out aliasing x0")
    want = fp16_of_product(first.cpu(), C.IN_SCALE).reshape(-1)
    for dup in (1, 2, 3):
        res = run_mix(ops, ins, filt, a, s, 1.7, dup=dup)
        oc.assert_bits(res["out"], first.cpu(), label=f"out with dup = {dup}")
        for j, part in enumerate(res["model_in"].reshape(dup, -1)):
            oc.assert_bits(part, want, label=f"copy {j} of {dup}")


# ------------------------------------------------------------------ 4. refusals through the C ABI
def test_c_abi_refusals_touch_nothing(ops):
    from lavie_amd import _lib
    lib = _lib.load()
    shape = (3, 5, 6, 8)
    n = 3 * 5 * 6 * 8
    t = {k: oc.guarded(shape, f32t, fill="finite") for k in ("x0", "e0", "z", "out")}
    filt = oc.guarded(shape[1:], f32t, fill="finite")
    min_ = oc.guarded((3 * n,), f16, fill="nan")
    need = lib.lavie_freq_mix_workspace_bytes(*shape)
    assert need == ops.freq_mix_workspace_bytes(*shape) == 2 * 8 * n
    ws = oc.guarded((need // 4,), f32t, fill="nan")

    def args(**over):
        a = _lib.FreqMixArgsC()
        a.struct_size = ctypes.sizeof(_lib.FreqMixArgsC)
        a.images, a.F, a.H, a.W = shape
        a.x0, a.e0, a.z, a.out = (t[k].t.data_ptr() for k in ("x0", "e0", "z", "out"))
        a.filter = filt.t.data_ptr()
        a.a, a.s, a.r = 0.1, 0.9, 1.0
        a.model_in, a.dup, a.dup_stride, a.input_scale = min_.t.data_ptr(), 3, n, 1.0
        a.workspace, a.workspace_bytes = ws.t.data_ptr(), need
        for k, v in over.items():
            setattr(a, k, v)
        return a

    cases = [(dict(struct_size=8), "struct_size"), (dict(x0=None), "x0 is null"), (dict(e0=None), "e0 is null"), (dict(z=None), "z is null"),
             (dict(filter=None), "filter is null"), (dict(out=None), "out is null"), (dict(workspace=None), "workspace is null"),
             (dict(workspace_bytes=need - 1), "workspace_bytes"), (dict(images=0), "images=0"), (dict(F=0), "F=0"), (dict(F=257), "F=257"),
             (dict(H=129), "H=129"), (dict(H=0), "H=0"), (dict(W=129), "W=129"), (dict(W=0), "W=0"), (dict(dup=0), "dup=0"),
             (dict(dup=4), "dup=4"), (dict(dup_stride=n - 1), "dup_stride"), (dict(a=float("nan")), "must be finite"),
             (dict(out=t["z"].t.data_ptr()), "out and z overlap"), (dict(out=t["e0"].t.data_ptr() + 4), "out and e0 overlap")]
    for over, text in cases:
        rc = lib.lavie_freq_mix_f32(ctypes.byref(args(**over)), None)
        assert rc != 0 and text in lib.lavie_last_error().decode(), (over, lib.lavie_last_error())
    assert lib.lavie_freq_mix_f32(None, None) != 0 and b"args is null" in lib.lavie_last_error()
    for bad in ((0, 5, 6, 8), (1, 257, 6, 8), (1, 5, 129, 8), (1, 5, 6, 129), (1, 0, 6, 8)):
        assert lib.lavie_freq_mix_workspace_bytes(*bad) == 0
    sync()
    for k, g in {**t, "filter": filt, "model_in": min_, "workspace": ws}.items():
        g.check_bands(k)
        if k in ("model_in", "workspace"):
            assert g.unwritten().numel() == g.n, k
        else:
            g.check_unchanged(k)
    assert lib.lavie_freq_mix_f32(ctypes.byref(args()), None) == 0          # the unmodified record goes through
    sync()
    assert min_.unwritten().numel() == 0


# ------------------------------------------------------------------ 5. the pipeline
STEPS, GUIDANCE = 3, 7.5


def build(sd, **kw):
    from lavie_amd.unet import UNet3DConditionModel
    net = UNet3DConditionModel(init_weights=False, **kw)
    net.load_state_dict({k: v.to(f16) for k, v in sd.items()})
    return net.to("cuda", f16)


@pytest.fixture(scope="module")
def base():
    net = build(LC.base_weights(), **LC.BASE_KW)
    yield net
    net.disable_layer_cache()


def scheduler_of(name):
    if name == "ddpm":
        from lavie_amd.scheduling_ddpm import DDPMScheduler
        return DDPMScheduler()
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler()


def pipeline_inputs(frames):
    g = torch.Generator().manual_seed(77)
    return torch.randn(2, 77, 128, generator=g).half().cuda(), (1, 4, frames, 16, 16)


PIPE_CASES = [("ddpm", 4, {}), ("dpm", 4, {}), ("ddpm", 6, dict(window_length=4, window_stride=2)), ("dpm", 6, dict(window_length=4, window_stride=2)),
              ("ddpm", 4, dict(cache_interval=2)), ("dpm", 4, dict(cache_interval=2))]


@pytest.mark.parametrize("sched,frames,extra", PIPE_CASES, ids=[f"{s}-F{f}-{'-'.join(e) or 'plain'}" for s, f, e in PIPE_CASES])
def test_pipeline_iterations_vs_plain_calls(base, sched, frames, extra):
    """num_iters = 1 is the plain call bit for bit; num_iters = 2 is two plain calls with the float64 model's mix in between, inside
    the whole-forward tolerance the three-step trajectory tests use (gpu_util.TOL_UNET on the final latents); a seeded call is
    reproducible bit for bit."""
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddpm import randn_tensor
    pipe = VideoGenPipeline(unet=base, scheduler=scheduler_of(sched))
    ctx, shape = pipeline_inputs(frames)

    def draw(g):
        return randn_tensor(shape, generator=g, device=torch.device("cuda"), dtype=f32t)

    def plain(latents, g, **kw):
        return pipe.denoise(latents, ctx, STEPS, GUIDANCE, generator=g, **extra, **kw)

    g = torch.Generator().manual_seed(5)
    e0 = draw(g)
    x1 = plain(e0, g)
    z = draw(g)
    a, s = pipe.scheduler.noise_level(pipe.scheduler.config.num_train_timesteps - 1)
    lpf = R.published_filter(*shape[2:], "butterworth", C.ORDER, C.DS, C.DT)
    mixed = R.mix(x1.cpu(), e0.cpu(), z.cpu(), a, s, 1.0, lpf).real.float().cuda()
    want = plain(mixed, g)

    g = torch.Generator().manual_seed(5)
    one = plain(draw(g), g, free_init=dict(num_iters=1))
    assert torch.equal(one, x1)
    runs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(5)
        steps = []
        runs.append(plain(draw(g), g, free_init=dict(num_iters=2), callback=lambda i, t, x: steps.append(i)))
        assert steps == list(range(STEPS)) * 2                 # the step index restarts with each iteration
    assert torch.equal(runs[0], runs[1])
    err = rel_l2(runs[0], want)
    print(f"free_init {sched} F={frames} {extra}: rel-L2 against two plain calls {err:.2e}; against the first iteration {rel_l2(runs[0], x1):.2e}")
    assert torch.isfinite(runs[0]).all() and err < TOL_UNET
    assert not torch.equal(runs[0], x1)
    # the setting on the pipeline is the keyword
    pipe.enable_free_init(num_iters=2)
    g = torch.Generator().manual_seed(5)
    assert torch.equal(plain(draw(g), g), runs[0])
    pipe.disable_free_init()
    g = torch.Generator().manual_seed(5)
    assert torch.equal(plain(draw(g), g), x1)


class Counting:
    """A UNet-shaped callable that counts its forwards and hands everything else to the model."""

    def __init__(self, net):
        self._net, self.calls = net, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self._net(*a, **kw)

    def __getattr__(self, name):
        return getattr(self._net, name)


def test_fast_sampling_takes_the_step_counts(base):
    from lavie_amd.free_init import FreeInit
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    counting = Counting(base)
    pipe = VideoGenPipeline(unet=counting, scheduler=scheduler_of("ddpm"))
    ctx, shape = pipeline_inputs(4)
    lat = torch.randn(shape, generator=torch.Generator().manual_seed(9)).cuda()
    setting = FreeInit(num_iters=3, use_fast_sampling=True)
    want = [setting.steps_at(i, STEPS) for i in range(3)]
    assert want == [1, 2, 3]
    seen = []
    pipe.denoise(lat, ctx, STEPS, GUIDANCE, generator=torch.Generator().manual_seed(1), free_init=setting,
                 callback=lambda i, t, x: seen.append(i))
    assert counting.calls == sum(want) and seen == [0, 0, 1, 0, 1, 2]
    counting.calls = 0
    pipe.denoise(lat, ctx, STEPS, GUIDANCE, generator=torch.Generator().manual_seed(1), free_init=dict(num_iters=3))
    assert counting.calls == 3 * STEPS
    with pytest.raises(ValueError, match="known latents"):
        pipe.denoise(lat, ctx, STEPS, GUIDANCE, known=lat, free_init=setting)
    assert counting.calls == 3 * STEPS                      # refused before anything reached the engine
