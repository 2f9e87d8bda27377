"""UniPC before a GPU is involved: the scheduler mirror against the independent float64 restatement of
tests/unipc_reference.py, the solver's accuracy on a Gaussian problem with a closed-form solution, the step kinds, the refusals, the
C entries' argument checks through ctypes, and the launches of a traced denoising loop."""
import ctypes
import math
import os
import types

import pytest
import torch

import unipc_reference as R
from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
from lavie_amd.scheduling_unipc_multistep import UniPCCoefficients, UniPCMultistepScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drive(scheduler, model, x, keep=None):
    for t in [int(v) for v in scheduler.timesteps]:
        out = model(x, t)
        nxt = scheduler.step(out, t, x).prev_sample
        if keep is not None:
            keep.append((x, out, nxt))
        x = nxt
    return x


# ------------------------------------------------------------------ 1. the mirror against the reference
def step_bound(timesteps, ab):
    """Per-step bound on |mirror - reference| in units of M, the sum of the magnitudes of a step's terms.

    Both sides evaluate, in float64 (unit roundoff u = 2^-53), the same linear combination of at most four terms (x_last, m, m1,
    m2) from the same inputs; they differ in how the scalars are formed (the reference keeps differences D / r and the integrals
    I_k, the mirror folds everything into ten coefficients with diffusers' phi recursion) and in the order of the sum.
      * x0 prediction, the folded coefficients and the sum: under 32 operations on either side, each a relative perturbation of at
        most u on an intermediate that M bounds: 64 u M for the two sides together.
      * the right-hand side b_2 of the order-2 corrector's system is a cancelling difference on both sides: I_2 = h^2 / 2 - I_1
        with I_1 = h - I_0 (reference), (phi / (-h) - 1 / 2) with phi = expm1(-h) / (-h) - 1 (mirror).  The operands are O(h^2)
        resp. O(1) with absolute error 3 u h^2 resp. 3 u, the results h^3 / 6 resp. h / 6: a relative error of 18 u / h^2 each.
        rho = solve([[1, 1], [r, 1]], b) has condition below 4 / |1 - r| <= 4 (r < 0), and rho enters terms that M bounds: at most
        2 * 4 * 18 u / h^2 M, rounded up to 256 u / h^2 for the solve's own roundings.
    h is the smallest lambda step of the table."""
    lam = [R.level(ab[t])[2] for t in timesteps]
    h_min = min((b - a for a, b in zip(lam, lam[1:])), default=1.0)
    return (64.0 + 256.0 / h_min ** 2) * R.U64


@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("steps", [1, 2, 3, 10, 20])
def test_step_and_coefficients_reproduce_the_reference_trajectory(steps, order, prediction):
    """`coefficients()` and `step()` against unipc_reference.trajectory with a non-linear model.
    1. `coefficients()`, position by position, no accumulation: the kernel's form evaluated from the reference's own states must
       give the reference's m, x^c and x' within step_bound * M, M the sum of the magnitudes of the terms of each.
    2. `step()` along its own trajectory.  A difference made at position j travels on through the remaining steps like a
       perturbation of the state there.  How much the reference itself amplifies a perturbation is measured on the reference (S:
       the largest |x_i(start + d) - x_i(start)| / |d| over the positions for a 1e-6 perturbation of the start, per element, at
       least 1); position i is then held to (i + 1) * 2 S * step_bound * M_max, the factor 2 for a perturbation that enters
       through the history (m1, m2) as well as through the sample.  An estimate written down, not a proof; the measured
       differences are ~1e-15."""
    ab, ts = R.abar_table(), R.leading_timesteps(steps)
    g = torch.Generator().manual_seed(steps * 10 + order)
    x_start = torch.randn(32, generator=g, dtype=torch.float64)
    shift = torch.randn(32, generator=g, dtype=torch.float64)
    model = lambda x, t: torch.tanh(0.7 * x + shift * (t / 1000.0))      # noqa: E731
    ref_keep, moved_keep, got_keep = [], [], []
    ref = R.trajectory(model, x_start, ts, ab, order=order, prediction=prediction, keep=ref_keep)
    R.trajectory(model, x_start + 1e-6, ts, ab, order=order, prediction=prediction, keep=moved_keep)
    sens = max(1.0, max(float((a[4] - b[4]).abs().max()) / 1e-6 for a, b in zip(ref_keep, moved_keep)))
    sch = UniPCMultistepScheduler(solver_order=order, prediction_type=prediction)
    sch.set_timesteps(steps)
    assert [int(t) for t in sch.timesteps] == ts
    bound = step_bound(ts, ab)
    x_last = m1 = m2 = torch.zeros_like(x_start)
    m_max = 0.0
    for i, (x, out, x_c, m, x_next) in enumerate(ref_keep):
        c = sch.coefficients(ts[i])
        m_k = c.k_x * x - c.k_eps * out
        mag_m = abs(c.k_x) * x.abs() + abs(c.k_eps) * out.abs()
        if c.corr:
            xc_k = c.c_l * x_last + c.c_0 * m_k + c.c_1 * m1 + c.c_2 * m2
            mag_c = abs(c.c_l) * x_last.abs() + abs(c.c_0) * mag_m + abs(c.c_1) * m1.abs() + abs(c.c_2) * m2.abs()
        else:
            xc_k, mag_c = x, x.abs()
        xn_k = c.p_x * xc_k + c.p_0 * m_k + c.p_1 * m1
        mag_n = abs(c.p_x) * mag_c + abs(c.p_0) * mag_m + abs(c.p_1) * m1.abs()
        for what, a, b, mag in (("m", m_k, m, mag_m), ("xc", xc_k, x_c, mag_c), ("x'", xn_k, x_next, mag_n)):
            assert ((a - b).abs() <= bound * mag).all(), (i, what, float(((a - b).abs() / mag).max()), bound)
        m_max = max(m_max, float(mag_n.max()), float(mag_c.max()))
        x_last, m1, m2 = x_c, m, m1
    got = drive(sch, model, x_start, got_keep)
    worst = 0.0
    for i, ((_, _, _, _, want), (_, _, have)) in enumerate(zip(ref_keep, got_keep)):
        worst = max(worst, float((have - want).abs().max()))
        assert float((have - want).abs().max()) <= (i + 1) * 2.0 * sens * bound * m_max, i
    assert torch.equal(got, got_keep[-1][2]) and float((got - ref).abs().max()) <= steps * 2.0 * sens * bound * m_max
    print(f"steps={steps} order={order} {prediction}: worst |step() - reference| {worst:.2e}, S = {sens:.2f}, step bound {bound:.2e} M")


# ------------------------------------------------------------------ 2. ground truth without any sampler
def _via(make):
    def solver(model, x, ts, ab):
        sch = make()
        sch.set_timesteps(len(ts))
        assert [int(t) for t in sch.timesteps] == ts
        return drive(sch, model, x)
    return solver


def test_gaussian_closed_form_orderings():
    """Data N(mu, s^2) per element: the exact noise prediction and the probability-flow ODE's closed form (unipc_reference).  At 10,
    20 and 40 steps UniPC's end error is below DPM-Solver++ 2M's (this package's, landing on the same sigma = 0) and below UniPC's
    with the corrector disabled, and it shrinks with the step count.  Orderings, not tolerances: s = 0.06 is chosen so that the
    float64 reference satisfies them (the reference's own figures are asserted first); for s in 0.1 .. 32 it does not, see
    unipc_reference.gaussian_case.  Measured (max |x_0 - closed form| over 64 elements):
        N      UniPC       no corrector = DPM-Solver++ 2M     order 1
        10     7.177e-02   7.189e-02                          9.934e-02
        20     3.962e-02   3.992e-02                          7.870e-02
        40     1.016e-02   1.079e-02                          5.257e-02"""
    counts = (10, 20, 40)
    ref = [R.gaussian_end_error(lambda m, x, ts, ab: R.trajectory(m, x, ts, ab), n) for n in counts]
    ref_p = [R.gaussian_end_error(lambda m, x, ts, ab: R.trajectory(m, x, ts, ab, corrector=False), n) for n in counts]
    assert all(a < b for a, b in zip(ref, ref_p)) and ref[0] > ref[1] > ref[2]          # the reference alone
    uni = [R.gaussian_end_error(_via(UniPCMultistepScheduler), n) for n in counts]
    off = [R.gaussian_end_error(_via(lambda: UniPCMultistepScheduler(disable_corrector=list(range(n)))), n) for n in counts]
    dpm = [R.gaussian_end_error(_via(lambda: DPMSolverMultistepScheduler(set_alpha_to_one=True)), n) for n in counts]
    for n, a, b, c, d in zip(counts, uni, off, dpm, ref):
        print(f"N={n}: UniPC {a:.3e}  corrector off {b:.3e}  DPM-Solver++ 2M {c:.3e}  reference {d:.3e}")
    assert all(a < c for a, c in zip(uni, dpm))
    assert all(a < b for a, b in zip(uni, off))
    assert uni[0] > uni[1] > uni[2]


# ------------------------------------------------------------------ 3. the step kinds
def test_step_kinds():
    sch = UniPCMultistepScheduler()
    sch.set_timesteps(10)
    ts = [int(t) for t in sch.timesteps]
    assert ts == [901 - 100 * i for i in range(10)]
    cs = [sch.coefficients(t) for t in ts]
    assert all(isinstance(c, UniPCCoefficients) for c in cs)
    first, second, middle, last = cs[0], cs[1], cs[5], cs[-1]
    assert not first.corr and first.p_1 == 0.0 and (first.c_l, first.c_0, first.c_1, first.c_2) == (0.0, 0.0, 0.0, 0.0)
    # the step after the first: the corrector has the order of the first predictor (1: rho = 1/2, no m2); the predictor is order 2
    assert second.corr and second.c_2 == 0.0 and second.c_0 == second.c_1 != 0.0 and second.p_1 != 0.0
    assert middle.corr and middle.c_2 != 0.0 and middle.p_1 != 0.0
    # the last step: a second-order corrector, then a first-order predictor onto sigma = 0, which returns the x0 prediction
    assert last.corr and last.c_2 != 0.0 and (last.p_x, last.p_0, last.p_1) == (0.0, 1.0, 0.0)
    assert [sch.predictor_order(i) for i in range(10)] == [1] + [2] * 8 + [1]
    # the corrector's and the predictor's coefficients are consistent updates: a constant x0 prediction m and the matching
    # sample x = alpha m + sigma e stay on that line (the coefficients of m and of the previous sample sum as the exact solution's)
    for i, c in enumerate(cs[1:], 1):
        a_p, s_p = sch.noise_level(ts[i - 1])
        a_i, s_i = sch.noise_level(ts[i])
        assert abs(c.c_l - s_i / s_p) < 1e-15 and abs(c.c_l * a_p + c.c_0 + c.c_1 + c.c_2 - a_i) < 1e-12
    # without lower_order_final the last step is first order all the same (its target has sigma = 0); order 1 never reads m2
    free = UniPCMultistepScheduler(lower_order_final=False)
    free.set_timesteps(10)
    assert free.coefficients(ts[-1]) == last
    one = UniPCMultistepScheduler(solver_order=1)
    one.set_timesteps(10)
    assert all(c.c_2 == 0.0 and c.p_1 == 0.0 for c in (one.coefficients(t) for t in ts))
    # disable_corrector lists the positions whose prediction stays uncorrected
    off = UniPCMultistepScheduler(disable_corrector=[0, 4])
    off.set_timesteps(10)
    assert [off.coefficients(t).corr for t in ts] == [False, False, True, True, True, False, True, True, True, True]
    # step(): the last step returns its x0 prediction; steps out of order are refused; position 0 starts afresh
    x = torch.randn(8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for t in ts:
        out = sch.step(0.3 * x, t, x)
        x = out.prev_sample
    assert torch.equal(out.prev_sample, out.pred_original_sample)
    with pytest.raises(ValueError, match="expected position"):
        sch.step(x, ts[3], x)
    sch.step(x, ts[0], x)
    assert sch.scale_model_input(x, ts[0]) is x and sch.init_noise_sigma == 1.0 and sch.noise_level(None) == (1.0, 0.0)
    assert sch.unipc and not getattr(sch, "multistep", False)


# ------------------------------------------------------------------ 4. refusals and from_config
@pytest.mark.parametrize("key,value", [("solver_type", "bh1"), ("solver_order", 3), ("predict_x0", False), ("thresholding", True),
                                       ("use_karras_sigmas", True), ("timestep_spacing", "trailing"), ("timestep_spacing", "linspace"),
                                       ("final_sigmas_type", "sigma_min"), ("beta_schedule", "squaredcos_cap_v2")])
def test_constructor_refuses_by_name(key, value):
    with pytest.raises(NotImplementedError, match=key if key != "beta_schedule" else "squaredcos"):
        UniPCMultistepScheduler(**{key: value})
    with pytest.raises(NotImplementedError):
        UniPCMultistepScheduler.from_config({key: value})


def test_from_config():
    with pytest.raises(ValueError, match="prediction_type"):
        UniPCMultistepScheduler(prediction_type="flow")
    cfg = {"_class_name": "UniPCMultistepScheduler", "_diffusers_version": "0.27.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
           "beta_start": 0.00085, "disable_corrector": [], "dynamic_thresholding_ratio": 0.9, "lower_order_final": True,
           "num_train_timesteps": 1000, "predict_x0": True, "prediction_type": "v_prediction", "sample_max_value": 2.5,
           "solver_order": 2, "solver_p": None, "solver_type": "bh2", "steps_offset": 1, "thresholding": False,
           "timestep_spacing": "leading", "trained_betas": None, "use_karras_sigmas": False, "clip_sample": False,
           "final_sigmas_type": "zero", "rescale_betas_zero_snr": False}
    sch = UniPCMultistepScheduler.from_config(cfg)          # inert keys (thresholding's two, clip_sample, the underscore keys) load
    assert sch.config.prediction_type == "v_prediction" and sch.config.beta_schedule == "scaled_linear"
    assert UniPCMultistepScheduler.from_config(sch.config, solver_order=1).config.solver_order == 1
    for key, value in (("use_exponential_sigmas", True), ("use_beta_sigmas", True), ("use_flow_sigmas", True),
                       ("rescale_betas_zero_snr", True), ("solver_p", "dpm")):
        with pytest.raises(NotImplementedError, match=key):
            UniPCMultistepScheduler.from_config(dict(cfg, **{key: value}))
    with pytest.raises(TypeError, match="nonsense"):
        UniPCMultistepScheduler.from_config(cfg, nonsense=1)
    with pytest.raises(ValueError):
        UniPCMultistepScheduler().set_timesteps(0)
    with pytest.raises(ValueError, match="set_timesteps"):
        UniPCMultistepScheduler().coefficients(1)


# ------------------------------------------------------------------ 5. the C entries refuse bad arguments before any HIP call
def test_c_entries_refuse_bad_arguments_before_any_hip_call():
    from lavie_amd import _lib
    lib = _lib.load()
    ptr = lambda k: ctypes.c_void_p(1 << 20 | k << 12)     # noqa: E731  (never dereferenced: every call below is refused on the host)
    eps, x, xl, m1, m2, mi, table = (ptr(k) for k in range(7))

    def coeffs(**kw):
        v = dict(struct_size=ctypes.sizeof(_lib.UnipcCoeffsC), corr=1, guidance=7.5, k_x=1.0, k_eps=0.5, c_l=0.9, c_0=0.05, c_1=0.04,
                 c_2=0.01, p_x=0.8, p_0=0.3, p_1=-0.1, next_input_scale=1.0)
        v.update(kw)
        return _lib.UnipcCoeffsC(**v)

    def refused(rc, text):
        assert rc != 0
        msg = lib.lavie_last_error().decode()
        assert text in msg, msg

    one, cfg, scaled = lib.lavie_unipc_step, lib.lavie_cfg_unipc_step, lib.lavie_cfg_unipc_step_scaled
    good = [eps, x, xl, m1, m2, mi]
    names = ["eps", "x", "x_last", "m1", "m2", "model_in"]
    for i, name in enumerate(names):
        args = list(good)
        args[i] = None
        refused(one(*args, 64, coeffs(), None), f"{name} is null")
        refused(cfg(*args, 64, coeffs(), None), f"{name} is null")
        refused(scaled(*args, 64, table, 32, coeffs(), None), f"{name} is null")
        args[i] = ctypes.c_void_p(good[i].value + 8)
        refused(one(*args, 64, coeffs(), None), f"{name} at")
        refused(cfg(*args, 64, coeffs(), None), "not 16-byte aligned")
        refused(scaled(*args, 64, table, 32, coeffs(), None), "not 16-byte aligned")
    refused(scaled(*good, 64, None, 32, coeffs(), None), "table is null")
    for n in (0, -1):
        refused(one(*good, n, coeffs(), None), "must be >= 1")
        refused(cfg(*good, n, coeffs(), None), "must be >= 1")
    refused(cfg(*good, 64, coeffs(struct_size=48), None), "struct_size")
    refused(one(*good, 64, coeffs(struct_size=0), None), "struct_size")
    for field in ("guidance", "k_x", "k_eps", "c_l", "c_0", "c_1", "c_2", "p_x", "p_0", "p_1", "next_input_scale"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(cfg(*good, 64, coeffs(**{field: bad}), None), f"{field} (")
            refused(one(*good, 64, coeffs(**{field: bad}), None), "not finite")
    refused(one(eps, x, x, m1, m2, mi, 64, coeffs(), None), "x and x_last overlap")
    refused(cfg(eps, x, xl, m1, ctypes.c_void_p(m1.value + 16), mi, 64, coeffs(), None), "m1 and m2 overlap")
    refused(scaled(*good, 64, table, 1, coeffs(), None), "per=1")
    refused(scaled(*good, 64, table, 24, coeffs(), None), "whole number")
    assert lib.lavie_abi_version() == 8 == _lib.ABI_VERSION                   # additive entries


def test_ops_refuse_host_tensors_and_wrong_sizes():
    from lavie_amd import ops
    x = torch.zeros(16)
    hist = (x.clone(), x.clone(), x.clone())
    c = UniPCCoefficients(1.0, 0.5, False, 0, 0, 0, 0, 0.8, 0.3, 0.0)
    half = lambda n: torch.zeros(n, dtype=torch.float16)      # noqa: E731
    with pytest.raises(ValueError):
        ops.cfg_unipc_step(half(32), x, hist, half(32), 7.5, c)
    with pytest.raises(ValueError):
        ops.unipc_step(half(16), x, hist, half(16), c)
    with pytest.raises(ValueError, match="history"):
        ops.unipc_step(half(16), x, hist[:2], half(16), c)
    with pytest.raises(ValueError, match="table"):
        ops.cfg_unipc_step_scaled(half(32), x, hist, half(32), None, c)


def test_driver_and_documents_carry_the_new_entries():
    """The stand-alone host-sanitizer program (`make asan`, run by tests/test_host_logic.py) exercises the three entries; the header,
    the binding and INTEGRATION.md name them."""
    from lavie_amd import _lib
    read = lambda *p: open(os.path.join(ROOT, *p)).read()      # noqa: E731
    driver, header, doc = read("lavie_amd", "csrc", "hostcheck", "driver.cpp"), read("include", "lavie_hip.h"), read("INTEGRATION.md")
    for name in ("lavie_unipc_step", "lavie_cfg_unipc_step", "lavie_cfg_unipc_step_scaled"):
        assert name + "(" in driver and name + "(" in header and name in _lib.SIGNATURES and name in doc
    assert ctypes.sizeof(_lib.UnipcCoeffsC) == 52


# ------------------------------------------------------------------ 6. the traced loop
class _StubUNet:
    class config:
        in_channels, sample_size = 4, 8
    device = torch.device("cpu")

    def __init__(self):
        self.forwards = 0

    def prepare(self, *a):
        pass

    def __call__(self, model_in, t, *more, encoder_hidden_states=None, **kw):
        self.forwards += 1
        return types.SimpleNamespace(sample=torch.zeros_like(model_in))


def _record(monkeypatch):
    from lavie_amd import ops, sampling
    calls = []
    names = ["latents_to_model_input", "latents_to_model_input1", "guidance_table"] + list(sampling.UNIPC_WRAPPERS.values()) + \
        sorted(set(sampling.STEP_WRAPPERS.values())) + ["window_step", "window_step_scaled", "known_blend", "freq_mix"]
    for name in names:
        monkeypatch.setattr(ops, name, (lambda n: (lambda *a, **k: calls.append((n, a)) or (k.get("out") if n == "guidance_table" else None)))(name))
    monkeypatch.setattr(ops, "guidance_partials_floats", lambda *a: 16)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: None)
    return calls


@pytest.mark.parametrize("guidance,wrapper", [(7.5, "cfg_unipc_step"), (1.0, "unipc_step"), ([5.0], "cfg_unipc_step_scaled")])
def test_traced_loop_launches_one_step_per_position(monkeypatch, guidance, wrapper):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    calls = _record(monkeypatch)
    net = _StubUNet()
    pipe = VideoGenPipeline(unet=net, scheduler=UniPCMultistepScheduler())
    pe = torch.zeros(1, 77, 16)
    seen = []
    pipe(prompt_embeds=pe, negative_prompt_embeds=pe, video_length=2, height=64, width=64, num_inference_steps=6,
         guidance_scale=guidance, output_type="latent", callback=lambda i, t, x: seen.append(t), cache_interval=None)
    steps = [c for c in calls if "step" in c[0]]
    assert [c[0] for c in steps] == [wrapper] * 6 and net.forwards == 6 and seen == [int(t) for t in pipe.scheduler.timesteps]
    assert sum(c[0] == "guidance_table" for c in calls) == (6 if wrapper.endswith("_scaled") else 0)
    x, hist = steps[0][1][1], steps[0][1][2]
    assert len(hist) == 3 and all(h.dtype == torch.float32 and h.shape == x.shape for h in hist)
    assert len({h.data_ptr() for h in hist} | {x.data_ptr()}) == 4
    assert all(c[1][2] is hist for c in steps)                            # allocated once per run
    coeffs = [c[1][-2] for c in steps]
    assert [c.corr for c in coeffs] == [False] + [True] * 5 and coeffs[0].p_1 == 0.0 and coeffs[1].c_2 == 0.0
    assert (coeffs[-1].p_x, coeffs[-1].p_0, coeffs[-1].p_1) == (0.0, 1.0, 0.0)
    # a second call starts with a fresh history: new buffers, position 0 again
    calls.clear()
    pipe(prompt_embeds=pe, negative_prompt_embeds=pe, video_length=2, height=64, width=64, num_inference_steps=3,
         guidance_scale=guidance, output_type="latent")
    again = [c for c in calls if "step" in c[0]]
    assert len(again) == 3 and again[0][1][2] is not hist and not again[0][1][-2].corr


def test_vsr_chunks_each_start_with_a_fresh_history(monkeypatch):
    from lavie_amd.vsr.pipeline import VideoUpscalePipeline, upscale_in_chunks
    calls = _record(monkeypatch)
    net = _StubUNet()
    net.config = types.SimpleNamespace(in_channels=7, sample_size=8)
    pipe = VideoUpscalePipeline(unet=net, scheduler=UniPCMultistepScheduler())
    pe = torch.zeros(1, 77, 16)
    upscale_in_chunks(pipe, torch.zeros(1, 3, 6, 4, 6), short_seq=4, num_inference_steps=3, prompt_embeds=pe, negative_prompt_embeds=pe,
                      generator=torch.Generator().manual_seed(0))
    steps = [c for c in calls if "step" in c[0]]
    assert [c[0] for c in steps] == ["cfg_unipc_step"] * 6
    assert [c[1][-2].corr for c in steps] == [False, True, True] * 2
    assert steps[0][1][2] is steps[2][1][2] and steps[3][1][2] is not steps[0][1][2]


def test_features_outside_the_claim_are_refused_by_name(monkeypatch):
    from lavie_amd import sampling
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.vsr.pipeline import VideoUpscalePipeline, upscale_in_chunks
    calls = _record(monkeypatch)
    pipe = VideoGenPipeline(unet=_StubUNet(), scheduler=UniPCMultistepScheduler())
    pe = torch.zeros(1, 77, 16)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=pe, video_length=4, height=32, width=48, num_inference_steps=3, output_type="latent")
    known = torch.zeros(1, 4, 4, 4, 6)
    for extra, text in ((dict(known_latents=known), "known_latents"), (dict(known_latents=known, known_mask=torch.ones(1, 1, 4, 4, 6)), "known_mask"),
                        (dict(video=torch.zeros(1, 4, 32, 48, 3, dtype=torch.uint8)), "video"), (dict(known_latents=known, strength=0.5), "strength"),
                        (dict(window_length=2), "window_length"), (dict(pag_scale=3.0), "pag_scale"),
                        (dict(free_init=dict(num_iters=2)), "FreeInit")):
        with pytest.raises(ValueError, match="UniPC") as e:
            pipe(**kw, **extra)
        assert text in str(e.value), (extra, str(e.value))
    lat = torch.zeros(1, 4, 4, 4, 6)
    ctx = torch.zeros(2, 77, 8, dtype=torch.float16)
    for extra, text in ((dict(known=lat), "known"), (dict(window_length=2), "window_length"), (dict(pag_scale=3.0), "pag_scale"),
                        (dict(free_init=dict(num_iters=2)), "free_init")):
        with pytest.raises(ValueError, match="UniPC") as e:
            pipe.denoise(lat, ctx, 3, 7.5, **extra)
        assert text in str(e.value)
    vsr_net = _StubUNet()
    vsr_net.config = types.SimpleNamespace(in_channels=7, sample_size=8)
    vsr = VideoUpscalePipeline(unet=vsr_net, scheduler=UniPCMultistepScheduler())
    with pytest.raises(ValueError, match="window_length"):
        upscale_in_chunks(vsr, torch.zeros(1, 3, 6, 4, 6), short_seq=4, overlap=2, num_inference_steps=3, prompt_embeds=pe,
                          negative_prompt_embeds=pe)
    assert not [c for c in calls if "step" in c[0]]
    assert all(("unipc", what) in sampling.REFUSED for what in ("known", "window_length", "pag", "free_init"))


class _CachingUNet(_StubUNet):
    layer_cache = 0

    def __init__(self):
        super().__init__()
        self.modes = []

    def enable_layer_cache(self, depth):
        self.layer_cache = depth

    def disable_layer_cache(self):
        self.layer_cache = 0

    def __call__(self, model_in, t, *more, layer_cache=None, **kw):
        self.modes.append(layer_cache)
        return super().__call__(model_in, t, *more, **kw)


def test_layer_cache_is_claimed(monkeypatch):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    calls = _record(monkeypatch)
    net = _CachingUNet()
    pipe = VideoGenPipeline(unet=net, scheduler=UniPCMultistepScheduler())
    pe = torch.zeros(1, 77, 16)
    pipe(prompt_embeds=pe, negative_prompt_embeds=pe, video_length=2, height=64, width=64, num_inference_steps=5, guidance_scale=7.5,
         output_type="latent", cache_interval=2)
    assert net.modes == ["refresh", "reuse", "refresh", "reuse", "refresh"] and net.layer_cache == 0
    assert [c[0] for c in calls if "step" in c[0]] == ["cfg_unipc_step"] * 5
