"""DPM-Solver++ multistep sampler, everything that needs no GPU: the scheduler against the reference's DDIM fixture (order 1),
against a problem with a known solution (order 2), `coefficients` against `step`, config handling, the C ABI's argument
refusals and the pipeline's dispatch."""
import ctypes
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dpm_reference as R
import golden_util as G
from lavie_amd import _lib
from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------ 1. order 1 is DDIM
def test_order_1_reproduces_the_reference_ddim_fixture():
    """DPM-Solver++ of order 1 is algebraically DDIM with eta = 0: every eta = 0 case of tests/golden/ddim_steps.pt (outputs of
    the reference's vendored DDIM class, all three prediction types) within the 5e-5 the DDIM mirror is held to on this fixture
    (tests/test_host_logic.py), and the same timesteps."""
    fx = G.load("ddim_steps.pt")
    cases = [dict(c, kind="epsilon", model_output=c["eps"]) for c in fx["cases"]] + list(fx["prediction_cases"])
    cases = [c for c in cases if c["eta"] == 0.0]
    assert {c["kind"] for c in cases} == {"epsilon", "v_prediction", "sample"} and len(cases) == 11
    for c in cases:
        sch = DPMSolverMultistepScheduler(solver_order=1, prediction_type=c["kind"])
        sch.set_timesteps(50)
        assert [int(t) for t in sch.timesteps[:5]] == list(fx["chain"]["timesteps"]) and int(sch.timesteps[-1]) == 1
        sch._next = sch._position(c["t"])              # a fixture case is one step out of the middle of a trajectory
        out = sch.step(c["model_output"], c["t"], c["x"])
        e_prev, e_x0 = rel(out.prev_sample, c["prev"]), rel(out.pred_original_sample, c["x0"])
        print(c["kind"], c["t"], f"prev {e_prev:.2e} x0 {e_x0:.2e}")
        assert e_prev < 5e-5 and e_x0 < 5e-5, (c["kind"], c["t"])
    # the whole timestep table is the DDIM mirror's, for both offsets
    from lavie_amd.scheduling_ddim import DDIMScheduler
    for off in (0, 1):
        a, b = DPMSolverMultistepScheduler(steps_offset=off), DDIMScheduler(steps_offset=off)
        for n in (4, 20, 50):
            a.set_timesteps(n)
            b.set_timesteps(n)
            assert torch.equal(a.timesteps, b.timesteps)


# ------------------------------------------------------------------ 2. known-solution accuracy
def product_error(steps, order, s):
    """The toy problem of dpm_reference.gaussian_flow_error through the product's `step()` in float64: linear betas 1e-4..0.02,
    1000 train steps, leading spacing, final step to abar = 1."""
    sch = DPMSolverMultistepScheduler(solver_order=order, set_alpha_to_one=True, steps_offset=0)
    sch.set_timesteps(steps)
    ts = [int(t) for t in sch.timesteps]
    assert ts == R.leading_timesteps(steps)
    return R.gaussian_flow_error(lambda i, t, eps, x: sch.step(eps, t, x).prev_sample, ts, R.abar_table(), s)


def test_known_solution_product_equals_restatement():
    """`step()` and the test-side float64 restatement (tests/dpm_reference.py, written from the paper's formulas) agree on the
    toy problem to float64 rounding, for both orders, so the figures below are the algorithm's and not one implementation's."""
    for steps in (10, 20, 40, 50):
        for order in (1, 2):
            for s in (0.5, 1.0, 2.0):
                a, b = product_error(steps, order, s), R.restated_error(steps, order, s)
                assert abs(a - b) < 1e-9, (steps, order, s, a, b)


def test_known_solution_order_2_beats_order_1():
    """Data N(0, s^2 I), s = 2, exact noise model and exact probability-flow solution (tests/dpm_reference.py); |x_0 - s| / s.
    (a) at 20, 40 and 50 steps order 2 has a strictly smaller error than order 1 at the same step count;
    (b) the order-2 error at 20 steps is no larger than the order-1 error at 40 steps.

    Measured (float64, CPU), order 1 / order 2:
        steps      s = 0.5              s = 1                s = 2
         10     0.2518 / 0.3818     0.1683 / 0.2965     0.1397 / 0.1429
         20     0.1326 / 0.2270     0.0875 / 0.1054     0.0724 / 0.0354
         40     0.0684 / 0.0801     0.0447 / 0.0277     0.0369 / 0.00818
         50     0.0551 / 0.0535     0.0359 / 0.0176     0.0296 / 0.00510
    What is NOT asserted, because it is not true: on this stiff toy problem the multistep solver is WORSE than order 1 (DDIM) at
    10 and 20 steps for s = 0.5 and s = 1 (s = 1, 20 steps: 0.105 against 0.087) and wins only from 40 steps on (s = 0.5: from
    50), and even at
    s = 2 order 2 at 20 steps (0.035) does not beat order 1 at 50 steps (0.030).  The feature is the sampler; none of this says
    that 20 steps replace 50, and nothing here is a statement about output quality on a trained model."""
    err = {(n, o): product_error(n, o, 2.0) for n in (20, 40, 50) for o in (1, 2)}
    print({k: f"{v:.5f}" for k, v in err.items()})
    for n in (20, 40, 50):
        assert err[(n, 2)] < err[(n, 1)], n
    assert err[(20, 2)] <= err[(40, 1)]
    want = {(20, 1): 0.0724, (20, 2): 0.0354, (40, 1): 0.0369, (40, 2): 0.00818, (50, 1): 0.0296, (50, 2): 0.00510}
    for k, v in want.items():                                         # the table above is this code's: three significant digits
        assert abs(err[k] - v) < 0.006 * v, (k, err[k])
    # the cases where the multistep solver loses stay visible: if one of these flips, the table in the docstring is stale
    assert product_error(20, 2, 1.0) > product_error(20, 1, 1.0) and product_error(10, 2, 0.5) > product_error(10, 1, 0.5)
    assert product_error(20, 2, 2.0) > product_error(50, 1, 2.0)


def test_known_solution_order_2_error_falls_3x_from_20_to_40_steps():
    """(c) From 20 to 40 steps the order-2 error falls by more than 3x (a first-order method: 2x).  Measured: 0.0354 -> 0.00818,
    4.3x; order 1: 0.0724 -> 0.0369, 1.96x."""
    e20, e40 = product_error(20, 2, 2.0), product_error(40, 2, 2.0)
    o20, o40 = product_error(20, 1, 2.0), product_error(40, 1, 2.0)
    print(f"order 2: {e20:.5f} -> {e40:.5f}, factor {e20 / e40:.2f}; order 1: factor {o20 / o40:.2f}")
    assert e20 / e40 > 3.0
    assert 1.8 < o20 / o40 < 2.2


# ------------------------------------------------------------------ 3. coefficients <-> step
@pytest.mark.parametrize("kind", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("steps,alpha_one", [(20, True), (20, False), (10, True), (10, False)])
def test_coefficients_are_the_step(kind, steps, alpha_one):
    """One kernel-form update in torch equals `step()` to fp32 rounding at every step of a run: the first (c_prev = 0), the
    last with sigma_t = 0 (c_xt == 0, c_x0 == 1, c_prev == 0), `lower_order_final` (10 steps < 15: the last step is first
    order; 20 steps: it is second order unless sigma_t = 0).  c_prev is h / (2 h_prev) from the log-SNRs, computed here."""
    sch = DPMSolverMultistepScheduler(prediction_type=kind, set_alpha_to_one=alpha_one)
    sch.set_timesteps(steps)
    ab = sch.alphas_cumprod.double().numpy()
    g = torch.Generator().manual_seed(steps)
    x = torch.randn(2, 4, 2, 8, 8, generator=g)
    xk, hist = x.clone(), None
    ts = [int(t) for t in sch.timesteps]
    for i, t in enumerate(ts):
        m = torch.randn(x.shape, generator=g)
        k_x, k_e, c_x0, c_xt, c_prev = sch.coefficients(t)
        last = i == steps - 1
        if i == 0:
            assert c_prev == 0.0
        if last and alpha_one:
            assert (c_x0, c_xt, c_prev) == (1.0, 0.0, 0.0)
        elif last:
            assert (c_prev == 0.0) == (steps < 15)
        if 0 < i < steps - 1:
            h = R.lam(ab[ts[i + 1]]) - R.lam(ab[t])
            h_prev = R.lam(ab[t]) - R.lam(ab[ts[i - 1]])
            assert c_prev == pytest.approx(h / (2.0 * h_prev), rel=1e-12) and c_prev > 0
        x0 = k_x * xk - k_e * m
        d = x0 + c_prev * (x0 - hist) if c_prev != 0.0 else x0
        xk, hist = c_xt * xk + c_x0 * d, x0
        out = sch.step(m, t, x)
        x = out.prev_sample
        assert x.dtype == torch.float32
        assert torch.allclose(xk, x, rtol=1e-6, atol=1e-6), (kind, i)
        assert torch.allclose(hist, out.pred_original_sample, rtol=1e-6, atol=1e-6)
        xk = x.clone()
    no_lower = DPMSolverMultistepScheduler(lower_order_final=False)
    no_lower.set_timesteps(10)
    assert no_lower.coefficients(int(no_lower.timesteps[-1]))[4] != 0.0
    first = DPMSolverMultistepScheduler(solver_order=1)
    first.set_timesteps(10)
    assert all(first.coefficients(int(t))[4] == 0.0 for t in first.timesteps)


# ------------------------------------------------------------------ 4. from_config / refusals
def test_from_config_refusals_and_history_reset(tmp_path):
    S = DPMSolverMultistepScheduler
    for kw, name in ((dict(algorithm_type="dpmsolver"), "algorithm_type"), (dict(algorithm_type="sde-dpmsolver++"), "algorithm_type"),
                     (dict(solver_type="heun"), "solver_type"), (dict(thresholding=True), "thresholding"),
                     (dict(use_karras_sigmas=True), "use_karras_sigmas"), (dict(solver_order=3), "solver_order"),
                     (dict(timestep_spacing="trailing"), "timestep_spacing"), (dict(beta_schedule="squaredcos_cap_v2"), "squaredcos")):
        with pytest.raises(NotImplementedError, match=name):
            S(**kw)
        with pytest.raises(NotImplementedError, match=name):
            S.from_config(kw)
    for kw, name in ((dict(use_lu_lambdas=True), "use_lu_lambdas"), (dict(euler_at_final=True), "euler_at_final"),
                     (dict(use_exponential_sigmas=True), "use_exponential_sigmas"), (dict(lambda_min_clipped=-5.1), "lambda_min_clipped"),
                     (dict(final_sigmas_type="other"), "final_sigmas_type")):
        with pytest.raises(NotImplementedError, match=name):
            S.from_config(kw)
    with pytest.raises(ValueError):
        S(prediction_type="flow")
    with pytest.raises(TypeError, match="no_such_field"):
        S.from_config({}, no_such_field=1)
    # a stock diffusers file with inert keys loads: values that act only behind refused flags, bookkeeping, library defaults
    stock = {"_class_name": "DPMSolverMultistepScheduler", "_diffusers_version": "0.16.0", "algorithm_type": "dpmsolver++",
             "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085, "dynamic_thresholding_ratio": 0.9,
             "lower_order_final": True, "num_train_timesteps": 1000, "prediction_type": "v_prediction", "sample_max_value": 2.5,
             "solver_order": 2, "solver_type": "midpoint", "steps_offset": 1, "thresholding": False, "trained_betas": None,
             "clip_sample": False, "clip_sample_range": 3.0, "use_karras_sigmas": False, "lambda_min_clipped": -math.inf,
             "variance_type": None, "use_lu_lambdas": False, "final_sigmas_type": "zero"}
    path = tmp_path / "scheduler_config.json"
    path.write_text(json.dumps({k: v for k, v in stock.items() if k != "lambda_min_clipped"}))
    for src in (stock, str(path)):
        sch = S.from_config(src, solver_order=1)
        assert sch.config.solver_order == 1 and sch.config.prediction_type == "v_prediction" and sch.config.set_alpha_to_one
        assert sch.config.beta_schedule == "scaled_linear" and abs(float(sch.betas[-1]) - 0.012) < 1e-7
    assert S.from_config(S().config).config.steps_offset == 1          # another scheduler's .config object
    # trained_betas as an ndarray (no ambiguous truth value), and as a list
    tb = np.linspace(1e-4, 0.02, 1000)
    for v in (tb, tb.tolist(), torch.from_numpy(tb)):
        sch = S.from_config({"trained_betas": v})
        assert torch.allclose(sch.betas, S().betas, atol=1e-7)
    with pytest.raises(ValueError, match="trained_betas"):
        S(trained_betas=tb[:10])
    # surface of the other mirrors
    sch = S()
    assert sch.order == 1 and sch.multistep is True and sch.init_noise_sigma == 1.0
    x = torch.randn(3)
    assert sch.scale_model_input(x, 5) is x
    with pytest.raises(ValueError, match="set_timesteps"):
        sch.coefficients(981)
    sch.set_timesteps(20)
    with pytest.raises(ValueError, match="not one of"):
        sch.coefficients(980)
    with pytest.raises(ValueError):
        sch.set_timesteps(1001)
    # set_timesteps resets the history; steps out of order are refused instead of using a stale one
    sch.set_timesteps(20)
    ts = [int(t) for t in sch.timesteps]
    a = sch.step(x, ts[0], x).prev_sample
    b = sch.step(x, ts[1], a).prev_sample
    with pytest.raises(ValueError, match="in order"):
        sch.step(x, ts[3], b)
    sch.set_timesteps(20)
    assert sch._x0_prev is None
    with pytest.raises(ValueError, match="in order"):
        sch.step(x, ts[1], a)
    assert torch.equal(sch.step(x, ts[0], x).prev_sample, a) and torch.equal(sch.step(x, ts[1], a).prev_sample, b)
    assert torch.equal(sch.step(x, ts[0], x).prev_sample, a)           # stepping from the first timestep starts again


# ------------------------------------------------------------------ 5. ABI refusals before any device call
def test_abi_refusals_before_any_device_call():
    """lavie_cfg_multistep_step / lavie_multistep_step check their arguments on the host: in a process that never touched a
    GPU every refusal below returns before a HIP call (the pointers are never dereferenced)."""
    lib = _lib.load()
    ok = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4096 + 8)
    nan, inf = float("nan"), float("inf")

    def refused(rc, text):
        assert rc != 0
        msg = lib.lavie_last_error().decode()
        assert text in msg, msg

    cfg, one = lib.lavie_cfg_multistep_step, lib.lavie_multistep_step
    good = (7.5, 1.0, 0.5, 0.3, 0.7, 0.5, 1.0)
    for i in range(4):
        ptrs = [ok] * 4
        ptrs[i] = None
        refused(cfg(*ptrs, 64, *good, None), "null argument")
        refused(one(*ptrs, 64, *good[1:], None), "null argument")
        ptrs[i] = odd
        refused(cfg(*ptrs, 64, *good, None), "not 16-byte aligned")
        refused(one(*ptrs, 64, *good[1:], None), "not 16-byte aligned")
    for n in (0, -1):
        refused(cfg(ok, ok, ok, ok, n, *good, None), "must be >= 1")
        refused(one(ok, ok, ok, ok, n, *good[1:], None), "must be >= 1")
    for i in range(7):
        for bad in (nan, inf, -inf):
            s = list(good)
            s[i] = bad
            refused(cfg(ok, ok, ok, ok, 64, *s, None), "not finite")
            if i:
                refused(one(ok, ok, ok, ok, 64, *s[1:], None), "not finite")
    assert lib.lavie_abi_version() == 8                                  # additive: the ABI version did not move


def test_ops_refuse_host_tensors_and_wrong_sizes():
    from lavie_amd import ops
    x = torch.zeros(16)
    with pytest.raises(ValueError):
        ops.cfg_multistep_step(torch.zeros(32, dtype=torch.float16), x, x.clone(), torch.zeros(32, dtype=torch.float16), 7.5,
                               (1, 1, 1, 0, 0))
    with pytest.raises(ValueError):
        ops.multistep_step(torch.zeros(16, dtype=torch.float16), x, x.clone(), torch.zeros(16, dtype=torch.float16), (1, 1, 1, 0, 0))


# ------------------------------------------------------------------ 6. sanitizer host build
def test_make_asan_covers_the_new_entries():
    """`make asan` (host-only AddressSanitizer + UBSan build against the HIP stub) passes with the multistep cases in
    hostcheck/driver.cpp."""
    src = open(os.path.join(ROOT, "lavie_amd", "csrc", "hostcheck", "driver.cpp")).read()
    assert "lavie_cfg_multistep_step" in src and "lavie_multistep_step(" in src
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lavie_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1)), "asan"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hostcheck: ok" in r.stdout


# ------------------------------------------------------------------ 7. pipeline dispatch (no GPU)
class _StubUNet:
    class config:
        in_channels, sample_size = 4, 8
    device = torch.device("cpu")

    def prepare(self, *a):
        pass

    def __call__(self, model_in, t, encoder_hidden_states=None):
        return types.SimpleNamespace(sample=torch.zeros_like(model_in))


def _dispatch(monkeypatch, scheduler, guidance):
    from lavie_amd import pipeline_videogen as P
    calls = []
    rec = lambda name: (lambda *a, **k: calls.append((name, a)))
    for name in ("latents_to_model_input", "latents_to_model_input1", "cfg_ddpm_step", "sampler_step", "cfg_multistep_step",
                 "multistep_step"):
        monkeypatch.setattr(P.ops, name, rec(name))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: None)
    pipe = P.VideoGenPipeline(unet=_StubUNet(), scheduler=scheduler)
    pe = torch.zeros(1, 77, 16)
    pipe(prompt_embeds=pe, negative_prompt_embeds=pe, video_length=2, height=64, width=64, num_inference_steps=5,
         guidance_scale=guidance, output_type="latent")
    return calls


def test_pipeline_dispatches_on_the_multistep_marker(monkeypatch):
    """VideoGenPipeline runs the multistep op for a scheduler that declares `multistep = True` and the five-coefficient op
    for DDPM / DDIM / Euler, with and without guidance; the history buffer is one fp32 tensor beside the latents for the
    whole call.  Dispatch only: the ops are recorded, no kernel runs."""
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.scheduling_ddpm import DDPMScheduler
    from lavie_amd.scheduling_euler_discrete import EulerDiscreteScheduler
    for guidance, new, old in ((7.5, "cfg_multistep_step", "cfg_ddpm_step"), (1.0, "multistep_step", "sampler_step")):
        calls = _dispatch(monkeypatch, DPMSolverMultistepScheduler(), guidance)
        steps = [c for c in calls if "step" in c[0]]
        assert [c[0] for c in steps] == [new] * 5
        x, hist = steps[0][1][1], steps[0][1][2]
        assert hist.dtype == torch.float32 and hist.shape == x.shape and hist.data_ptr() != x.data_ptr()
        assert all(c[1][2] is hist for c in steps)                       # allocated once per call
        coeffs = [c[1][5] if guidance > 1 else c[1][4] for c in steps]
        assert coeffs[0][4] == 0.0 and coeffs[-1][4] == 0.0 and all(c[4] > 0 for c in coeffs[1:-1])
        for sch in (DDPMScheduler(), DDIMScheduler(), EulerDiscreteScheduler()):
            names = [c[0] for c in _dispatch(monkeypatch, sch, guidance) if "step" in c[0]]
            assert names == [old] * 5, type(sch).__name__
    # sample_method: the new name builds the new scheduler from the same keys, the old names and the refusal are unchanged
    cfg = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_sampling_steps=20)
    pipe, kw, _ = VideoGenPipeline.from_sample_yaml(dict(cfg, sample_method="dpmsolver++"), unet=_StubUNet())
    assert isinstance(pipe.scheduler, DPMSolverMultistepScheduler) and pipe.scheduler.config.beta_schedule == "scaled_linear"
    assert abs(float(pipe.scheduler.betas[0]) - 0.00085) < 1e-8 and kw["num_inference_steps"] == 20
    for method, cls in (("ddpm", DDPMScheduler), ("ddim", DDIMScheduler), ("eulerdiscrete", EulerDiscreteScheduler)):
        assert type(VideoGenPipeline.from_sample_yaml(dict(cfg, sample_method=method), unet=_StubUNet())[0].scheduler) is cls
    with pytest.raises(NotImplementedError, match="unipc"):
        VideoGenPipeline.from_sample_yaml(dict(cfg, sample_method="unipc"), unet=_StubUNet())


def test_cascade_takes_stage_schedulers():
    """text_to_video_cascade(base_scheduler=, vsr_scheduler=) installs them for the call and restores the pipelines' own."""
    import inspect
    from lavie_amd import cascade
    sig = inspect.signature(cascade.text_to_video_cascade).parameters
    assert sig["base_scheduler"].default is None and sig["vsr_scheduler"].default is None
    own_b, own_v, new_b, new_v = object(), object(), DPMSolverMultistepScheduler(), DPMSolverMultistepScheduler()
    seen = {}

    class Base:
        scheduler, device = own_b, torch.device("cpu")

        def __call__(self, **kw):
            seen["base"] = self.scheduler
            raise RuntimeError("stop after the base stage")

    base, vsr = Base(), types.SimpleNamespace(scheduler=own_v)
    with pytest.raises(RuntimeError, match="stop after"):
        cascade.text_to_video_cascade(base, None, None, vsr, None, None, None, None, None, None, None, None,
                                      base_scheduler=new_b, vsr_scheduler=new_v)
    assert seen["base"] is new_b and base.scheduler is own_b and vsr.scheduler is own_v
