"""lavie_amd.sampling, everything that needs no GPU: the step plan against the schedulers' own calls, the dispatch among the
eight step ops with recorded stubs, the engine session's clean-up with a recording stub UNet, and the step noise on CPU
tensors against randn_tensor."""
from types import SimpleNamespace

import pytest
import torch

from lavie_amd import sampling
from lavie_amd.scheduling_ddim import DDIMScheduler
from lavie_amd.scheduling_ddpm import DDPMScheduler, randn_tensor
from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
from lavie_amd.scheduling_euler_discrete import EulerDiscreteScheduler


# ------------------------------------------------------------------ 1. the step plan
@pytest.mark.parametrize("make,eta", [(DDPMScheduler, 0.0), (DDIMScheduler, 0.0), (DDIMScheduler, 0.5), (EulerDiscreteScheduler, 0.0),
                                      (DPMSolverMultistepScheduler, 0.0)])
def test_step_plan_is_the_schedulers_own_calls(make, eta):
    plan = sampling.StepPlan(make(), 5, eta)
    own = make()
    own.set_timesteps(5)
    kind = float if make is EulerDiscreteScheduler else int
    assert len(plan.timesteps) == 5 and all(type(t) is kind for t in plan.timesteps)
    assert plan.timesteps == [kind(t) for t in own.timesteps]
    assert plan.multistep is (make is DPMSolverMultistepScheduler)
    t_dev = plan.t_dev("cpu")
    assert t_dev.dtype == torch.float32 and t_dev.tolist() == [float(torch.tensor(t, dtype=torch.float32)) for t in plan.timesteps]
    for i, t in enumerate(plan.timesteps):
        want = own.coefficients(t, eta) if make is DDIMScheduler else own.coefficients(t)
        assert plan.coeffs(i) == want
        assert plan.adds_noise(want) == (not plan.multistep and want[4] != 0.0)
        assert plan.input_scale(i) == (own.model_input_scale(t) if hasattr(own, "model_input_scale") else 1.0)
        assert plan.noise_level(i) == own.noise_level(t)
        # a run that starts at step i has no x0 history: a multistep step is first order there, any other is untouched
        assert plan.coeffs(i, first=True) == (tuple(want[:4]) + (0.0,) if plan.multistep else want)
    assert plan.input_scale(5) == 1.0 and plan.noise_level(5) == (1.0, 0.0)
    if make is EulerDiscreteScheduler:
        assert plan.input_scale(0) != 1.0                             # the scale is really the scheduler's
    if make is DDIMScheduler:
        assert (plan.coeffs(1)[4] != 0.0) == (eta != 0.0)             # eta reached the scheduler
    if make is DPMSolverMultistepScheduler:
        assert plan.coeffs(2)[4] > 0.0 and not plan.adds_noise(plan.coeffs(2))


# ------------------------------------------------------------------ 2. the dispatch
NAMES = ("cfg_ddpm_step", "sampler_step", "cfg_multistep_step", "multistep_step", "cfg_sampler_step_known", "sampler_step_known",
         "cfg_multistep_step_known", "multistep_step_known")


@pytest.mark.parametrize("guided,multistep,pinned,name", [
    (True, False, False, "cfg_ddpm_step"), (False, False, False, "sampler_step"),
    (True, True, False, "cfg_multistep_step"), (False, True, False, "multistep_step"),
    (True, False, True, "cfg_sampler_step_known"), (False, False, True, "sampler_step_known"),
    (True, True, True, "cfg_multistep_step_known"), (False, True, True, "multistep_step_known")])
def test_step_reaches_the_op_of_its_family_with_its_positional_arguments(monkeypatch, guided, multistep, pinned, name):
    calls = []
    for n in NAMES:
        monkeypatch.setattr(sampling.ops, n, (lambda n: lambda *a, **k: calls.append((n, a, k)))(n))
    eps, x, aux, model_in, coeffs = object(), object(), object(), object(), (1.0, 2.0, 3.0, 4.0, 5.0)
    region = (object(), object(), object(), (0.5, 0.25)) if pinned else None
    sampling.step(eps, x, aux, model_in, 7.5 if guided else None, coeffs, 0.75, multistep, region)
    want = (eps, x, aux, model_in) + ((7.5,) if guided else ()) + (coeffs, 0.75) + (region or ())
    assert calls == [(name, want, {})]


# ------------------------------------------------------------------ 3. the engine session
class RecordingUNet:
    def __init__(self, fail=()):
        self.log, self.fail = [], set(fail)

    def _call(self, name, *a):
        self.log.append((name,) + a)
        if name in self.fail:
            raise RuntimeError(f"{name} failed")

    def prepare(self, *a):
        self._call("prepare", *a)

    def cache_context(self, ctx):
        self._call("cache" if ctx is not None else "uncache")
        return "cached" if ctx is not None else None

    def set_cfg_shared_input(self, on):
        self._call("share" if on else "unshare")


def test_session_undoes_shared_input_then_the_cached_context():
    unet, ctx = RecordingUNet(), torch.zeros(2, 77, 8)
    with sampling.engine_session(unet, 2, 3, 4, 6, ctx, shared_inputs=[torch.zeros(2, 1)]) as got:
        assert got == "cached" and unet.log == [("prepare", 2, 3, 4, 6, 77), ("cache",), ("share",)]
    assert unet.log[3:] == [("unshare",), ("uncache",)]
    unet = RecordingUNet()
    with sampling.engine_session(unet, 2, 3, 4, 6, ctx):                # no shared inputs: the switch is never touched
        pass
    assert [e[0] for e in unet.log] == ["prepare", "cache", "uncache"]


def test_session_never_masks_the_loops_exception():
    ctx = torch.zeros(2, 77, 8)
    for fail in ((), ("unshare",), ("unshare", "uncache")):
        unet, boom = RecordingUNet(fail), KeyError("the loop's own")
        with pytest.raises(KeyError) as info:
            with sampling.engine_session(unet, 2, 3, 4, 6, ctx, shared_inputs=[]):
                raise boom
        assert info.value is boom and [e[0] for e in unet.log[3:]] == ["unshare", "uncache"]
    # an undo that raises is re-raised only when the body succeeded: the first failure, after every undo has been attempted
    for fail, text in ((("unshare",), "unshare failed"), (("uncache",), "uncache failed"), (("unshare", "uncache"), "unshare failed")):
        unet = RecordingUNet(fail)
        with pytest.raises(RuntimeError, match=text):
            with sampling.engine_session(unet, 2, 3, 4, 6, ctx, shared_inputs=[]):
                pass
        assert [e[0] for e in unet.log[3:]] == ["unshare", "uncache"]
    # set_cfg_shared_input(True) failing counts as the body: both undos run, its exception propagates
    unet = RecordingUNet(("share",))
    with pytest.raises(RuntimeError, match="share failed"):
        with sampling.engine_session(unet, 2, 3, 4, 6, ctx, shared_inputs=[]):
            raise AssertionError("the body must not run")
    assert [e[0] for e in unet.log] == ["prepare", "cache", "share", "unshare", "uncache"]


def test_session_debug_check_covers_every_model_input(monkeypatch):
    monkeypatch.setenv("LAVIE_DEBUG_CHECK_SHARED", "1")
    same, differ = torch.ones(4, 3), torch.arange(12.0).reshape(4, 3)
    with sampling.engine_session(RecordingUNet(), 4, 3, 4, 6, torch.zeros(4, 77, 8), shared_inputs=[same, same.clone()]):
        pass
    unet = RecordingUNet()
    with pytest.raises(RuntimeError, match="two halves"):
        with sampling.engine_session(unet, 4, 3, 4, 6, torch.zeros(4, 77, 8), shared_inputs=[same, differ]):
            raise AssertionError("the body must not run")
    assert [e[0] for e in unet.log[3:]] == ["unshare", "uncache"]


def test_session_takes_a_unet_without_the_optional_methods():
    class Bare:
        prepared = None

        def prepare(self, *a):
            self.prepared = a

    unet, ctx = Bare(), torch.zeros(2, 5, 8)
    with sampling.engine_session(unet, 2, 3, 4, 6, ctx, shared_inputs=[torch.zeros(2, 1)]) as got:
        assert got is ctx and unet.prepared == (2, 3, 4, 6, 5)
    with pytest.raises(KeyError):
        with sampling.engine_session(unet, 2, 3, 4, 6, ctx):
            raise KeyError("propagates")


# ------------------------------------------------------------------ 4. the step noise on CPU tensors
SHAPE = (2, 4, 3, 4, 6)


def seeded(seeds):
    return [torch.Generator().manual_seed(s) for s in seeds]


@pytest.mark.parametrize("seeds", [(5,), (5, 9)])
def test_cpu_draws_are_randn_tensors(monkeypatch, seeds):
    """Three consecutive draws from a CPU generator (or a list of two) are randn_tensor's, bit for bit; no CUDA stream is
    touched for a CPU tensor."""
    def no_cuda(*a, **k):
        raise AssertionError("CUDA streams touched for a CPU tensor")
    for name in ("Stream", "Event", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    as_arg = lambda gens: gens[0] if len(gens) == 1 else gens         # noqa: E731
    noise, ref = sampling.StepNoise(torch.zeros(SHAPE), as_arg(seeded(seeds))), as_arg(seeded(seeds))
    for _ in range(3):
        got = noise.draw()
        noise.done()
        assert got.dtype == torch.float32 and torch.equal(got, randn_tensor(SHAPE, ref))
    none = sampling.StepNoise(torch.zeros(SHAPE)).draw()               # no generator: the default one
    assert none.shape == SHAPE and none.std() > 0.5


def test_generator_lists_are_refused_with_their_messages():
    x = torch.zeros(SHAPE)
    with pytest.raises(ValueError, match="got a list of 3 generators for 2 latents"):
        sampling.StepNoise(x, seeded((1, 2, 3)))
    on_device = SimpleNamespace(device=torch.device("cuda"))          # only its device is looked at before the refusal
    with pytest.raises(ValueError, match="a list of generators must live on one device type"):
        sampling.StepNoise(x, [torch.Generator(), on_device])


def test_window_forwards_keep_every_prediction_alive():
    """A forward that hands back one buffer is seen at the second window of the first step: predictions are cloned from then on
    and the overwritten first one is redone; a forward with fresh outputs is never cloned or repeated."""
    buf, calls = torch.zeros(3), []

    def reusing(w, i):
        calls.append(w)
        return buf.fill_(10 * i + w)

    forwards = sampling.WindowForwards(reusing)
    assert [e.tolist()[0] for e in forwards(3, 0)] == [0.0, 1.0, 2.0] and calls == [0, 1, 0, 2]
    del calls[:]
    assert [e.tolist()[0] for e in forwards(3, 1)] == [10.0, 11.0, 12.0] and calls == [0, 1, 2]
    del calls[:]
    outs = []

    def fresh(w, i):
        calls.append(w)
        outs.append(torch.full((3,), float(w)))
        return outs[-1]

    forwards = sampling.WindowForwards(fresh)
    got = forwards(2, 0) + forwards(2, 1)
    assert calls == [0, 1, 0, 1] and all(a is b for a, b in zip(got, outs))
    assert sampling.WindowForwards(fresh)(1, 0)[0] is outs[-1]        # one window: nothing to decide
