"""FreeInit on the host: the filter of lavie_amd/free_init.py against the published filter of
tests/freeinit_reference.py pushed through "even part, un-shift"; the one-transform form with that filter against the literal
two-transform formula; the step counts; argument validation and the refused combinations; the launch sequence of the iterations
with recording stand-ins for the device ops; yaml and cascade plumbing; the header and the bindings."""
import contextlib
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import freeinit_cases as C
import freeinit_reference as R
from lavie_amd import _lib, cascade, free_init, ops, sampling
from lavie_amd.free_init import FreeInit, freq_filter
from lavie_amd.pipeline_videogen import VideoGenPipeline
from lavie_amd.scheduling_ddim import DDIMScheduler
from lavie_amd.scheduling_ddpm import DDPMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the filter
@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("shape", C.FILTER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_filter_is_the_even_part_of_the_published_filter(shape, method):
    """Both sides work in float64 and round to fp32 once: they may differ by the rounding of a value that the two float64 paths place
    on either side of a tie, one unit roundoff of fp32 at 1 (the filter lies in [0, 1])."""
    for ds, dt in C.FILTER_STOPS:
        got = freq_filter(*shape, method, C.ORDER, ds, dt)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        want = R.even_part_native(R.published_filter(*shape, method, C.ORDER, ds, dt))
        assert float((got.double() - want).abs().max()) <= 2.0 ** -23, (shape, method, ds, dt)
        if ds == 0 or dt == 0:
            assert not got.any()
            continue
        neg = [(-torch.arange(n)) % n for n in shape]
        assert torch.equal(got[neg[0]][:, neg[1]][:, :, neg[2]], got)                   # even in frequency
        assert 0.0 <= float(got.min()) and float(got.max()) <= 1.0
        if all(n % 2 == 0 for n in shape):          # (an odd axis puts frequency 0 at 2 t / N - 1 = -1 / N, not 0: the published filter)
            assert float(got[0, 0, 0]) == 1.0
        # even lengths: the published filter is even already, up to the rounding of 2 t / N - 1 at mirrored indices (which may put a
        # boundary point of the ideal filter on either side of its threshold: the smooth filters show it)
        if all(n % 2 == 0 for n in shape) and method != "ideal":
            plain = torch.fft.ifftshift(R.published_filter(*shape, method, C.ORDER, ds, dt))
            assert float((got.double() - plain).abs().max()) <= 2.0 ** -23


@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("shape", [(5, 6, 8), (61, 10, 12), (8, 6, 4)], ids=lambda s: "x".join(map(str, s)))
def test_one_transform_with_the_even_part_is_the_published_formula(shape, method):
    """float64: r z + IFFT3(even .* FFT3(z_T - r z)) has no imaginary part and equals the real part of the literal formula, also where
    the literal result has an imaginary part to drop (odd lengths)."""
    x0, e0, z = (t.double() for t in C.op_inputs((2,) + shape))
    a, s = C.noise_level()
    lpf = R.published_filter(*shape, method, C.ORDER, C.DS, C.DT)
    literal = R.mix(x0, e0, z, a, s, 1.7, lpf)
    even = R.even_part_native(lpf)
    one = torch.fft.ifftn(even * torch.fft.fftn(a * x0 + s * e0 - 1.7 * z, dim=R.DIMS), dim=R.DIMS)
    assert float(one.imag.abs().max()) < 1e-13
    assert float((1.7 * z + one.real - literal.real).abs().max()) < 1e-13
    if any(n % 2 for n in shape):
        assert float(literal.imag.abs().max()) > 1e-3
    else:
        assert float(literal.imag.abs().max()) < 1e-13


# ------------------------------------------------------------------ the setting
def test_steps_at_is_the_formula():
    for iters in (1, 2, 3, 5):
        for n in (1, 2, 3, 7, 25, 50):
            fast, slow = FreeInit(num_iters=iters, use_fast_sampling=True), FreeInit(num_iters=iters)
            for i in range(iters):
                assert fast.steps_at(i, n) == max(1, int(n / iters * (i + 1)))
                assert slow.steps_at(i, n) == n
    assert [FreeInit(3, True).steps_at(i, 25) for i in range(3)] == [8, 16, 25]
    with pytest.raises(ValueError, match="iteration"):
        FreeInit(3).steps_at(3, 10)


def test_defaults_and_validation():
    d = FreeInit()
    assert (d.num_iters, d.use_fast_sampling, d.method, d.order, d.spatial_stop_frequency, d.temporal_stop_frequency) == \
        (3, False, "butterworth", 4, 0.25, 0.25)
    for bad, text in ((dict(num_iters=0), "num_iters"), (dict(num_iters=2.5), "num_iters"), (dict(num_iters=True), "num_iters"),
                      (dict(method="box"), "method"), (dict(order=0), "order"), (dict(order=1.5), "order"),
                      (dict(spatial_stop_frequency=-0.1), "spatial_stop_frequency"),
                      (dict(temporal_stop_frequency=float("nan")), "temporal_stop_frequency")):
        with pytest.raises(ValueError, match=text):
            FreeInit(**bad)
    with pytest.raises(ValueError, match="method"):
        freq_filter(4, 4, 4, "box")
    assert free_init.coerce(None) is None and free_init.coerce(FreeInit(num_iters=1)) is None and free_init.coerce(dict(num_iters=1)) is None
    assert free_init.coerce(dict(num_iters=2, method="ideal")).method == "ideal"
    with pytest.raises(TypeError):
        free_init.coerce(dict(iterations=2))


def stub_unet():
    def forward(x, t, encoder_hidden_states=None, **kw):
        forward.calls.append((tuple(x.shape), float(t), kw))
        return SimpleNamespace(sample=torch.zeros_like(x))
    forward.calls = []
    forward.config = SimpleNamespace(sample_size=8, in_channels=4)
    forward.device = "cpu"
    forward.prepare = lambda *a: None
    return forward


def test_refused_combinations_raise_before_the_engine():
    unet = stub_unet()
    pipe = VideoGenPipeline(unet=unet, scheduler=DDIMScheduler())
    shape = (1, 4, 4, 4, 6)
    lat, ctx = torch.zeros(shape), torch.zeros(2, 77, 8)
    for kw in (dict(known=lat), dict(known=lat, mask=torch.ones(1, 1, 4, 4, 6)), dict(known=lat, start_step=1), dict(known_noise=lat), dict(start_step=1)):
        with pytest.raises(ValueError, match="FreeInit.*known latents"):
            pipe.denoise(lat, ctx, 4, 7.5, free_init=dict(num_iters=2), **kw)
    emb = dict(prompt_embeds=torch.zeros(1, 77, 8), negative_prompt_embeds=torch.zeros(1, 77, 8), height=32, width=48, video_length=4,
               num_inference_steps=2, output_type="latent")
    for kw in (dict(known_latents=lat), dict(known_latents=lat, known_mask=torch.ones(1, 1, 4, 4, 6)), dict(video=torch.zeros(1, 4, 32, 48, 3, dtype=torch.uint8)),
               dict(strength=0.5)):
        with pytest.raises(ValueError, match="FreeInit.*cannot be combined"):
            pipe(free_init=FreeInit(num_iters=2), **emb, **kw)
    pipe.enable_free_init(num_iters=2)                    # the setting on the pipeline is refused the same way
    with pytest.raises(ValueError, match="FreeInit.*cannot be combined"):
        pipe(**emb, known_latents=lat)
    with pytest.raises(ValueError, match="FreeInit.*known latents"):
        pipe.denoise(lat, ctx, 4, 7.5, known=lat)
    with pytest.raises(ValueError, match="FreeInit"):
        cascade.continue_clip(pipe, torch.zeros(1, 4, 8, 4, 6), overlap=2, **{k: v for k, v in emb.items() if k not in ("video_length", "output_type")})
    with pytest.raises(ValueError, match="chain"):
        cascade.text_to_long_video(pipe, None, 2, overlap=2, **{k: v for k, v in emb.items() if k not in ("video_length", "output_type")})
    pipe.disable_free_init()
    assert pipe.free_init is None
    with pytest.raises(ValueError, match="num_iters"):
        pipe.enable_free_init(num_iters=0)
    assert unet.calls == []


# ------------------------------------------------------------------ the iterations, launch for launch
def record_loop(monkeypatch, scheduler, free, steps=3, frames=4, generator=None, **kw):
    """pipe.denoise on CPU tensors with recording stand-ins for the device ops -> the list of events."""
    events = []
    unet = stub_unet()
    pipe = VideoGenPipeline(unet=unet, scheduler=scheduler)

    def fill(name):
        def f(x, m, scale=1.0):
            events.append((name, tuple(x.shape), tuple(m.shape), round(float(scale), 6)))
        return f

    def step(eps, x, aux, model_in, guidance, coeffs, next_scale, multistep, region=None):
        events.append(("step", aux is not None, tuple(round(float(c), 9) for c in coeffs), multistep))

    def window_step(eps, x, aux, model_in, starts, profile, guidance, coeffs, next_scale, multistep):
        events.append(("window_step", len(eps), list(starts)))

    def freq_mix(x0, e0, z, filt, a, s, r, out=None, model_in=None, input_scale=1.0, workspace=None):
        assert out is x0 and tuple(filt.shape) == tuple(x0.shape[2:]) and tuple(e0.shape) == tuple(z.shape) == tuple(x0.shape)
        assert workspace.numel() * 4 >= ops.freq_mix_workspace_bytes(x0.shape[0] * x0.shape[1], *x0.shape[2:])
        events.append(("freq_mix", None if model_in is None else tuple(model_in.shape), round(float(a), 9), round(float(s), 9), float(r),
                       float(z.sum()), float(e0.sum())))

    monkeypatch.setattr(ops, "latents_to_model_input", fill("fill2"))
    monkeypatch.setattr(ops, "latents_to_model_input1", fill("fill1"))
    monkeypatch.setattr(ops, "freq_mix", freq_mix)
    monkeypatch.setattr(sampling, "step", step)
    monkeypatch.setattr(sampling, "window_step", window_step)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(1, 4, frames, 4, 6, generator=g)
    seen = []
    pipe.denoise(lat, torch.zeros(2, 77, 8), steps, 7.5, generator=generator, callback=lambda i, t, x: seen.append((i, t)),
                 **({"free_init": free} if free is not None else {}), **kw)
    return events, unet.calls, seen, lat


def test_one_iteration_is_the_call_without_it(monkeypatch):
    plain = record_loop(monkeypatch, DDPMScheduler(), None, generator=torch.Generator().manual_seed(1))
    one = record_loop(monkeypatch, DDPMScheduler(), dict(num_iters=1, use_fast_sampling=True), generator=torch.Generator().manual_seed(1))
    assert one[:3] == plain[:3] and not any(e[0] == "freq_mix" for e in one[0])


def test_iterations_launch_sequence(monkeypatch):
    sch = DDPMScheduler()
    gen = torch.Generator().manual_seed(1)
    events, calls, seen, lat = record_loop(monkeypatch, sch, dict(num_iters=3), generator=gen)
    kinds = [e[0] for e in events]
    assert kinds == ["fill2"] + ["step"] * 3 + ["freq_mix"] + ["step"] * 3 + ["freq_mix"] + ["step"] * 3      # no fill between iterations
    assert len(calls) == 9 and [i for i, _ in seen] == [0, 1, 2] * 3
    a, s = sch.noise_level(sch.config.num_train_timesteps - 1)
    mixes = [e for e in events if e[0] == "freq_mix"]
    assert all(m[1] == (2, 4, 4, 4, 6) and m[2:5] == (round(a, 9), round(s, 9), 1.0) for m in mixes)        # both guidance halves, r = 1
    assert all(abs(m[6] - float(lat.sum())) < 1e-4 for m in mixes)                 # e0: the latents the call started from, kept
    assert mixes[0][5] != mixes[1][5]                                              # a fresh draw each time
    # the draws come from `generator` in the order: step noise of iteration 0, z, step noise of iteration 1, z, ...
    ref = torch.Generator().manual_seed(1)
    shape = tuple(lat.shape)
    for m in mixes:
        for _ in range(2):                      # DDPM: every step but the last draws
            torch.empty(shape).normal_(generator=ref)
        assert float(torch.randn(shape, generator=ref).sum()) == m[5]
    # every iteration's steps are the plain run's steps (multistep history and layer cache restart at position 0)
    steps = [e for e in events if e[0] == "step"]
    assert steps[:3] == steps[3:6] == steps[6:]


def test_fast_sampling_windows_cache_and_multistep(monkeypatch):
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    events, calls, seen, _ = record_loop(monkeypatch, DPMSolverMultistepScheduler(), dict(num_iters=3, use_fast_sampling=True), steps=6)
    assert [e[0] for e in events] == ["fill2"] + ["step"] * 2 + ["freq_mix"] + ["step"] * 4 + ["freq_mix"] + ["step"] * 6
    assert [i for i, _ in seen] == [0, 1, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5]
    firsts = [e for e, (i, _) in zip([e for e in events if e[0] == "step"], seen) if i == 0]
    assert all(e[2][4] == 0.0 for e in firsts)                       # c_prev = 0: no history read at an iteration's first step
    # frame windows: the mix spans the whole clip and writes no model input; every window's input is cut from the mixed clip
    events, calls, _, _ = record_loop(monkeypatch, DDIMScheduler(), dict(num_iters=2), steps=2, frames=6, window_length=4, window_stride=2)
    assert [e[0] for e in events] == ["fill2", "fill2", "window_step", "window_step", "freq_mix", "fill2", "fill2", "window_step", "window_step"]
    assert [e for e in events if e[0] == "freq_mix"][0][1] is None
    assert all(c[0] == (2, 4, 4, 4, 6) for c in calls)


def test_layer_cache_refreshes_at_every_iteration(monkeypatch):
    monkeypatch.setattr(sampling, "layer_cache_session", lambda unet, interval, depth=1: contextlib.nullcontext())
    _, calls, _, _ = record_loop(monkeypatch, DDIMScheduler(), dict(num_iters=2), steps=3, cache_interval=2)
    assert [c[2].get("layer_cache") for c in calls] == ["refresh", "reuse", "refresh"] * 2


# ------------------------------------------------------------------ yaml and cascade
def test_yaml_key_and_cascade_keyword():
    unet = stub_unet()
    pipe, kw, _ = VideoGenPipeline.from_sample_yaml({"sample_method": "ddim", "free_init": {"num_iters": 2, "use_fast_sampling": True,
                                                    "method": "gaussian", "order": 2, "spatial_stop_frequency": 0.5,
                                                    "temporal_stop_frequency": 0.125}}, unet)
    f = pipe.free_init
    assert (f.num_iters, f.use_fast_sampling, f.method, f.order, f.spatial_stop_frequency, f.temporal_stop_frequency) == \
        (2, True, "gaussian", 2, 0.5, 0.125)
    assert "free_init" not in kw
    pipe, _, _ = VideoGenPipeline.from_sample_yaml({"free_init": {"num_iters": 4}}, unet)
    assert pipe.free_init.num_iters == 4 and pipe.free_init.method == "butterworth"
    pipe, _, _ = VideoGenPipeline.from_sample_yaml({}, unet)
    assert pipe.free_init is None
    with pytest.raises(ValueError, match="method"):
        VideoGenPipeline.from_sample_yaml({"free_init": {"method": "box"}}, unet)

    class Pipe:
        unet, scheduler, device, free_init = None, None, "cpu", None

        def __init__(self):
            self.calls = []

        def __call__(self, **kw):
            self.calls.append(kw)
            raise KeyError("stop after the first call")

    setting = FreeInit(num_iters=2)
    for extra, want in ((dict(base_free_init=setting), {"free_init": setting}), ({}, {})):
        base_pipe = Pipe()
        with pytest.raises(KeyError):
            cascade.text_to_video_cascade(base_pipe, None, None, Pipe(), *([None] * 8), **extra)
        assert {k: v for k, v in base_pipe.calls[0].items() if k == "free_init"} == want
    # long clips: forwarded to the one run over windows and to a chain of one clip; refused where an overlap is pinned
    for method, clips in (("windows", 3), ("chain", 1)):
        p = Pipe()
        with pytest.raises(KeyError):
            cascade.text_to_long_video(p, "a prompt", clips, overlap=4, method=method, free_init=setting)
        assert p.calls[0]["free_init"] is setting
    p = Pipe()
    with pytest.raises(ValueError, match="chain"):
        cascade.text_to_long_video(p, "a prompt", 2, overlap=4, method="chain", free_init=setting)
    assert p.calls == []
    cascade_ok = Pipe()
    with pytest.raises(KeyError):                       # num_iters = 1 is off: the chain runs
        cascade.text_to_long_video(cascade_ok, "a prompt", 2, overlap=4, method="chain", free_init=dict(num_iters=1))


# ------------------------------------------------------------------ the C interface
def test_header_keeps_abi_8_and_declares_the_entries():
    header = open(os.path.join(ROOT, "include", "lavie_hip.h")).read()
    assert re.search(r"#define LAVIE_ABI_VERSION 8\b", header)
    lib = _lib.load()
    assert lib.lavie_abi_version() == 8 == _lib.ABI_VERSION
    for name in ("lavie_freq_mix_workspace_bytes", "lavie_freq_mix_f32"):
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"typedef struct lavie_freq_mix_args \{\s*int struct_size;", header)
    assert lib.lavie_freq_mix_workspace_bytes.restype is ctypes.c_longlong
    assert lib.lavie_freq_mix_workspace_bytes(4, 16, 40, 64) == 2 * 8 * 4 * 16 * 40 * 64
    for bad in ((0, 16, 40, 64), (4, 0, 40, 64), (4, 257, 40, 64), (4, 16, 129, 64), (4, 16, 40, 129), (4, 16, 40, 0)):
        assert lib.lavie_freq_mix_workspace_bytes(*bad) == 0, bad
    assert lib.lavie_freq_mix_workspace_bytes(1, 256, 128, 128) == 2 * 8 * 256 * 128 * 128
    # refusals need no device: nothing is dereferenced or launched
    assert lib.lavie_freq_mix_f32(None, None) != 0 and b"args is null" in lib.lavie_last_error()
    a = _lib.FreqMixArgsC()
    a.struct_size = ctypes.sizeof(_lib.FreqMixArgsC) - 4
    assert lib.lavie_freq_mix_f32(ctypes.byref(a), None) != 0 and b"struct_size" in lib.lavie_last_error()
    a.struct_size = ctypes.sizeof(_lib.FreqMixArgsC)
    a.images, a.F, a.H, a.W = 1, 300, 4, 4
    assert lib.lavie_freq_mix_f32(ctypes.byref(a), None) != 0 and b"F=300" in lib.lavie_last_error()
    a.F = 4
    assert lib.lavie_freq_mix_f32(ctypes.byref(a), None) != 0 and b"x0 is null" in lib.lavie_last_error()
    with pytest.raises(ValueError):
        ops.freq_mix(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4), torch.zeros(4, 4, 4), 1.0, 0.0, 1.0)   # CPU tensors
