"""Guidance from a per-latent table, everything that needs no GPU: the launch rule of the case shapes, the checks of
guidance_reference.py against injected defects on the float64 / fp32 model, the host logic of the pipelines with a recording `ops`,
and the refusals.  Except for the default-path recording test, which pins today's call sequences and passes with or without the
feature, every test here needs the new keywords, wrappers or entry points: the injected-defect tests too, whose model takes the
chunking of its partial sums from the library's own size query (`ops.guidance_partials_floats`), so that the model the defects are
placed on is the layout the kernels write."""
from types import SimpleNamespace

import pytest
import torch

import guidance_cases as C
import guidance_reference as R
import opcheck as oc
from gpu_util import TOL_OP
from lavie_amd import ops, sampling


def test_case_shapes_reach_the_paths_they_are_there_for():
    rule = {n: R.launch_rule(C.SHAPES[n][0], C.per_of(n)) for n in C.SHAPES}
    assert [C.SHAPES[n][0] * 0 + C.per_of(n) for n in C.SHAPES] == [420, R.CH + 8, 3 * R.CH, 8, 655360]
    assert not rule["3x420"]["vector"] and rule["3x420"]["step_grid"] == (2, 3) and 420 % 256 != 0      # scalar route, ragged block
    assert rule["2x(CH+8)"]["vector"] and rule["2x(CH+8)"]["chunks"] == 2 and rule["2x(CH+8)"]["last_chunk"] == 8
    assert rule["2x3CH"]["chunks"] == 3 and rule["2x3CH"]["last_chunk"] == R.CH
    assert rule["1x8"]["vector"] and rule["1x8"]["moments_grid"] == (1, 1) and 8 // 8 < 256              # one vector, one lane
    assert rule["base"]["chunks"] == 320 and rule["base"]["vector"]
    w = C.WINDOWS
    assert [hw % 8 == 0 for hw in w["hws"]] == [True, False]                     # the windowed step: 16-byte route, then one element per lane
    assert all(R.launch_rule(2 * w["P"], w["C"] * w["L"] * hw)["vector"] for hw in w["hws"])      # a window's latent is a multiple of 8 either way
    assert ops.guidance_partials_floats(3, 420) == 3 * 4 and ops.guidance_partials_floats(1, 655360) == 320 * 4
    with pytest.raises(ValueError):
        ops.guidance_partials_floats(1, 1)


# ------------------------------------------------------------------ injected defects, on the model
def model(name, defect=None):
    """What the kernel chain would return for case `name`, computed in float64 and stored in the kernels' formats, with one defect.
    Returns (partials [P, chunks, 4] fp32, sums [P, 4] f64, table [P, 2] fp32, x [P, per] fp32)."""
    p, per = C.SHAPES[name][0], C.per_of(name)
    d = C.inputs(name)
    g = list(C.GUIDANCE[:p])
    eu, ec = d["eps"][:p].reshape(p, per), d["eps"][p:].reshape(p, per)
    t = R.terms(eu, ec, g)
    if defect == "ec_twice":                      # the statistics taken of ec in both places
        t[:, :, 2:] = t[:, :, :2]
    partials = R.chunk_sums(t)[0]
    # the model's chunking is the library's: its size query counts the very partials the model forms
    assert ops.guidance_partials_floats(p, per) == partials.numel(), (R.CH, tuple(partials.shape))
    sums = partials.sum(1)
    if defect == "last_chunk":                    # the fold leaves the last chunk out of latent 1's sums
        sums[1] = partials[1, :-1].sum(0)
    f = R.factor64(sums, per, R.f32s(C.PHI))
    if defect == "biased":                        # per in place of per - 1, in one of the two variances
        var_t = (sums[:, 1] - sums[:, 0] ** 2 / per) / per
        var_e = (sums[:, 3] - sums[:, 2] ** 2 / per) / (per - 1.0)
        f = R.f32s(C.PHI) * var_t.sqrt() / var_e.sqrt() + (1.0 - R.f32s(C.PHI))
    table = torch.stack([torch.tensor(g, dtype=torch.float64), f], dim=1).float()
    used = table.clone()
    if defect == "pair_of_latent_0":              # latent 1 stepped with latent 0's pair
        used[1] = table[0]
    eps, _ = R.scaled_eps64(eu, ec, used)
    x = R.step64("five", eps, eps.abs(), d["x"].reshape(p, per), d["aux"].reshape(p, per), C.COEFFS["five"])[0].float()
    return partials.float(), sums, table, x


def check_all(name, partials, sums, table, x):
    """The GPU tests' checks, in the order of the kernel chain."""
    p, per = C.SHAPES[name][0], C.per_of(name)
    d = C.inputs(name)
    g = list(C.GUIDANCE[:p])
    eu, ec = d["eps"][:p].reshape(p, per), d["eps"][p:].reshape(p, per)
    R.check_chunk_sums(partials, eu, ec, g, label=name)
    R.check_latent_sums(sums, eu, ec, g, label=name)
    R.check_table(table, sums, per, g, C.PHI, label=name)
    eps, m_eps = R.scaled_eps64(eu, ec, table)
    xn, m, _, _ = R.step64("five", eps, m_eps, d["x"].reshape(p, per), d["aux"].reshape(p, per), C.COEFFS["five"])
    oc.assert_elementwise(x, xn, m, 2 * R.ROUNDINGS["five"] * R.U32, label=f"{name} x", u=0.0, where=lambda i: "latent %d, element %d" % divmod(i, per))


@pytest.mark.parametrize("defect,name,placed,passes_rel_l2", [
    ("last_chunk", "2x3CH", "latent sum outside its bound at latent 1", True),
    ("pair_of_latent_0", "3x420", "worst at latent 1", True),
    ("biased", "1x8", "f of latent 0", True),
    ("ec_twice", "3x420", "sum e:", True),
    ("biased", "base", "f of latent 0", True),
])
def test_an_injected_defect_is_placed(defect, name, placed, passes_rel_l2):
    """Each defect fails the per-element checks at the stage and latent where it sits.  Whether the whole-output rel-L2 of x at
    TOL_OP (2e-3) would have passed it, recorded on the model with phi = 0.7 and the step coefficients of the cases: ALL FOUR pass
    it.  The last chunk left out: 6.3e-6 (both variances lose the same third, their ratio barely moves); latent 0's pair: 1.7e-3;
    the biased variance at per = 8: 3.5e-4 (f 0.844 for 0.882); the statistics of ec twice: 4.1e-4 (f = 1 everywhere).  The
    prediction enters x' with weight k_eps c_x0 = 0.025 here, so a factor that is wrong by several percent stays below 2e-3.
    The biased variance at the base shape, per = 655,360, moves f by 5.6e-7 relative (0.7 x 0.95 / (2 per) over f = 0.956): invisible to any whole-output
    figure (rel-L2 of x 2e-8), still outside the table check's 2^-22 = 2.4e-7."""
    check_all(name, *model(name))
    bad = model(name, defect=defect)
    with pytest.raises(AssertionError, match=placed):
        check_all(name, *bad)
    rel = R.rel_l2(bad[3], model(name)[3])
    print(f"{defect}: whole-output rel-L2 of x {rel:.3e}, TOL_OP {TOL_OP}: {'passes' if rel < TOL_OP else 'fails'}")
    assert (rel < TOL_OP) == passes_rel_l2


# ------------------------------------------------------------------ host logic with a recording `ops`
STEP_OPS = ("cfg_ddpm_step", "sampler_step", "cfg_multistep_step", "multistep_step", "cfg_sampler_step_known", "sampler_step_known",
            "cfg_multistep_step_known", "multistep_step_known", "window_step", "known_blend", "latents_to_model_input",
            "latents_to_model_input1", "guidance_table", "cfg_sampler_step_scaled", "cfg_multistep_step_scaled",
            "cfg_sampler_step_known_scaled", "cfg_multistep_step_known_scaled", "window_step_scaled")


class FakeUNet:
    device = torch.device("cpu")
    config = SimpleNamespace(sample_size=2, in_channels=4)

    def prepare(self, *a):
        pass

    def __call__(self, model_in, t, encoder_hidden_states=None, **kw):
        return SimpleNamespace(sample=torch.zeros_like(model_in))


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    for n in STEP_OPS:
        monkeypatch.setattr(ops, n, (lambda n: lambda *a, **k: calls.append((n, a, k)) or torch.zeros(1))(n), raising=False)
    monkeypatch.setattr(ops, "guidance_partials_floats", lambda latents, per: 4 * latents, raising=False)
    return calls


def make_pipe(method):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    return VideoGenPipeline.from_sample_yaml(dict(sample_method=method), unet=FakeUNet())[0]


STEPS = 3
PLAIN = {"ddpm": "cfg_ddpm_step", "ddim": "cfg_ddpm_step", "eulerdiscrete": "cfg_ddpm_step", "dpmsolver++": "cfg_multistep_step"}
KNOWN = {m: ("cfg_multistep_step_known" if m == "dpmsolver++" else "cfg_sampler_step_known") for m in PLAIN}


def denoise(method, mode, **kw):
    pipe = make_pipe(method)
    frames = 13 if mode == "windows" else 4
    unguided = isinstance(kw.get("guidance_scale"), float) and kw["guidance_scale"] <= 1.0
    x, ctx = torch.randn(2, 4, frames, 2, 2), torch.zeros(2 if unguided else 4, 77, 8, dtype=torch.float16)
    if mode == "known":
        m = torch.zeros(2, 1, frames, 2, 2)
        m[:, :, :1] = 1.0
        kw.update(known=torch.randn_like(x), mask=m, known_noise=torch.randn_like(x))
    if mode == "windows":
        kw.update(window_length=8, window_stride=5)
    pipe.denoise(x, ctx, STEPS, kw.pop("guidance_scale", 7.5), torch.Generator().manual_seed(0), **kw)


@pytest.mark.parametrize("method", list(PLAIN))
def test_default_arguments_make_todays_call_sequence(recorded, method):
    """Passes on the parent commit as well: it pins what must not change."""
    denoise(method, "plain")
    assert [c[0] for c in recorded] == ["latents_to_model_input"] + [PLAIN[method]] * STEPS
    assert all(c[1][4] == 7.5 for c in recorded[1:])
    del recorded[:]
    denoise(method, "known")
    assert [c[0] for c in recorded] == ["known_blend"] + [KNOWN[method]] * STEPS
    del recorded[:]
    denoise(method, "windows")
    assert [c[0] for c in recorded] == ["latents_to_model_input"] * 2 + ["window_step"] * STEPS
    assert all(c[1][6] == 7.5 and c[2] == {"multistep": method == "dpmsolver++"} for c in recorded[2:])
    del recorded[:]
    denoise(method, "plain", guidance_scale=1.0)
    assert [c[0] for c in recorded] == ["latents_to_model_input1"] + ["multistep_step" if method == "dpmsolver++" else "sampler_step"] * STEPS


@pytest.mark.parametrize("scale,phi", [(7.5, 0.7), ([5.0, 9.0], 0.0), ((5.0, 9.0), 0.3)])
@pytest.mark.parametrize("method", list(PLAIN))
def test_rescale_or_a_sequence_inserts_the_table_call_before_the_scaled_step(recorded, method, scale, phi):
    for mode, first, step in (("plain", ["latents_to_model_input"], PLAIN[method].replace("cfg_ddpm", "cfg_sampler") + "_scaled"),
                              ("known", ["known_blend"], KNOWN[method] + "_scaled"),
                              ("windows", ["latents_to_model_input"] * 2, "window_step_scaled")):
        del recorded[:]
        denoise(method, mode, guidance_scale=scale, guidance_rescale=phi)
        assert [c[0] for c in recorded] == first + ["guidance_table", step] * STEPS, mode
        for table_call, step_call in zip(recorded[len(first)::2], recorded[len(first) + 1::2]):
            eps, latents, g, rescale, workspace, out = table_call[1]
            assert latents == 2 and rescale == phi and (workspace is None) == (phi == 0.0)
            assert (g.tolist() == [5.0, 9.0]) if not isinstance(scale, float) else g == 7.5
            assert isinstance(eps, list) == (mode == "windows") and (mode != "windows" or len(eps) == 2)      # one call covers all windows
            assert tuple(out.shape) == ((2, 2, 2) if mode == "windows" else (2, 2))
        # table and workspace are allocated once per loop
        assert len({c[1][5].data_ptr() for c in recorded if c[0] == "guidance_table"}) == 1


def test_refusals(recorded):
    for kw, text in ((dict(guidance_rescale=1.5), "guidance_rescale"), (dict(guidance_rescale=-0.1), "guidance_rescale"),
                     (dict(guidance_scale=[5.0]), "1 values for 2"), (dict(guidance_scale=[5.0, 1.0]), "> 1"),
                     (dict(guidance_scale=[5.0, 9.0, 3.0]), "3 values for 2")):
        with pytest.raises(ValueError, match=text):
            denoise("ddim", "plain", **kw)
    assert recorded == []
    assert sampling.check_guidance(1.0, 0.7, 2) == (False, None, 0.0)                 # ignored without guidance, as in diffusers
    assert sampling.check_guidance([5.0, 9.0], 0.5, 2, repeat=2) == (True, [5.0, 5.0, 9.0, 9.0], 0.5)
    assert sampling.check_guidance(torch.tensor([5.0, 9.0]), 0.0, 2) == (True, [5.0, 9.0], 0.0)
    # a 0-dim tensor is one number, as before: no per-prompt count, and <= 1 switches guidance off
    assert sampling.check_guidance(torch.tensor(7.5), 0.5, 3) == (True, None, 0.5)
    assert sampling.check_guidance(torch.tensor(1.0), 0.5, 3) == (False, None, 0.0)


def test_keywords_pass_through(recorded):
    """__call__ of both pipelines, from_sample_yaml and the cascade forward the keyword; chain / windows / chunks forward **kwargs."""
    import inspect
    from lavie_amd import cascade
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.vsr import VideoUpscalePipeline
    for fn in (VideoGenPipeline.__call__, VideoGenPipeline.denoise, VideoUpscalePipeline.__call__, VideoUpscalePipeline.denoise):
        assert inspect.signature(fn).parameters["guidance_rescale"].default == 0.0
    sig = inspect.signature(cascade.text_to_video_cascade).parameters
    assert sig["base_guidance_rescale"].default == 0.0 and sig["vsr_guidance_rescale"].default == 0.0
    _, kw, _ = VideoGenPipeline.from_sample_yaml(dict(sample_method="ddim", guidance_rescale=0.7), unet=FakeUNet())
    assert kw["guidance_rescale"] == 0.7
    assert "guidance_rescale" not in VideoGenPipeline.from_sample_yaml(dict(sample_method="ddim"), unet=FakeUNet())[1]
    seen = []
    pipe = lambda **k: seen.append(k) or type("O", (), {"video": torch.zeros(1, 4, k["video_length"], 2, 2), "images": None})()
    pipe.vae_scale_factor = 8
    cascade.text_to_long_video(pipe, None, 2, overlap=1, video_length=4, guidance_rescale=0.7, height=16, width=16)
    cascade.text_to_long_video(pipe, None, 2, overlap=1, method="windows", video_length=4, guidance_rescale=0.7)
    assert len(seen) == 3 and all(k["guidance_rescale"] == 0.7 for k in seen)
    from lavie_amd.vsr import upscale_in_chunks
    seen_v = []
    vsr = lambda image=None, **k: seen_v.append(k) or type("O", (), {"images": torch.zeros(1, 4, image.shape[2], 2, 2)})()
    upscale_in_chunks(vsr, torch.zeros(1, 3, 10, 2, 2), short_seq=8, guidance_rescale=0.5)
    upscale_in_chunks(vsr, torch.zeros(1, 3, 10, 2, 2), short_seq=8, overlap=2, guidance_rescale=0.5)
    assert len(seen_v) == 3 and all(k["guidance_rescale"] == 0.5 for k in seen_v)
    # VideoGenPipeline.__call__: one value per prompt, repeated per num_images_per_prompt, reaches denoise as one value per latent
    vp = make_pipe("ddim")
    got = {}
    vp.denoise = lambda latents, ctx, steps, g, *a, **k: got.update(g=g, kw=k) or latents
    pe = torch.zeros(2, 77, 8)
    vp(prompt_embeds=pe, negative_prompt_embeds=pe, height=16, width=16, video_length=2, num_inference_steps=2, num_images_per_prompt=2,
       guidance_scale=[5.0, 9.0], guidance_rescale=0.7, output_type="latent", latents=torch.zeros(4, 4, 2, 2, 2))
    assert got["g"] == [5.0, 5.0, 9.0, 9.0] and got["kw"]["guidance_rescale"] == 0.7
    vp(prompt_embeds=pe, negative_prompt_embeds=pe, height=16, width=16, video_length=2, num_inference_steps=2, guidance_scale=7.5,
       output_type="latent", latents=torch.zeros(2, 4, 2, 2, 2))
    assert got["g"] == 7.5 and "guidance_rescale" not in got["kw"]


def test_c_entries_refuse_before_anything_is_launched():
    """Fake pointers, never dereferenced: every refusal names its argument."""
    import ctypes
    from lavie_amd import _lib
    lib = _lib.load()
    refused = lambda rc, word: rc != 0 and word.encode() in lib.lavie_last_error()
    a = _lib.GuidanceTableArgsC()
    assert refused(lib.lavie_guidance_table(None, None), "args")
    assert refused(lib.lavie_guidance_table(ctypes.byref(a), None), "struct_size")
    a.struct_size, a.W, a.P, a.per = ctypes.sizeof(a), 1, 1, 1
    assert refused(lib.lavie_guidance_table(ctypes.byref(a), None), "per=1")
    a.per = 16
    assert refused(lib.lavie_guidance_table(ctypes.byref(a), None), "eps_host")
    coeffs = (1.0, 0.5, 0.3, 0.7, 0.0, 1.0)
    assert refused(lib.lavie_cfg_sampler_step_scaled(0x1000, 0x2000, None, 0x3000, 16, None, 8, *coeffs, None), "table is null")
    assert refused(lib.lavie_cfg_sampler_step_scaled(0x1000, 0x2000, None, 0x3000, 16, 0x4000, 1, *coeffs, None), "per=1")
    assert refused(lib.lavie_cfg_sampler_step_scaled(0x1000, 0x2000, None, 0x3000, 17, 0x4000, 8, *coeffs, None), "n=17")
    assert refused(lib.lavie_cfg_multistep_step_scaled(0x1000, 0x2008, 0x5000, 0x3000, 16, 0x4000, 8, *coeffs, None), "16-byte")
    assert refused(lib.lavie_cfg_multistep_step_scaled(0x1000, 0x2000, None, 0x3000, 16, 0x4000, 8, *coeffs, None), "x0_prev")
    assert refused(lib.lavie_window_step_scaled(None, None, None), "table is null")
    assert lib.lavie_abi_version() == 8
