"""Perturbed-attention guidance before a GPU is involved: the patched oracle and the separation the GPU forward test
relies on; the float64 step model, its bound and an injected defect; the adaptive scale; the refusals of the C entry points, none of
which reaches HIP; the Python surfaces.  CPU only."""
import ctypes
import math
import os
import re

import pytest
import torch

import opcheck as oc
import pagcases as P
from gpu_util import TOL_UNET, rel_l2

f16, f32t, f64 = torch.float16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
             down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))


# ------------------------------------------------------------------ the patched oracle
def test_nothing_selected_is_the_oracle_bit_for_bit():
    from oracle import unet_fp32 as O
    x, ctx, t = P.forward_inputs("F4-16x16")
    _, plain = P.forward_refs("F4-16x16", P.LAYERS_BITS)
    sd = P.base_weights()
    for layers, perturbed in (((), 1), (P.LAYERS_BITS, 0), (("mid_bloc",), 1)):
        with P.patched_oracle(layers, x.shape[0], perturbed):
            assert torch.equal(O.unet_forward(sd, x.float(), t, ctx.float(), P.ocfg()), plain), (layers, perturbed)
    assert O.cross_attention.__module__ == "oracle.unet_fp32"                 # the original is back


@pytest.mark.parametrize("name", list(P.FORWARD_CASES))
def test_mid_block_selected_leaves_the_leading_entries_alone(name):
    ref, plain = P.forward_refs(name, P.LAYERS_BITS)
    assert torch.equal(ref[:2], plain[:2])
    assert not torch.equal(ref[2], ref[1])                                   # the perturbed entry differs from its unperturbed twin
    assert rel_l2(ref[2], ref[1]) > 1e-3


@pytest.mark.parametrize("name", list(P.FORWARD_CASES))
def test_separation_of_the_perturbed_entry(name):
    """What makes test_gpu_pag.py's forward parity fail on an engine that ignores the setting: with the layer set of the parity case
    the perturbed third of the reference is farther than 3 TOL_UNET from the prompt third.  `mid_block` alone is not (one block of
    sixteen, at a 2 x 2 / 3 x 5 image): it stays a bit-property case."""
    ref, plain = P.forward_refs(name, P.LAYERS_PARITY)
    d, d_mid = rel_l2(ref[2], ref[1]), rel_l2(P.forward_refs(name, P.LAYERS_BITS)[0][2], plain[1])
    print(f"{name}: rel_l2(perturbed, prompt) = {d:.4f} with {P.LAYERS_PARITY}, {d_mid:.4f} with {P.LAYERS_BITS}; 3 TOL_UNET = {3 * TOL_UNET}")
    assert torch.equal(ref[:2], plain[:2])
    assert d > 3 * TOL_UNET
    assert P.LAYERS_PARITY == ("mid_block", "up_blocks.1") and P.LAYERS_BITS == ("mid_block",)


def test_selection_rule():
    assert P.selected("mid_block.attentions.0", ("mid_block",)) and P.selected("up_blocks.1.attentions.2", ("up_blocks.1",))
    assert P.selected("up_blocks.1.attentions.0", ("up_blocks.1.attentions.0",))
    assert not P.selected("up_blocks.10.attentions.0", ("up_blocks.1",)) and not P.selected("mid_block.attentions.0", ("mid_bloc",))


# ------------------------------------------------------------------ the float64 step model
STEP_CASES = [(n, fam, cfg) for n in P.SIZES for fam in P.FAMILIES for cfg in P.CFGS]
STEP_IDS = [f"{n}-{fam}-{'cfg' if cfg else 'nocfg'}" for n, fam, cfg in STEP_CASES]


def model32(family, d, cfg, g, s):
    """The kernel's arithmetic with every fp32 rounding point of sampler_pag.hip / sampler_element.h applied to float64 values."""
    r = lambda t: t.float().double()
    g, s = P.R.f32s(g), P.R.f32s(s)
    k_x, k_e, c_x0, c_xt, c4 = (P.R.f32s(c) for c in P.COEFFS[family])
    parts = [p.double() for p in d["eps"]]
    ec, ep, x, aux = parts[-2], parts[-1], d["x"].double(), d["aux"].double()
    e = r(g * r(ec - parts[0]) + parts[0]) if cfg else ec
    eps = r(s * r(ec - ep) + e) if s != 0 else e
    x0 = r(-k_e * eps + r(k_x * x))
    if family == "multistep":
        dd = r(c4 * r(x0 - aux) + x0) if c4 != 0 else x0
        return r(r(c_xt * x) + r(c_x0 * dd)).float(), x0.float()
    xn = r(r(c_xt * x) + r(c_x0 * x0))
    return (r(c4 * aux + xn) if c4 != 0 else xn).float(), None


@pytest.mark.parametrize("name,family,cfg", STEP_CASES, ids=STEP_IDS)
def test_fp32_model_meets_the_bound_and_a_swap_does_not(name, family, cfg):
    d = P.step_inputs(name, cfg)
    xn, m, x0, m0 = P.step64(family, d["eps"], cfg, d["x"], d["aux"], P.GUIDANCE, P.PAG_SCALE)
    got_x, got_h = model32(family, d, cfg, P.GUIDANCE, P.PAG_SCALE)
    c = 2 * P.ROUNDINGS[family] * P.U32
    oc.assert_elementwise(got_x, xn, m, c, label=f"{name} model x", u=0.0)
    if family == "multistep":
        oc.assert_elementwise(got_h, x0, m0, 2 * P.ROUNDINGS["history"] * P.U32, label=f"{name} model x0_prev", u=0.0)
    # the injected defect: prompt and perturbed parts exchanged
    bad, _, bad0, _ = P.step64(family, d["eps"], cfg, d["x"], d["aux"], P.GUIDANCE, P.PAG_SCALE, swap=True)
    with pytest.raises(AssertionError, match="outside the bound"):
        oc.assert_elementwise(bad.float(), xn, m, c, label=f"{name} swapped x", u=0.0)
    outside = ~((bad - xn).abs() <= c * m)
    print(f"{name} {family} cfg={cfg}: swapped parts leave the bound at {int(outside.sum())} of {outside.numel()} elements")
    assert outside.float().mean() > 0.9
    if family == "multistep":
        with pytest.raises(AssertionError, match="outside the bound"):
            oc.assert_elementwise(bad0.float(), x0, m0, 2 * P.ROUNDINGS["history"] * P.U32, label=f"{name} swapped x0_prev", u=0.0)


@pytest.mark.parametrize("family", P.FAMILIES)
@pytest.mark.parametrize("cfg", P.CFGS)
def test_zero_scale_and_equal_parts_reduce_to_the_plain_formula(family, cfg):
    d = P.step_inputs("n420", cfg)
    eps = d["eps"]
    if cfg:
        table = torch.tensor([[P.R.f32s(P.GUIDANCE), 1.0]], dtype=f32t)
        e, m = P.R.scaled_eps64(eps[0][None], eps[1][None], table)
        e, m = e[0], m[0]
    else:
        e, m = eps[0].double(), eps[0].double().abs()
    plain = P.R.step64(family, e, m, d["x"], d["aux"], P.COEFFS[family])
    zero = P.step64(family, eps, cfg, d["x"], d["aux"], P.GUIDANCE, 0.0)
    same = torch.cat([eps[:-1], eps[-2:-1]])                                 # ep = ec
    equal = P.step64(family, same, cfg, d["x"], d["aux"], P.GUIDANCE, P.PAG_SCALE)
    for got in (zero, equal):
        assert torch.equal(got[0], plain[0]) and (family != "multistep" or torch.equal(got[2], plain[2]))
    assert torch.equal(zero[1], plain[1])                                    # and the magnitude sum is the plain one at s = 0


def test_launch_rule_and_sizes():
    assert P.launch_rule(8) == (True, 1) and P.launch_rule(420) == (False, 2) and P.launch_rule(P.SIZES["two-workgroups+8"]) == (True, 3)
    src = open(os.path.join(ROOT, "lavie_amd", "csrc", "sampler_pag.hip")).read()
    assert "__launch_bounds__(256)" in src and "a.n % 8 == 0" in src and "dim3(256)" in src


# ------------------------------------------------------------------ adaptive scale
def test_adaptive_scale_is_diffusers_formula():
    from lavie_amd import sampling
    for s, a, t in ((3.0, 0.0, 999), (3.0, 0.002, 981), (3.0, 0.002, 500), (3.0, 0.01, 1), (0.0, 0.5, 700), (5.0, 0.005, 0)):
        want = P.pag_scale_at(s, a, t)
        assert sampling.pag_scale_at(s, a, t) == want and want >= 0.0, (s, a, t)
    assert sampling.pag_scale_at(3.0, 0.002, 981) == 3.0 - 0.002 * 19
    assert sampling.pag_scale_at(3.0, 0.01, 1) == 0.0                          # clamped
    assert sampling.pag_scale_at(3.0, 0.0, 1) == 3.0
    assert sampling.pag_scale_at(3.0, 0.002, torch.tensor(500)) == P.pag_scale_at(3.0, 0.002, 500)


# ------------------------------------------------------------------ the C entry points refuse before HIP
def lib_or_skip():
    from lavie_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.fail("liblavie_hip.so is not built: build() first")
    return _lib.load()


def test_entry_points_are_declared_and_bound():
    from lavie_amd import _lib
    header = open(os.path.join(ROOT, "include", "lavie_hip.h")).read()
    for name in ("lavie_cfg_pag_sampler_step", "lavie_pag_sampler_step", "lavie_cfg_pag_multistep_step", "lavie_pag_multistep_step",
                 "lavie_unet_set_pag"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    assert re.search(r"int lavie_unet_set_pag\(lavie_unet_t h, const char\* const\* layers_host, int n_layers, int perturbed\);", header)
    assert _lib.ABI_VERSION == 8 and re.search(r"#define LAVIE_ABI_VERSION 8\b", header)
    assert "_known), frame-window" in header and "(_scaled) forms" in header    # the out-of-scope statement


def test_step_entries_refuse_bad_arguments():
    lib = lib_or_skip()
    ok, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    co = (1.0, 0.5, 0.3, 0.7)
    nan = float("nan")

    def refused(rc, text):
        msg = lib.lavie_last_error().decode()
        assert rc != 0 and text in msg, (text, msg)

    cfg5 = lambda eps, x, aux, m, n, g=7.5, c4=0.1, scale=0.9, s=3.0: lib.lavie_cfg_pag_sampler_step(eps, x, aux, m, n, g, *co, c4, scale, s, None)
    one5 = lambda eps, x, aux, m, n, c4=0.1, scale=0.9, s=3.0: lib.lavie_pag_sampler_step(eps, x, aux, m, n, *co, c4, scale, s, None)
    cfgm = lambda eps, x, aux, m, n, g=7.5, c4=0.5, scale=0.9, s=3.0: lib.lavie_cfg_pag_multistep_step(eps, x, aux, m, n, g, *co, c4, scale, s, None)
    onem = lambda eps, x, aux, m, n, c4=0.5, scale=0.9, s=3.0: lib.lavie_pag_multistep_step(eps, x, aux, m, n, *co, c4, scale, s, None)
    for fn in (cfg5, one5, cfgm, onem):
        refused(fn(None, ok, ok, ok, 48), "eps is null")
        refused(fn(ok, None, ok, ok, 48), "x is null")
        refused(fn(ok, ok, ok, None, 48), "model_in is null")
        refused(fn(ok, ok, ok, ok, 0), "n=0")
        refused(fn(ok, ok, ok, ok, 48, s=nan), "pag_scale (nan) is not finite")
        refused(fn(ok, ok, ok, ok, 48, s=float("inf")), "pag_scale")
        refused(fn(ok, ok, ok, ok, 48, scale=nan), "next_input_scale")
        refused(fn(ok, ok, ok, ok, 48, s=-0.25), "pag_scale=-0.25 must be >= 0")
        # n % 8 == 0: the eight-element form.  A misaligned eps puts every part, the perturbed third included, off a 16-byte boundary
        refused(fn(odd, ok, ok, ok, 48), "eps at")
        refused(fn(ok, odd, ok, ok, 48), "x at")
        refused(fn(ok, ok, odd, ok, 48), "16-byte aligned")
        refused(fn(ok, ok, ok, odd, 48), "model_in at")
    refused(cfg5(ok, ok, None, ok, 48), "noise is null")
    refused(one5(ok, ok, None, ok, 48), "noise is null")
    refused(cfgm(ok, ok, None, ok, 48), "x0_prev is null")
    refused(onem(ok, ok, None, ok, 48, c4=0.0), "x0_prev is null")
    refused(cfg5(ok, ok, ok, ok, 48, g=nan), "guidance")
    refused(cfgm(ok, ok, ok, ok, 48, c4=nan), "c_prev")


def make_handle(lib, net):
    from lavie_amd import _lib
    handle, cfg_c = ctypes.c_void_p(), net._config_c()
    _lib.check(lib.lavie_unet_create(ctypes.byref(cfg_c), ctypes.byref(handle)), "lavie_unet_create")
    return handle


def names(*entries):
    return (ctypes.c_char_p * max(len(entries), 1))(*[e.encode() for e in entries]), len(entries)


def test_set_pag_refuses_bad_arguments():
    """no GPU here, so the handles are not finalized: the arguments are judged first, and only a call that passes them is refused for
    that (on a finalized handle the same calls are made by the host checker, csrc/hostcheck/driver.cpp, and by test_gpu_pag.py)"""
    from lavie_amd.interpolation import UNet3DConditionModel as InterpUNet
    from lavie_amd.unet import UNet3DConditionModel
    lib = lib_or_skip()

    def refused(rc, *texts):
        msg = lib.lavie_last_error().decode()
        assert rc != 0 and all(t in msg for t in texts), (texts, msg)

    h = make_handle(lib, UNet3DConditionModel(init_weights=False, **SMALL))
    try:
        refused(lib.lavie_unet_set_pag(None, *names("mid_block"), 1), "null handle")
        refused(lib.lavie_unet_set_pag(h, *names("mid_blocks"), 1), "layers_host[0]='mid_blocks'", "selects no transformer")
        refused(lib.lavie_unet_set_pag(h, *names("mid_block", "down_blocks.1"), 1), "layers_host[1]='down_blocks.1'", "selects no transformer")
        refused(lib.lavie_unet_set_pag(h, *names("up_blocks.1.attentions.3"), 1), "selects no transformer")
        refused(lib.lavie_unet_set_pag(h, *names("mid_block"), -1), "perturbed=-1")
        refused(lib.lavie_unet_set_pag(h, None, 1, 1), "layers_host")
        refused(lib.lavie_unet_set_pag(h, *names("mid_block", "up_blocks.1.attentions.2", "down_blocks.0"), 1), "finalize")
    finally:
        lib.lavie_unet_destroy(h)
    h = make_handle(lib, InterpUNet(init_weights=False, sample_size=8, in_channels=8, block_out_channels=(256, 512), cross_attention_dim=128,
                                    use_first_frame=True, down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
                                    up_block_types=("UpBlock3D", "CrossAttnUpBlock3D")))
    try:
        refused(lib.lavie_unet_set_pag(h, *names("mid_block"), 1), "layers_host[0]='mid_block'", "not the plain spatial self-attention", "sparse-causal")
    finally:
        lib.lavie_unet_destroy(h)


def test_host_checker_makes_the_same_calls():
    src = open(os.path.join(ROOT, "lavie_amd", "csrc", "hostcheck", "driver.cpp")).read()
    for name in ("lavie_cfg_pag_sampler_step", "lavie_pag_sampler_step", "lavie_cfg_pag_multistep_step", "lavie_pag_multistep_step",
                 "lavie_unet_set_pag"):
        assert name in src
    for text in ('"pag_scale=-0.5"', '"selects no transformer"', '"plain spatial self-attention"', '"perturbed=-1"', '"n=0"', '"eps at"'):
        assert text in src, text


# ------------------------------------------------------------------ Python surfaces
def small_unet():
    from lavie_amd.unet import UNet3DConditionModel
    return UNet3DConditionModel(init_weights=False, **SMALL)


def test_unet_set_pag_validates_and_stores():
    net = small_unet()
    assert net.pag == ((), 0)
    net.set_pag(["mid_block", "up_blocks.1.attentions.0"], 1)
    assert net.pag == (("mid_block", "up_blocks.1.attentions.0"), 1)
    net.set_pag("mid_block", 2)
    assert net.pag == (("mid_block",), 2)
    for bad, text in ((("mid_blocks",), "selects no transformer"), (("down_blocks.1",), "selects no transformer")):
        with pytest.raises(ValueError, match=text):
            net.set_pag(bad, 1)
        assert net.pag == (("mid_block",), 2)
    with pytest.raises(ValueError, match="perturbed=-1"):
        net.set_pag(("mid_block",), -1)
    net.set_pag(("mid_block",), 0)
    assert net.pag == ((), 0)
    net.set_pag(("mid_block",), 1)
    net.disable_pag()
    assert net.pag == ((), 0)


def call_kw(p=1, **kw):
    g = torch.Generator().manual_seed(1)
    base = dict(prompt_embeds=torch.randn(p, 77, 128, generator=g), negative_prompt_embeds=torch.randn(p, 77, 128, generator=g),
                height=64, width=64, video_length=2, num_inference_steps=2, guidance_scale=7.5, output_type="latent", pag_scale=3.0)
    base.update(kw)
    return base


def test_forbidden_combinations_raise_naming_both_arguments():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline(unet=small_unet())
    lat = torch.zeros(1, 4, 2, 8, 8)
    for kw, other in ((dict(known_latents=lat), "known_latents"), (dict(video=torch.zeros(1, 2, 64, 64, 3, dtype=torch.uint8)), "video"),
                      (dict(known_latents=lat, known_mask=torch.ones(1, 1, 2, 8, 8)), "known_latents"),
                      (dict(known_mask=torch.ones(1, 1, 2, 8, 8)), "known_mask"), (dict(window_length=1), "window_length"),
                      (dict(guidance_rescale=0.5), "guidance_rescale"), (dict(guidance_scale=[7.5]), "guidance_scale")):
        with pytest.raises(ValueError) as e:
            pipe(**call_kw(**kw))
        assert "pag_scale" in str(e.value) and other in str(e.value), (other, str(e.value))
    ctx3, ctx2 = torch.zeros(3, 77, 128, dtype=f16), torch.zeros(2, 77, 128, dtype=f16)
    for kw, other in ((dict(known=lat), "known"), (dict(known=lat, mask=torch.ones(1, 1, 2, 8, 8)), "known"), (dict(window_length=1), "window_length"),
                      (dict(guidance_rescale=0.5), "guidance_rescale")):
        with pytest.raises(ValueError) as e:
            pipe.denoise(lat, ctx3, 2, 7.5, pag_scale=3.0, **kw)
        assert "pag_scale" in str(e.value) and other in str(e.value), (other, str(e.value))
    with pytest.raises(ValueError, match="guidance_scale"):
        pipe.denoise(lat, ctx3, 2, [7.5], pag_scale=3.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pag_scale"):
            pipe(**call_kw(pag_scale=bad))
        with pytest.raises(ValueError, match="pag_adaptive_scale"):
            pipe(**call_kw(pag_adaptive_scale=bad))
    assert pipe.unet.pag == ((), 0)
    del ctx2


def test_too_many_prompts_raise_before_the_engine():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline(unet=small_unet())
    with pytest.raises(ValueError, match="at most 2 prompts"):
        pipe(**call_kw(p=3))
    with pytest.raises(ValueError, match="at most 2 prompts"):
        pipe(**call_kw(p=1, num_images_per_prompt=3))
    with pytest.raises(ValueError, match="at most 4 prompts"):
        pipe(**call_kw(p=5, guidance_scale=1.0))
    with pytest.raises(ValueError, match="at most 2 prompts"):
        pipe.denoise(torch.zeros(3, 4, 2, 8, 8), torch.zeros(9, 77, 128, dtype=f16), 2, 7.5, pag_scale=3.0)
    with pytest.raises(ValueError, match="at most 4 prompts"):
        pipe.denoise(torch.zeros(5, 4, 2, 8, 8), torch.zeros(10, 77, 128, dtype=f16), 2, 1.0, pag_scale=3.0)
    assert VideoGenPipeline.check_pag(3.0, 0.0, 2, 7.5, 0.0) and VideoGenPipeline.check_pag(3.0, 0.0, 4, 1.0, 0.0)
    assert not VideoGenPipeline.check_pag(0.0, 0.0, 8, 7.5, 0.7, window_length=4)      # pag_scale == 0: today's call, nothing judged


def test_step_dispatch_and_wrappers():
    from lavie_amd import ops, sampling
    assert sampling.STEP_WRAPPERS[False, "pag", False] == "pag_sampler_step" and sampling.STEP_WRAPPERS[False, "pag_cfg", False] == "cfg_pag_sampler_step"
    assert sampling.STEP_WRAPPERS[True, "pag", False] == "pag_multistep_step" and sampling.STEP_WRAPPERS[True, "pag_cfg", False] == "cfg_pag_multistep_step"
    assert all(hasattr(ops, name) for name in sampling.STEP_WRAPPERS.values())
    seen = []
    names_ = {"cfg_pag_sampler_step": None, "pag_multistep_step": None}
    try:
        for name in names_:
            names_[name] = getattr(ops, name)
            setattr(ops, name, lambda *a, _n=name: seen.append((_n, a)))
        sampling.step("eps", "x", "aux", "min", sampling.PagGuidance(7.5, 2.5), (1, 2, 3, 4, 5), 0.9, False)
        sampling.step("eps", "x", "aux", "min", sampling.PagGuidance(None, 1.5), (1, 2, 3, 4, 5), 0.8, True)
    finally:
        for name, fn in names_.items():
            setattr(ops, name, fn)
    assert seen == [("cfg_pag_sampler_step", ("eps", "x", "aux", "min", 7.5, 2.5, (1, 2, 3, 4, 5), 0.9)),
                    ("pag_multistep_step", ("eps", "x", "aux", "min", 1.5, (1, 2, 3, 4, 5), 0.8))]
    with pytest.raises(ValueError, match="known region"):
        sampling.step("eps", "x", "aux", "min", sampling.PagGuidance(7.5, 2.5), (1, 2, 3, 4, 5), 0.9, False, region=(1, 2, 3, 4))
    with pytest.raises(ValueError):
        ops.cfg_pag_sampler_step(torch.zeros(3, 8, dtype=f16), torch.zeros(8), None, torch.zeros(3, 8, dtype=f16), 7.5, 3.0, (1, 2, 3, 4, 0))   # CPU tensors


def test_yaml_keys_and_cascade_keywords(monkeypatch):
    from lavie_amd import cascade
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net = small_unet()
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"pag_scale": 3, "pag_adaptive_scale": 0.002, "pag_applied_layers": ["mid_block", "up_blocks.1"]}, net)
    assert kw["pag_scale"] == 3.0 and kw["pag_adaptive_scale"] == 0.002 and kw["pag_applied_layers"] == ("mid_block", "up_blocks.1")
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"pag_applied_layers": "mid_block"}, net)
    assert kw["pag_applied_layers"] == ("mid_block",) and "pag_scale" not in kw
    _, kw, _ = VideoGenPipeline.from_sample_yaml({}, net)
    assert not any(k.startswith("pag") for k in kw)

    class Pipe:
        unet, scheduler, device = None, None, "cpu"

        def __init__(self):
            self.calls = []

        def __call__(self, **kw):
            self.calls.append(kw)
            raise KeyError("stop after the base stage")

    for extra, want in ((dict(base_pag_scale=3.0, base_pag_adaptive_scale=0.001, base_pag_applied_layers=("mid_block", "up_blocks.1")),
                         dict(pag_scale=3.0, pag_adaptive_scale=0.001, pag_applied_layers=("mid_block", "up_blocks.1"))), ({}, {})):
        base_pipe = Pipe()
        with pytest.raises(KeyError):
            cascade.text_to_video_cascade(base_pipe, None, None, Pipe(), *([None] * 8), **extra)
        got = {k: v for k, v in base_pipe.calls[0].items() if k.startswith("pag")}
        assert got == want
