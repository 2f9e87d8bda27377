"""CPU: the layer cache's references, schedule and Python-side refusals.

The restated walk of tests/layercache_cases.py is held to the oracle bit for bit; the cases are shown to separate the right shallow
output from what a stale, wrong-cut or ignored cache would give by more than 3 TOL_UNET, so the GPU parity test at TOL_UNET decides."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import layercache_cases as LC
from gpu_util import TOL_UNET, rel_l2
from lavie_amd import _lib, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, d) for n in LC.SHAPES for d in LC.DEPTHS]
IDS = [f"{n}-d{d}" for n, d in CASES]


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", list(LC.SHAPES))
def test_restated_full_walk_is_the_oracle(name):
    from oracle import unet_fp32 as O
    sd = {k: v.float() for k, v in LC.base_weights().items()}
    x_old, _, ctx = LC.inputs(name)
    want = O.unet_forward(sd, x_old.float(), LC.T_OLD, ctx.float(), LC.ocfg())
    for depth in LC.DEPTHS:
        out, feature = LC.full(sd, x_old.float(), LC.T_OLD, ctx.float(), LC.ocfg(), depth)
        assert torch.equal(out, want)
        b, f, h, w = LC.SHAPES[name]
        assert tuple(feature.shape) == (b, LC.WIDTHS[1 if depth == LC.ocfg().layers_per_block else 0], f, h, w)
    assert torch.equal(out, LC.refs(name, LC.DEPTHS[-1])["full_old"])


@pytest.mark.parametrize("name,depth", CASES, ids=IDS)
def test_shallow_walk_on_its_own_feature_is_the_full_walk(name, depth):
    """The shallow walk at the SAME input as the full walk that gave the feature recomputes exactly the layers it runs."""
    sd = {k: v.float() for k, v in LC.base_weights().items()}
    x_old, _, ctx = LC.inputs(name)
    out, feature = LC.full(sd, x_old.float(), LC.T_OLD, ctx.float(), LC.ocfg(), depth)
    assert torch.equal(LC.shallow(sd, x_old.float(), LC.T_OLD, ctx.float(), LC.ocfg(), depth, feature), out)


@pytest.mark.parametrize("name,depth", CASES, ids=IDS)
def test_separation_condition(name, depth):
    """The reference shallow output at the new input lies farther than 3 TOL_UNET from the full output at the new input (what a
    forward that ignores the cache gives) and from the refresh output at the old input (what a stale output gives)."""
    r = LC.refs(name, depth)
    ignored, stale = rel_l2(LC.full_new(name), r["shallow"]), rel_l2(r["full_old"], r["shallow"])
    print(f"{name} depth {depth}: shallow vs full(new) {ignored:.4f}, vs full(old) {stale:.4f} (3 TOL_UNET = {3 * TOL_UNET})")
    assert ignored > 3 * TOL_UNET and stale > 3 * TOL_UNET


def test_separation_of_the_cuts():
    """The two depths differ by more than 3 TOL_UNET as well: a walk cut at the wrong depth does not pass for the right one."""
    for name in LC.SHAPES:
        assert rel_l2(LC.refs(name, 1)["shallow"], LC.refs(name, 2)["shallow"]) > 3 * TOL_UNET


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("interval,want", [
    (1, [None] * 7),
    (2, ["refresh", "reuse", "refresh", "reuse", "refresh", "reuse", "refresh"]),
    (3, ["refresh", "reuse", "reuse", "refresh", "reuse", "reuse", "refresh"]),
    (5, ["refresh", "reuse", "reuse", "reuse", "reuse", "refresh", "reuse"]),
])
def test_schedule_over_seven_steps(interval, want):
    got = [sampling.layer_cache_mode(k, sampling.check_layer_cache(interval)) for k in range(7)]
    assert got == want == LC.schedule(7, interval)


def test_schedule_of_a_late_start_begins_with_a_refresh():
    """A run at reduced strength takes timesteps[start:]: the schedule counts executed steps, so its first step refreshes."""
    start, steps, interval = 4, 10, 3
    got = [sampling.layer_cache_mode(i - start, interval) for i in range(start, steps)]
    assert got == ["refresh", "reuse", "reuse", "refresh", "reuse", "reuse"]
    assert sampling.check_layer_cache(None) == 1 and sampling.layer_cache_mode(0, 1) is None


def test_schedule_arguments_are_checked():
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="cache_interval"):
            sampling.check_layer_cache(bad)
    for bad in (0, 1.5, None):
        with pytest.raises(ValueError, match="cache_depth"):
            sampling.check_layer_cache(2, bad)
    with pytest.raises(ValueError, match="window"):
        sampling.check_layer_cache(2, 1, windowed=True)
    assert sampling.check_layer_cache(1, 1, windowed=True) == 1        # off: nothing to refuse


# ------------------------------------------------------------------ Python-side refusals
def test_pipelines_refuse_the_cache_with_frame_windows():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.vsr.pipeline import VideoUpscalePipeline
    unet = SimpleNamespace(config=SimpleNamespace(sample_size=8, in_channels=4), device="cpu")
    pipe = VideoGenPipeline(unet=unet, scheduler=DDIMScheduler())
    shape = (1, 4, 12, 4, 6)
    with pytest.raises(ValueError, match="cache_interval.*window"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 7.5, window_length=8, cache_interval=2)
    with pytest.raises(ValueError, match="cache_interval.*window"):
        pipe(prompt_embeds=torch.zeros(1, 77, 8), negative_prompt_embeds=torch.zeros(1, 77, 8), height=32, width=48, video_length=12,
             num_inference_steps=2, output_type="latent", window_length=8, cache_interval=2)
    with pytest.raises(ValueError, match="cache_interval"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 7.5, cache_interval=0)
    vsr = VideoUpscalePipeline(unet=SimpleNamespace(config=SimpleNamespace(in_channels=7), device="cpu"), scheduler=DDIMScheduler())
    with pytest.raises(ValueError, match="cache_interval.*window"):
        vsr.denoise(torch.zeros(shape), torch.zeros(1, 3, 12, 4, 6), torch.zeros(2, 77, 8), 20, 4, 7.5, window_length=8, cache_interval=3)


def test_from_sample_yaml_reads_the_cache_keys():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    unet = SimpleNamespace(config=SimpleNamespace(sample_size=8, in_channels=4), device="cpu")
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"sample_method": "ddim", "cache_interval": 3, "cache_depth": 2}, unet)
    assert kw["cache_interval"] == 3 and kw["cache_depth"] == 2
    _, kw, _ = VideoGenPipeline.from_sample_yaml({"sample_method": "ddim"}, unet)
    assert "cache_interval" not in kw and "cache_depth" not in kw


def test_model_refuses_reuse_without_enable_layer_cache():
    from lavie_amd.unet import UNet3DConditionModel
    net = UNet3DConditionModel(init_weights=False, **LC.BASE_KW)
    assert net.layer_cache == 0
    x, ctx = torch.zeros(1, 4, 2, 8, 8), torch.zeros(1, 77, 128)
    for mode in ("reuse", "refresh"):
        with pytest.raises(RuntimeError, match="enable_layer_cache"):
            net(x, 10, encoder_hidden_states=ctx, layer_cache=mode)
    with pytest.raises(ValueError, match="layer_cache"):
        net(x, 10, encoder_hidden_states=ctx, layer_cache="always")
    with pytest.raises(ValueError, match="depth=3"):
        net.enable_layer_cache(3)
    with pytest.raises(ValueError, match="depth=0"):
        net.enable_layer_cache(0)
    net.enable_layer_cache(2)                        # no engine yet: recorded, handed to the engine when it is built
    assert net.layer_cache == 2
    net.enable_graph(True)
    with pytest.raises(RuntimeError, match="graph"):
        net(x, 10, encoder_hidden_states=ctx, layer_cache="reuse")
    net.enable_graph(False)
    net.disable_layer_cache()
    assert net.layer_cache == 0
    two = UNet3DConditionModel(init_weights=False, sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
                               down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
    with pytest.raises(ValueError, match="levels"):
        two.enable_layer_cache(1)


def test_layer_cache_session_restores_the_models_setting():
    calls = []
    unet = SimpleNamespace(layer_cache=2, enable_layer_cache=lambda d: calls.append(("on", d)),
                           disable_layer_cache=lambda: calls.append(("off",)))
    with pytest.raises(KeyError):
        with sampling.layer_cache_session(unet, 3, 1):
            raise KeyError("in the loop")
    assert calls == [("on", 1), ("on", 2)]
    calls.clear()
    unet.layer_cache = 0
    with sampling.layer_cache_session(unet, 3, 1):
        pass
    assert calls == [("on", 1), ("off",)]
    calls.clear()
    with sampling.layer_cache_session(unet, 1, 1):   # off: the model is not touched
        pass
    assert calls == []
    with pytest.raises(ValueError, match="no layer cache"):
        with sampling.layer_cache_session(SimpleNamespace(), 2, 1):
            pass


# ------------------------------------------------------------------ the C interface
def test_header_keeps_abi_8_and_bindings_declare_the_entries():
    """Fails on a library without the feature: the symbols do not exist there."""
    header = open(os.path.join(ROOT, "include", "lavie_hip.h")).read()
    assert re.search(r"#define LAVIE_ABI_VERSION 8\b", header)
    lib = _lib.load()
    assert lib.lavie_abi_version() == 8 == _lib.ABI_VERSION
    for name in ("lavie_unet_set_layer_cache", "lavie_unet_layer_cache_bytes", "lavie_unet_forward_cached"):
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.lavie_unet_forward_cached.argtypes[-2] is ctypes.c_int            # the mode, in front of the stream
    assert lib.lavie_unet_layer_cache_bytes.restype is ctypes.c_longlong
    for word, value in (("OFF", 0), ("REFRESH", 1), ("REUSE", 2)):
        assert re.search(r"#define LAVIE_LAYER_CACHE_%s %d\b" % (word, value), header)
    # null handles are refused before anything else is looked at
    assert lib.lavie_unet_set_layer_cache(None, 1) != 0 and b"null handle" in lib.lavie_last_error()
    assert lib.lavie_unet_layer_cache_bytes(None) == -1
    assert lib.lavie_unet_forward_cached(None, None, None, None, None, None, 1, 1, 8, 8, 77, 2, None) != 0
    assert b"null handle" in lib.lavie_last_error()
