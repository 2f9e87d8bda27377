"""FreeU before a GPU is involved: the mode-sum formula against the torch.fft restatement of diffusers'
fourier_filter; the fp32 model of the two kernels inside the bound of every GPU case; injected defects located; the launch geometry
tied to the library through `hostcheck optrace`; the host API.  CPU only; the optrace test needs hipcc."""
import math
import os
import re
import shutil

import pytest
import torch

import freeucases as FC
import opcases as C
import opcheck as oc
from gpu_util import TOL_OP, rel_l2

f16, f32t, f64 = torch.float16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the formula
@pytest.mark.parametrize("H,W", FC.FORMULA_SIZES, ids=[f"{h}x{w}" for h, w in FC.FORMULA_SIZES])
def test_mode_sums_equal_the_fft_filter(H, W):
    x = torch.randn(2, 3, H, W, dtype=f64, generator=C.gen("formula", H, W))
    for s in (0.9, 0.2, 1.5):
        d = (FC.fourier_filter_modes(x, s) - FC.fourier_filter_fft(x, s)).abs().max().item()
        print(f"{H}x{W} s={s}: max |modes - fft| = {d:.3e}")
        assert d <= 1e-12
    assert len(FC.mode_set(H, W)) == (1 + (H > 1)) * (1 + (W > 1))
    assert torch.equal(FC.fourier_filter_modes(x, 1.0), x)


# ------------------------------------------------------------------ the bound is attainable
CASES = FC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fp32_model_meets_its_bound(case):
    """the two kernels in torch fp32, same slab order: zero offenders.  If this fails, K_FREEU or terms() is miscounted: fix the count."""
    case.check(case.model(), label="model ")


def test_in_place_cases_are_the_same_arithmetic():
    for c in FC.in_place_cases()[-2:]:
        c.check(c.model(), label="model ")


# ------------------------------------------------------------------ injected defects
def caught(fn, *texts):
    with pytest.raises(AssertionError) as e:
        fn()
    for t in texts:
        assert t in str(e.value), (t, str(e.value))
    return str(e.value)


def offenders(case, got):
    """flat indices of the skip elements outside the bound"""
    ref, scale = case.ref
    err = (got.to(f64) - ref).abs()
    return (~(err <= oc.U16 * ref.abs() + case.c * scale)).nonzero()


@pytest.fixture(scope="module")
def mid():
    """3 x 10 x 16, 1280 / 640 channels, (b, s) = (1.6, 0.2), N(0, 1): two runs of slabs per image, the last slab of each image full"""
    case = FC.case(3, 10, 16, 1280, 640, 1.6, 0.2, "normal")
    return case, case.model()


def test_dropped_sine_sum_of_one_mode(mid):
    case, good = mid
    x = FC.images(case.inputs["skip"].to(f64), case.NI, case.H, case.W)
    bad = FC.as_rows(FC.fourier_filter_modes(x, case.s, drop_sine_of=(case.H - 1, 0))).to(f16)
    r = rel_l2(bad, case.ref[0])
    print(f"dropped sine sum of mode (-1, 0): rel-L2 {r:.3e} (TOL_OP {TOL_OP})")
    assert r > TOL_OP                                        # visible to the whole-tensor criterion as well
    caught(lambda: case.check({**good, "skip_out": bad}), "skip_out")
    off = offenders(case, bad)
    rows = off[:, 0] % (case.H * case.W) // case.W           # y of every offender: the mode's sine vanishes at y = 0 and y = H / 2
    assert off.numel() and not ((rows == 0) | (rows == case.H // 2)).any()


def test_last_slab_left_out_of_one_image(mid):
    case, good = mid
    part = FC.model_sums(case.inputs["skip"], case.NI, case.H, case.W, skip_last_slab_of=1)
    bad = FC.model_apply(case.inputs["skip"], part, case.NI, case.H, case.W, case.s)
    r = rel_l2(bad, case.ref[0])
    print(f"last slab of image 1 left out: rel-L2 {r:.3e} (TOL_OP {TOL_OP})")
    assert r > TOL_OP
    msg = caught(lambda: case.check({**good, "skip_out": bad}), "(frame 1,")
    off = offenders(case, bad)
    assert off.numel() and (off[:, 0] // (case.H * case.W) == 1).all(), msg       # image 1 alone


def test_scaling_eight_channels_too_many(mid):
    case, good = mid
    bad = FC.model_h(case.inputs["h"], case.b, cols=case.C_h // 2 + 8)
    r = rel_l2(bad, good["h_out"])
    print(f"C_h / 2 + 8 channels scaled: rel-L2 {r:.3e} (TOL_OP {TOL_OP})")
    assert r > TOL_OP
    caught(lambda: case.check({**good, "h_out": bad}), f"at or above channel {case.C_h // 2} changed", f"channel {case.C_h // 2}")
    changed = (bad.view(torch.int16) != good["h_out"].view(torch.int16)).nonzero()
    assert changed[:, 1].min() == case.C_h // 2 and changed[:, 1].max() == case.C_h // 2 + 7


def test_image_filtered_with_its_neighbours_sums(mid):
    case, good = mid
    part = FC.model_sums(case.inputs["skip"], case.NI, case.H, case.W)
    bad = FC.model_apply(case.inputs["skip"], part, case.NI, case.H, case.W, case.s, sums_of={2: 1})
    r = rel_l2(bad, case.ref[0])
    print(f"image 2 filtered with image 1's sums: rel-L2 {r:.3e} (TOL_OP {TOL_OP})")
    assert r > TOL_OP
    caught(lambda: case.check({**good, "skip_out": bad}), "(frame 2,")
    off = offenders(case, bad)
    assert (off[:, 0] // (case.H * case.W) == 2).all()
    # with a dominant constant mode the neighbour's sums are nearly the image's own: the whole-tensor criterion passes it, the bound does not
    dc = FC.case(3, 10, 16, 1280, 640, 1.2, 0.9, "offset8")
    part = FC.model_sums(dc.inputs["skip"], dc.NI, dc.H, dc.W)
    bad = FC.model_apply(dc.inputs["skip"], part, dc.NI, dc.H, dc.W, dc.s, sums_of={2: 1})
    r = rel_l2(bad, dc.ref[0])
    print(f"the same at s = 0.9 on offset data: rel-L2 {r:.3e} (TOL_OP {TOL_OP})")
    assert r < TOL_OP
    caught(lambda: dc.check({**dc.model(), "skip_out": bad}), "(frame 2,")


# ------------------------------------------------------------------ the launch geometry, from the library's own launcher
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_launch_mirror_is_the_librarys():
    cases = FC.all_cases() + FC.in_place_cases()
    lines = [C.optrace_line(e, ints, 0, 0) for c in cases for e, ints in c.calls]
    refused = ["freeu C_h=24 C2=32 NI=1 H=2 W=2 b_milli=1200 s_milli=900 force_tile=0 force_splits=0",
               "freeu C_h=32 C2=12 NI=1 H=2 W=2 b_milli=1200 s_milli=900 force_tile=0 force_splits=0"]
    blocks = C.optrace(lines + refused)
    for c, (_, got) in zip(cases, blocks):
        want = FC.launches(c.C_h, c.C2, c.NI, c.H, c.W, c.b, c.s, c.in_place)
        assert [(C.launch_name(l), C.launch_grid(l)) for l in got] == want, (c.name, got, want)
        assert all(l.rsplit(" ", 3)[2] == "256,1,1" and l.rsplit(" ", 3)[3] == "0" for l in got)
    for _, got in blocks[len(cases):]:
        assert got == ["!! refused"]
    geoms = {(c.H, c.W): FC.geom(c.H, c.W) for c in cases}
    assert any(min(spr, nslabs) > 1 for _, nslabs, spr, _ in geoms.values())             # a workgroup that walks more than one slab
    assert any(runs > 1 for *_, runs in geoms.values())                                  # partials the apply kernel folds
    assert any(P % FC.SLAB != 0 and nslabs > 1 for P, nslabs, _, _ in geoms.values())    # a ragged last slab behind full ones
    assert any(nslabs % spr != 0 and runs > 1 for _, nslabs, spr, runs in geoms.values())        # a last run shorter than the others
    assert FC.geom(37, 53) == (1961, 62, 8, 8) and FC.geom(5, 8) == (40, 2, 4, 1) and FC.geom(80, 128) == (10240, 320, 40, 8)


def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, "lavie_amd", "csrc", "ops.h")).read()
    m = re.search(r"kFreeuSlab = (\d+), kFreeuMaxRuns = (\d+), kFreeuMinRunSlabs = (\d+), kFreeuSums = (\d+)", src)
    assert tuple(int(v) for v in m.groups()) == (FC.SLAB, FC.MAX_RUNS, FC.MIN_RUN_SLABS, FC.SUMS)


# ------------------------------------------------------------------ host API
SMALL = dict(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
             down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))


def small_unet():
    from lavie_amd.unet import UNet3DConditionModel
    return UNet3DConditionModel(init_weights=False, **SMALL)


def test_enable_freeu_validates_and_stores():
    net = small_unet()
    assert net.freeu == (1.0, 1.0, 1.0, 1.0)
    net.enable_freeu(0.9, 0.2, 1.5, 1.6)                       # diffusers' order: s1, s2, b1, b2
    assert net.freeu == (0.9, 0.2, 1.5, 1.6)
    for bad in ((0.0, 0.2, 1.5, 1.6), (0.9, -1.0, 1.5, 1.6), (0.9, 0.2, float("nan"), 1.6), (0.9, 0.2, 1.5, float("inf"))):
        with pytest.raises(ValueError, match="finite and > 0"):
            net.enable_freeu(*bad)
        assert net.freeu == (0.9, 0.2, 1.5, 1.6)
    net.disable_freeu()
    assert net.freeu == (1.0, 1.0, 1.0, 1.0)


def test_yaml_key_and_pipelines_reach_the_model():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.vsr.pipeline import VideoUpscalePipeline
    net = small_unet()
    pipe, kw, cfg = VideoGenPipeline.from_sample_yaml({"freeu": {"s1": 0.9, "s2": 0.2, "b1": 1.2, "b2": 1.4}}, net)
    assert net.freeu == (0.9, 0.2, 1.2, 1.4) and "freeu" not in kw
    pipe.disable_freeu()
    assert net.freeu == (1.0, 1.0, 1.0, 1.0)
    VideoGenPipeline.from_sample_yaml({}, net)
    assert net.freeu == (1.0, 1.0, 1.0, 1.0)
    with pytest.raises(KeyError):
        VideoGenPipeline.from_sample_yaml({"freeu": {"s1": 0.9}}, net)
    up = VideoUpscalePipeline(net, scheduler=object())
    up.enable_freeu(0.8, 0.3, 1.1, 1.3)
    assert net.freeu == (0.8, 0.3, 1.1, 1.3)
    up.disable_freeu()
    assert net.freeu == (1.0, 1.0, 1.0, 1.0)


def test_entry_points_are_bound():
    from lavie_amd import _lib
    for name in ("lavie_unet_set_freeu", "lavie_freeu_f16", "lavie_freeu_workspace_bytes"):
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "lavie_hip.h")).read()
    assert re.search(r"int lavie_unet_set_freeu\(lavie_unet_t h, float s1, float s2, float b1, float b2\);", header)
    assert re.search(r"#define LAVIE_ABI_VERSION 8\b", header)
    if os.path.isfile(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.lavie_abi_version() == 8
        fake = __import__("ctypes").c_void_p(4096)
        for args, text in (((fake, 24, fake, 32, 1, 2, 2, 1.2, 0.9, fake, fake, fake, None), "C_h=24"),
                           ((fake, 32, fake, 12, 1, 2, 2, 1.2, 0.9, fake, fake, fake, None), "C2=12"),
                           ((fake, 32, fake, 32, 1, 0, 2, 1.2, 0.9, fake, fake, fake, None), "H=0"),
                           ((fake, 32, fake, 32, 1, 2, 2, 0.0, 0.9, fake, fake, fake, None), "finite and > 0"),
                           ((fake, 32, fake, 32, 1, 2, 2, 1.2, float("nan"), fake, fake, fake, None), "finite and > 0"),
                           ((None, 32, fake, 32, 1, 2, 2, 1.2, 0.9, fake, fake, fake, None), "null tensor"),
                           ((fake, 32, fake, 32, 1, 2, 2, 1.2, 0.9, fake, fake, None, None), "workspace")):
            assert lib.lavie_freeu_f16(*args) != 0 and text in lib.lavie_last_error().decode(), (text, lib.lavie_last_error())
        assert lib.lavie_unet_set_freeu(None, 1.0, 1.0, 1.0, 1.0) != 0
        assert lib.lavie_freeu_workspace_bytes(640, 3, 10, 16) == 3 * 2 * 7 * 640 * 4 and lib.lavie_freeu_workspace_bytes(12, 1, 2, 2) == 0


class RecordingLib:
    def __init__(self):
        self.recorded = []

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *args: 64
        return lambda *args: self.recorded.append((name, args)) or 0


@pytest.mark.parametrize("case", [FC.case(3, 10, 16, 1280, 640, 1.6, 0.2, "normal"), FC.case(3, 10, 16, 1280, 640, 1.2, 0.9, "normal", True)],
                         ids=["out-of-place", "in-place"])
def test_call_description_is_what_run_passes(case, monkeypatch):
    from lavie_amd import _lib, ops
    lib = RecordingLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "check", lambda rc, *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_chk16", lambda *ts: None)

    def out_as_given(out, shape, dtype, device, what):
        assert out is not None and tuple(out.shape) == tuple(shape) and out.dtype == dtype, what
        return out
    monkeypatch.setattr(ops, "_out", out_as_given)
    i = case.inputs
    o = {"h_out": i["h"], "skip_out": i["skip"]} if case.in_place else {k: torch.empty(s, dtype=dt) for k, (s, dt) in case.outputs.items()}
    case.run(ops, i, o)
    (name, a), = lib.recorded
    assert name == "lavie_freeu_f16"
    (entry, want), = case.calls
    got = dict(C_h=a[1], C2=a[3], NI=a[4], H=a[5], W=a[6], b_milli=round(a[7] * 1000), s_milli=round(a[8] * 1000),
               in_place=int(a[9].value == a[0].value and a[10].value == a[2].value))
    assert entry == "freeu" and got == want
    assert a[0].value == i["h"].data_ptr() and a[2].value == i["skip"].data_ptr() and a[11] is not None


def test_ops_freeu_checks_its_operands():
    from lavie_amd import ops
    h, skip = torch.zeros(8, 32, dtype=f16), torch.zeros(8, 32, dtype=f16)
    with pytest.raises(ValueError):
        ops.freeu(h, skip, 2, 2, 2, 1.2, 0.9)                 # CPU tensors
