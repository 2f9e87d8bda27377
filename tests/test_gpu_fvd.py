"""-m gpu: FVD on the engine -- HipR3D18 against the float64 module with the stock fp16 module on the CPU as the
yardstick, batch invariance of the whole model, the video processor bit for bit against Pillow, and FvdScorer end to end."""
import numpy as np
import pytest
import torch

import opcheck as oc
import r3d_reference as R

pytestmark = pytest.mark.gpu

MODEL_SHAPES = [(2, 3, 5, 18, 22), (1, 3, 16, 32, 32)]


@pytest.fixture(scope="module")
def module():
    return R.make_r3d18(seed=0)


@pytest.fixture(scope="module")
def engine(module):
    from lavie_amd.fvd import HipR3D18
    return HipR3D18.from_state_dict(module.state_dict())


@pytest.fixture(scope="module")
def references(module):
    """shape -> (pixels, float64 features, stock fp16 CPU features); made once, never changed"""
    import copy
    out = {}
    for shape in MODEL_SHAPES:
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
        out[shape] = (x, R.features64(copy.deepcopy(module), x), R.features16_cpu(module, x))
    return out


def errors(got, ref64):
    d = got.double() - ref64
    return float(d.abs().max()), float(d.norm() / ref64.norm())


@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=str)
def test_model_is_within_twice_the_stock_fp16_modules_error(engine, references, shape):
    """maximum and relative-L2 error against the float64 module, each at most 2 x that of the same module in fp16 through stock torch.nn
    on the CPU (the margin of DESIGN 7.19, for the different accumulation order); fp32 and fp16 pixels"""
    x, ref64, yard = references[shape]
    y_max, y_l2 = errors(yard, ref64)
    for px in (x.cuda(), x.cuda().half()):
        got = engine(px).cpu()
        assert got.shape == (shape[0], 512) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        e_max, e_l2 = errors(got, ref64)
        print(f"r3d18 {shape} {px.dtype}: engine max {e_max:.3e} rel-L2 {e_l2:.3e}; stock fp16 max {y_max:.3e} rel-L2 {y_l2:.3e}")
        assert e_max <= 2 * y_max and e_l2 <= 2 * y_l2, (e_max, y_max, e_l2, y_l2)


def test_sequential_prefixes_load_the_same_model(module, engine, references):
    from lavie_amd.fvd import HipR3D18
    x = references[MODEL_SHAPES[0]][0].cuda()
    other = HipR3D18.from_stock(torch.nn.Sequential(*list(module.children())[:-1]))
    oc.assert_bits(other(x), engine(x).cpu(), label="numeric prefixes")


def test_clip_of_a_batch_has_the_bits_of_its_single_clip_call(engine):
    x = torch.randn(3, 3, 5, 18, 22, generator=torch.Generator().manual_seed(1)).cuda()
    whole = engine(x)
    oc.assert_bits(engine(x), whole.cpu(), label="two calls")
    for i in range(3):
        oc.assert_bits(engine(x[i:i + 1])[0], whole[i].cpu(), label=f"clip {i}")
    frames_major = x.permute(0, 2, 1, 3, 4).contiguous()
    oc.assert_bits(engine(frames_major, layout="ntchw"), whole.cpu(), label="frames-major pixels")
    oc.assert_bits(engine(frames_major.permute(0, 2, 1, 3, 4)), whole.cpu(), label="a permuted view read in place")


def test_model_refuses_by_name(engine):
    x = torch.randn(1, 3, 2, 8, 8, device="cuda")
    with pytest.raises(ValueError, match="planes of pixels must be contiguous"):
        engine(x[..., ::2])
    with pytest.raises(ValueError, match="fp16 or fp32"):
        engine(x.double())
    with pytest.raises(ValueError, match="3 channels"):
        engine(x[:, :2])
    with pytest.raises(ValueError, match="must be a tensor on"):
        engine(x.cpu())
    from lavie_amd import _lib
    import ctypes
    lib = _lib.load()
    out = torch.empty(1, 512, device="cuda")
    need = lib.lavie_r3d_workspace_bytes(engine._h, 1, 2, 8, 8)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.lavie_r3d_features(engine._h, p(x), 1, 384, 64, 128, 1, 2, 8, 8, p(out), p(ws), need - 1, None) != 0
    assert b"the workspace holds" in lib.lavie_last_error()
    assert lib.lavie_r3d_features(engine._h, p(x), 1, 384, 63, 128, 1, 2, 8, 8, p(out), p(ws), need, None) != 0
    assert b"strides" in lib.lavie_last_error()
    assert lib.lavie_r3d_finalize(engine._h, None) != 0 and b"finalized already" in lib.lavie_last_error()


# ------------------------------------------------------------------ the video processor
def frames(f, h, w, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
    v[0, ::2, :w // 2] = 255             # alternating rows and a flat white area: both clip ends of the resampler
    v[0, 1::2, :w // 2] = 0
    v[-1, :, 3 * w // 4:] = 255
    return v


@pytest.mark.parametrize("f,h,w,crop,size", [(2, 40, 64, 34, 28), (1, 320, 512, 270, 224)])
def test_video_processor_has_pillows_bits(f, h, w, crop, size):
    from lavie_amd import ops
    from lavie_amd.fvd import VideoProcessor
    v = frames(f, h, w, seed=h)
    want = R.pil_video_frames(v, crop, size)
    data = torch.from_numpy(v.reshape(-1).view(np.int32).copy())
    view = lambda t: t.view(torch.uint8).view(f, h, w, 3)
    for dtype, ref in ((torch.float32, want), (torch.float16, want.half())):
        got = oc.run_guarded(lambda i, o: ops.video_preprocess(view(i["px"]), crop, size, dtype=dtype, out=o["y"]), {"px": data},
                             {"y": ((f, 3, size, size), dtype)}, sync=lambda: torch.cuda.synchronize())["y"]
        oc.assert_bits(got, ref, where=oc.loc_nchw(3, size, size), label=f"video_preprocess {dtype} {h}x{w}")
    px = VideoProcessor(crop=crop, size=size)(torch.from_numpy(v))
    assert px.shape == (1, f, 3, size, size)
    oc.assert_bits(px[0], want, label="VideoProcessor")
    if f > 1:
        oc.assert_bits(VideoProcessor(crop=crop, size=size)(v[1:])[0, 0], want[1], label="a frame alone")


def test_video_processor_refuses_by_name():
    from lavie_amd.fvd import VideoProcessor
    proc = VideoProcessor(crop=34, size=28)
    with pytest.raises(ValueError, match="torch.float32 pixels are not built"):
        proc(torch.zeros(2, 40, 64, 3))
    with pytest.raises(ValueError, match="mixed sizes"):
        proc([np.zeros((2, 40, 64, 3), np.uint8), np.zeros((2, 40, 60, 3), np.uint8)])
    with pytest.raises(ValueError, match="crop=34 is greater than the frame 30 x 64"):
        proc(torch.zeros(2, 30, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"must be \[F, H, W, 3\]"):
        proc(torch.zeros(40, 64, 3, dtype=torch.uint8))


# ------------------------------------------------------------------ end to end
def test_fvd_scorer_end_to_end(module, engine):
    """compute() against frechet_distance of the float64 module's features.  The bound follows from the measured feature error:
    the distance is the squared 2-Wasserstein distance W^2 between the Gaussians fitted to the two sets, W obeys the triangle
    inequality, and for two fits to paired rows x_i and x_i + d_i, W^2 <= |mean d|^2 + |centred d|_F^2 / (n - 1) <= E^2 with
    E^2 = sum |d_i|^2 / (n - 1) (the Bures distance of M M^T and N N^T is at most |M - N|_F).  So
    |W_got - W_ref| <= E_real + E_gen =: E and |d_got - d_ref| <= E (2 W_ref + E); a set against itself: d_ref = 0, d_got <= E^2.
    1e-9 tr(S) is allowed on top for the float64 eigen-solver."""
    import copy
    from lavie_amd.fvd import FrechetStats, FvdScorer, VideoProcessor, frechet_distance
    rng = np.random.default_rng(3)
    real = rng.integers(0, 256, (6, 4, 40, 64, 3), dtype=np.uint8)
    gen = (rng.integers(0, 256, (6, 4, 40, 64, 3)) * 0.6 + 40).astype(np.uint8)
    scorer = FvdScorer(engine, VideoProcessor(crop=34, size=28))
    m64 = copy.deepcopy(module)
    stats, err = [], []
    for clips, update in ((real, scorer.update_real), (gen, scorer.update_generated)):
        got = update(torch.from_numpy(clips))
        assert got.shape == (6, 512) and got.dtype == torch.float32
        px = torch.stack([R.pil_video_frames(c, 34, 28) for c in clips]).permute(0, 2, 1, 3, 4)
        ref = R.features64(m64, px)
        stats.append(FrechetStats().update(ref))
        err.append(float(((got.cpu().double() - ref) ** 2).sum().div(5).sqrt()))
    d_got = scorer.compute()
    d_ref = frechet_distance(stats[0].mean, stats[0].cov, stats[1].mean, stats[1].cov)
    slack = 1e-9 * float(np.trace(stats[0].cov) + np.trace(stats[1].cov))
    e = err[0] + err[1]
    print(f"fvd: engine {d_got:.6f}, float64 {d_ref:.6f}, E {e:.3e}, bound {e * (2 * np.sqrt(d_ref) + e):.3e}")
    assert np.isfinite(d_got) and d_got >= 0
    assert abs(d_got - d_ref) <= e * (2 * np.sqrt(d_ref) + e) + slack
    scorer.reset()
    assert scorer.real.n == 0 and scorer.generated.n == 0
    scorer.update_real(torch.from_numpy(real))
    scorer.update_generated(torch.from_numpy(real))
    d_self = scorer.compute()
    assert abs(d_self) <= (2 * err[0]) ** 2 + slack, d_self
    whole = scorer.features(torch.from_numpy(real)).cpu()
    old, FvdScorer.MAX_BATCH = FvdScorer.MAX_BATCH, 2              # the chunking does not change a clip's bits
    try:
        oc.assert_bits(scorer.features(torch.from_numpy(real)), whole, label="chunks of 2")
    finally:
        FvdScorer.MAX_BATCH = old
