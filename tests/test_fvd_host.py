"""FVD, the parts that need no GPU: the Fréchet distance against the textbook form, its behaviour on singular
covariances, FrechetStats against NumPy, the BatchNorm fold against conv + BN in float64, the state-dict key mapping and its refusals,
the byte round trip of the stock transform's float detour, the bilinear host tables against Pillow, and the C ABI's new symbols."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import r3d_reference as R
from lavie_amd import fvd


def lib():
    from lavie_amd import _lib
    return _lib.load()


def gaussian_sets(dim, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, dim)) @ rng.normal(size=(dim, dim)) * 0.5
    b = rng.normal(size=(n, dim)) @ rng.normal(size=(dim, dim)) * 0.7 + rng.normal(size=dim) * 0.3
    return a, b


def moments(x):
    return x.mean(0), np.cov(x, rowvar=False)


# ------------------------------------------------------------------ the distance
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_frechet_distance_is_the_textbook_form_on_full_rank_cases(seed):
    linalg = pytest.importorskip("scipy.linalg")
    a, b = gaussian_sets(16, 64, seed)
    (m1, s1), (m2, s2) = moments(a), moments(b)
    want = float(((m1 - m2) ** 2).sum() + np.trace(s1 + s2 - 2.0 * linalg.sqrtm(s1 @ s2).real))
    got = fvd.frechet_distance(m1, s1, m2, s2)
    assert abs(got - want) <= 1e-8 * abs(want), (got, want)


@pytest.mark.parametrize("dim,n", [(16, 64), (64, 10)])
def test_identical_sets_are_at_distance_zero_also_when_singular(dim, n):
    a, _ = gaussian_sets(dim, n, 3)
    m, s = moments(a)
    if n < dim:
        assert np.linalg.matrix_rank(s) < dim
    assert abs(fvd.frechet_distance(m, s, m, s)) <= 1e-9 * np.trace(s)


@pytest.mark.parametrize("dim,n", [(16, 64), (64, 10)])
def test_distance_is_symmetric_finite_and_not_negative(dim, n):
    a, b = gaussian_sets(dim, n, 4)
    (m1, s1), (m2, s2) = moments(a), moments(b)
    d12, d21 = fvd.frechet_distance(m1, s1, m2, s2), fvd.frechet_distance(m2, s2, m1, s1)
    assert np.isfinite(d12) and d12 > 0
    assert abs(d12 - d21) <= 1e-9 * abs(d12)


def test_distance_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="do not agree"):
        fvd.frechet_distance(np.zeros(4), np.eye(4), np.zeros(5), np.eye(5))


# ------------------------------------------------------------------ the statistics
def test_frechet_stats_are_numpys_mean_and_cov():
    a, _ = gaussian_sets(24, 50, 5)
    st = fvd.FrechetStats(24).update(torch.from_numpy(a[:20])).update(a[20:])
    assert st.n == 50
    assert np.abs(st.mean - a.mean(0)).max() <= 1e-12
    assert np.abs(st.cov - np.cov(a, rowvar=False)).max() <= 1e-12


def test_merge_equals_one_update_with_all_features():
    a, _ = gaussian_sets(24, 50, 6)
    whole = fvd.FrechetStats(24).update(a)
    parts = fvd.FrechetStats(24).update(a[:13]).merge(fvd.FrechetStats(24).update(a[13:31])).merge(fvd.FrechetStats(24).update(a[31:]))
    assert parts.n == whole.n
    assert np.abs(parts.mean - whole.mean).max() <= 1e-12 and np.abs(parts.cov - whole.cov).max() <= 1e-12
    with pytest.raises(ValueError, match="merging dim"):
        whole.merge(fvd.FrechetStats(8))
    with pytest.raises(ValueError, match="columns"):
        whole.update(np.zeros((2, 8)))


# ------------------------------------------------------------------ the fold
@pytest.mark.parametrize("cin,cout,kernel,stride,pad", [(4, 6, (3, 3, 3), 2, 1), (3, 5, (3, 7, 7), (1, 2, 2), (1, 3, 3)), (4, 6, (1, 1, 1), 2, 0)])
def test_folded_conv_is_conv_then_batchnorm_in_float64(cin, cout, kernel, stride, pad):
    """per element: conv(x, w scale) + shift == BN(conv(x, w)); the fold's own roundings (fp16 weight, fp32 shift) bound the rest"""
    g = torch.Generator().manual_seed(7)
    w = torch.randn(cout, cin, *kernel, generator=g) * 0.2
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    mean, var = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5
    x = torch.randn(2, cin, 4, 9, 10, generator=g).double()
    want = F.batch_norm(F.conv3d(x, w.double(), stride=stride, padding=pad), mean.double(), var.double(), gamma.double(), beta.double(),
                        False, 0.0, fvd.BN_EPS)
    scale = gamma.double() / torch.sqrt(var.double() + fvd.BN_EPS)
    exact_w, exact_b = w.double() * scale.view(-1, 1, 1, 1, 1), beta.double() - mean.double() * scale
    exact = F.conv3d(x, exact_w, stride=stride, padding=pad) + exact_b.view(1, -1, 1, 1, 1)
    assert (exact - want).abs().max() <= 1e-12 * want.abs().max()
    w16, b32 = fvd.fold_batchnorm(w, gamma, beta, mean, var)
    assert w16.dtype == torch.float16 and b32.dtype == torch.float32
    assert torch.equal(w16, exact_w.to(torch.float16)) and torch.equal(b32, exact_b.to(torch.float32))      # one rounding each
    got = F.conv3d(x, w16.double(), stride=stride, padding=pad) + b32.double().view(1, -1, 1, 1, 1)
    bound = 2.0 ** -11 * F.conv3d(x.abs(), exact_w.abs(), stride=stride, padding=pad) + 2.0 ** -24 * exact_b.abs().view(1, -1, 1, 1, 1)
    assert bool(((got - want).abs() <= bound + 1e-12).all())


# ------------------------------------------------------------------ key mapping
@pytest.fixture(scope="module")
def module():
    return R.make_r3d18(seed=0)


def test_both_prefix_styles_map_to_the_same_tensors(module):
    own = fvd.map_state_dict(module.state_dict())
    seq = fvd.map_state_dict(R.sequential_state_dict(module))
    shapes = fvd.r3d18_param_shapes()
    assert set(own) == set(seq) == set(shapes) and len(shapes) == 5 * 20
    assert all(k.startswith(("0.", "1.", "2.", "3.", "4.")) for k in R.sequential_state_dict(module))
    for k in shapes:
        assert own[k].data_ptr() == seq[k].data_ptr() and tuple(own[k].shape) == shapes[k]
    assert not any(k.startswith("fc.") or k.endswith("num_batches_tracked") for k in own)
    assert fvd.canonical_key("0.1.running_var") == "stem.1.running_var"
    assert fvd.canonical_key("3.0.downsample.0.weight") == "layer3.0.downsample.0.weight"


def test_missing_unexpected_and_misshapen_keys_are_refused_by_name(module):
    sd = dict(module.state_dict())
    gone = dict(sd)
    del gone["layer2.0.downsample.1.running_var"]
    with pytest.raises(ValueError, match=r"lacks 'layer2\.0\.downsample\.1\.running_var'"):
        fvd.map_state_dict(gone)
    with pytest.raises(ValueError, match=r"unexpected state-dict key 'layer1\.0\.downsample\.0\.weight'"):
        fvd.map_state_dict({**sd, "layer1.0.downsample.0.weight": torch.zeros(64, 64, 1, 1, 1)})
    with pytest.raises(ValueError, match=r"unexpected state-dict key '5\.0\.conv1\.0\.weight'"):
        fvd.map_state_dict({**sd, "5.0.conv1.0.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match=r"'stem\.0\.weight' has shape \(64, 3, 3, 3, 3\), expected \(64, 3, 3, 7, 7\)"):
        fvd.map_state_dict({**sd, "stem.0.weight": torch.zeros(64, 3, 3, 3, 3)})


# ------------------------------------------------------------------ preprocessing on the host
def test_the_float_detour_of_the_stock_transform_is_the_identity_on_bytes():
    """uint8 -> float / 255 -> ToPILImage's x * 255 -> byte gives every byte back: the device path may start from the bytes"""
    u = torch.arange(256, dtype=torch.uint8)
    back = (u.to(torch.float32) / 255.0).mul(255).byte()
    assert torch.equal(back, u)


def test_centre_offsets_round_half_to_even_as_python():
    assert (R.centre_offset(320, 270), R.centre_offset(512, 270)) == (25, 121)
    assert [R.centre_offset(n, 10) for n in (10, 11, 12, 13, 15, 17)] == [0, 0, 1, 2, 2, 4]


def host_table(n_in, n_out):
    L = lib()
    ks = L.lavie_video_resample_table_host(n_in, n_out, None, None, None)
    assert ks > 0, L.lavie_last_error()
    xmin, count, coeff = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, ks), np.int32)
    ip = C.POINTER(C.c_int)
    assert L.lavie_video_resample_table_host(n_in, n_out, xmin.ctypes.data_as(ip), count.ctypes.data_as(ip), coeff.ctypes.data_as(ip)) == ks
    return xmin, count, coeff


@pytest.mark.parametrize("n_in,n_out", [(270, 224), (34, 28), (224, 224), (17, 40), (500, 31)])
def test_bilinear_host_tables_reproduce_pillow(n_in, n_out):
    from PIL import Image
    xmin, count, coeff = host_table(n_in, n_out)
    assert (xmin >= 0).all() and (count >= 1).all() and (xmin + count <= n_in).all()
    rng = np.random.default_rng(n_in * 1000 + n_out)
    rows = [rng.integers(0, 256, n_in, dtype=np.uint8), (np.arange(n_in) % 2 * 255).astype(np.uint8), np.full(n_in, 255, np.uint8)]
    for row in rows:
        img = np.repeat(row[None, :, None], 3, axis=2)                                # one row: only the horizontal pass resamples
        want = np.asarray(Image.fromarray(np.repeat(img, 2, axis=0)).resize((n_out, 2), Image.BILINEAR))[0, :, 0]
        assert np.array_equal(R.apply_tables(row, xmin, count, coeff), want), (n_in, n_out)


def test_tables_compose_to_pillows_crop_and_resize():
    """both passes from the tables, horizontal first with a byte in between, against Pillow on a cropped frame"""
    from PIL import Image
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, (40, 64, 3), dtype=np.uint8)
    crop, size = 34, 28
    top, left = R.centre_offset(40, crop), R.centre_offset(64, crop)
    want = np.asarray(Image.fromarray(frame).crop((left, top, left + crop, top + crop)).resize((size, size), Image.BILINEAR))
    xmin, count, coeff = host_table(crop, size)
    box = frame[top:top + crop, left:left + crop]
    mid = np.stack([np.stack([R.apply_tables(box[y, :, c], xmin, count, coeff) for c in range(3)], -1) for y in range(crop)])
    got = np.stack([np.stack([R.apply_tables(mid[:, x, c], xmin, count, coeff) for c in range(3)], -1) for x in range(size)], 1)
    assert np.array_equal(got, want)


def test_table_entry_refuses_by_name():
    L = lib()
    assert L.lavie_video_resample_table_host(0, 4, None, None, None) == -1 and b"in=0" in L.lavie_last_error()
    assert L.lavie_video_resample_table_host(400, 4, None, None, None) == -1 and b"above 32" in L.lavie_last_error()
    assert L.lavie_video_preprocess_workspace_bytes(1, 40, 64, 41, 28) == -1 and b"crop=41 is greater than the frame" in L.lavie_last_error()
    assert L.lavie_video_preprocess_workspace_bytes(2, 40, 64, 34, 28) == (2 * 34 * 28 * 3 + 255) // 256 * 256


# ------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ["lavie_conv3d_packed_halfs", "lavie_conv3d_pack", "lavie_conv3d_f16", "lavie_conv3d_stem_f16", "lavie_mean_rows_f32",
               "lavie_r3d_create", "lavie_r3d_destroy", "lavie_r3d_num_params", "lavie_r3d_param_info", "lavie_r3d_set_param",
               "lavie_r3d_finalize", "lavie_r3d_workspace_bytes", "lavie_r3d_features", "lavie_video_resample_table_host",
               "lavie_video_preprocess_workspace_bytes", "lavie_video_preprocess_u8"]


def test_abi_version_is_still_8_and_the_new_symbols_are_bound():
    from lavie_amd import _lib
    L = lib()
    assert _lib.ABI_VERSION == 8 and L.lavie_abi_version() == 8
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "lavie_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1], name
        assert name + "(" in header, name


def test_r3d_handle_lists_the_modules_parameters_and_refuses_on_the_host(module):
    L = lib()
    h = C.c_void_p()
    assert L.lavie_r3d_create(C.byref(h)) == 0
    try:
        names = {}
        for i in range(L.lavie_r3d_num_params(h)):
            name, numel = C.c_char_p(), C.c_longlong()
            assert L.lavie_r3d_param_info(h, i, C.byref(name), C.byref(numel)) == 0
            names[name.value.decode()] = numel.value
        assert names == {k: int(np.prod(v)) for k, v in fvd.r3d18_param_shapes().items()}
        buf = (C.c_float * 64)()
        assert L.lavie_r3d_set_param(h, b"stem.1.weight", buf, 64) == 0
        assert L.lavie_r3d_set_param(h, b"0.1.bias", buf, 64) == 0                       # the numeric prefix
        assert L.lavie_r3d_set_param(h, b"fc.bias", buf, 400) == 0                       # ignored
        assert L.lavie_r3d_set_param(h, b"stem.1.num_batches_tracked", buf, 1) == 0      # ignored
        assert L.lavie_r3d_set_param(h, b"stem.2.weight", buf, 64) != 0 and b"unknown state-dict key 'stem.2.weight'" in L.lavie_last_error()
        assert L.lavie_r3d_set_param(h, b"stem.1.weight", buf, 63) != 0 and b"has 63 elements, expected 64" in L.lavie_last_error()
        assert L.lavie_r3d_set_param(h, b"stem.1.weight", None, 64) != 0 and b"null data" in L.lavie_last_error()
        assert L.lavie_r3d_finalize(h, None) != 0 and b"was never set" in L.lavie_last_error()
        out = (C.c_float * 512)()
        assert L.lavie_r3d_features(h, buf, 1, 48, 16, 16, 1, 1, 4, 4, out, buf, 256, None) != 0 and b"not finalized" in L.lavie_last_error()
        assert L.lavie_r3d_workspace_bytes(h, 1, 0, 4, 4) == -1 and b"T=0" in L.lavie_last_error()
        # x | t of the stem's 1 x 16 x 112 x 112 x 64 halfs, then layer2's 1 x 8 x 56 x 56 x 128
        assert L.lavie_r3d_workspace_bytes(h, 1, 16, 224, 224) == 2 * 16 * 112 * 112 * 64 * 2 + 8 * 56 * 56 * 128 * 2
    finally:
        L.lavie_r3d_destroy(h)
