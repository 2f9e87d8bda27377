"""-m gpu: engine attention at head dims 512 / 256 (csrc/attention_wide.hip) and the AutoencoderKL mid block on it.

Operator parity is against fp32 softmax(q k^T / sqrt(dh)) v on fp16-quantised inputs (TOL_OP), with q | k | v as column slices
of one fused tensor and q scaled by 4 so the softmax is not flat; the sharp cases force the online-softmax rescale and the
first-tile case of ADVICE.md; the production shape (NB 1, L 163,840, dh 512) is checked on 256 seeded rows and for bit
reproducibility; the VAE wrapper is compared with the stock module and its launches are counted through the profiling hook, so
a silent fallback to stock SDPA fails."""
import ctypes
import warnings

import pytest
import torch

from gpu_util import TOL_OP, h16, q16, rel_l2
from test_gpu_ops import ops  # noqa: F401  (the operator fixture: every GEMM kernel choice)

pytestmark = pytest.mark.gpu

KC_ATTENTION = 2


def gen(seed):
    return torch.Generator().manual_seed(seed)


def attn_ref(q, k, v, heads, kv_div=1):
    """fp32 reference; q [nb, lq, c], k / v [nb / kv_div, lk, c]."""
    nb, lq, c = q.shape
    dh = c // heads
    if kv_div > 1:
        k, v = k.repeat_interleave(kv_div, dim=0), v.repeat_interleave(kv_div, dim=0)
    qh = q.reshape(nb, lq, heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(nb, -1, heads, dh).permute(0, 2, 1, 3)
    vh = v.reshape(nb, -1, heads, dh).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * dh ** -0.5, dim=-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(nb, lq, c)


def fused_qkv(nb, l, c, seed):
    qkv = torch.randn(nb * l, 3 * c, generator=gen(seed))
    qkv[:, :c] *= 4.0
    return q16(qkv)


def run_fused(ops, qkv, nb, l, c, heads):
    d = h16(qkv)
    return ops.attention(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], nb=nb, lq=l, lk=l, heads=heads)


# ------------------------------------------------------------------ operator parity
@pytest.mark.parametrize("nb,l", [(1, 64), (2, 200), (3, 33), (1, 2560), (2, 4100)])
def test_attention_dh512_fused_qkv(ops, nb, l):
    c = 512
    qkv = fused_qkv(nb, l, c, 1000 + l)
    q, k, v = (t.reshape(nb, l, c) for t in qkv.split(c, dim=1))
    ref = attn_ref(q, k, v, 1).reshape(nb * l, c)
    got = run_fused(ops, qkv, nb, l, c, 1)
    err = rel_l2(got, ref)
    print(f"dh512 nb={nb} l={l}: rel-L2 {err:.3e}")
    assert torch.isfinite(got).all()
    assert err < TOL_OP


def test_attention_dh512_two_heads(ops):
    """heads 2: the fused tensor is [M, 3 * 1024], head h at columns 512 h of each slice."""
    nb, l, c = 2, 300, 1024
    qkv = fused_qkv(nb, l, c, 77)
    q, k, v = (t.reshape(nb, l, c) for t in qkv.split(c, dim=1))
    ref = attn_ref(q, k, v, 2).reshape(nb * l, c)
    err = rel_l2(run_fused(ops, qkv, nb, l, c, 2), ref)
    print(f"dh512 heads=2: rel-L2 {err:.3e}")
    assert err < TOL_OP


def test_attention_dh512_cross_kv_batch_div(ops):
    """Lq != Lk, two query batch entries per key / value batch entry; k | v are slices of one tensor, q of another."""
    nbq, lq, lk, c, div = 4, 150, 333, 512, 2
    g = gen(5)
    q = q16(4.0 * torch.randn(nbq, lq, c, generator=g))
    kv = q16(torch.randn(nbq // div, lk, 2 * c, generator=g))
    ref = attn_ref(q, kv[..., :c], kv[..., c:], 1, kv_div=div).reshape(-1, c)
    kvd = h16(kv.reshape(-1, 2 * c))
    got = ops.attention(h16(q.reshape(-1, c)), kvd[:, :c], kvd[:, c:], nb=nbq, lq=lq, lk=lk, heads=1, kv_batch_div=div)
    err = rel_l2(got, ref)
    print(f"dh512 cross kv_batch_div=2: rel-L2 {err:.3e}")
    assert err < TOL_OP


@pytest.mark.parametrize("nb,l", [(2, 200), (1, 2560)])
def test_attention_dh256_fused_qkv(ops, nb, l):
    """the 256-wide instance of the same template"""
    c = 256
    qkv = fused_qkv(nb, l, c, 2000 + l)
    q, k, v = (t.reshape(nb, l, c) for t in qkv.split(c, dim=1))
    ref = attn_ref(q, k, v, 1).reshape(nb * l, c)
    err = rel_l2(run_fused(ops, qkv, nb, l, c, 1), ref)
    print(f"dh256 nb={nb} l={l}: rel-L2 {err:.3e}")
    assert err < TOL_OP


# ------------------------------------------------------------------ sharp softmax
def test_attention_dh512_dominant_key_in_later_tile(ops):
    """one dominant key per chosen query, tiles after the first: the rescale branch (O and l shrink to ~0, then restart)."""
    g = gen(31)
    nb, l, c = 1, 192, 512
    q = 4.0 * torch.randn(nb, l, c, generator=g)
    k = torch.randn(nb, l, c, generator=g)
    k[:, 150] = q[:, 7] * 3.0 / 4.0             # key 150 (fifth 32-key tile) matches query 7
    k[:, 70] = q[:, 130] * 3.0 / 4.0            # key 70 (third tile) matches query 130
    v = torch.randn(nb, l, c, generator=g)
    q, k, v = q16(q), q16(k), q16(v)
    ref = attn_ref(q, k, v, 1).reshape(nb * l, c)
    assert torch.isfinite(ref).all()
    assert (ref[7] - v[0, 150]).abs().max() < 1e-3 and (ref[130] - v[0, 70]).abs().max() < 1e-3     # the keys do dominate
    got = ops.attention(h16(q.reshape(-1, c)), h16(k.reshape(-1, c)), h16(v.reshape(-1, c)), nb=nb, lq=l, lk=l, heads=1)
    err = rel_l2(got, ref)
    print(f"dh512 dominant key: rel-L2 {err:.3e}")
    assert torch.isfinite(got).all()
    assert err < TOL_OP


def test_attention_dh512_first_tile_far_below_zero(ops):
    """for some queries EVERY key of the first tile has logit < -100 nats and the matching key lies in a later
    tile.  A softmax that rescales O and l on its first tile by exp(-max) computes 0 * inf there.  The first 64 keys (two
    32-key tiles) are -2 u + noise, the chosen queries 3 u with u in {-1, +1}^512: logits -6 * 512 / sqrt(512) = -135.8."""
    g = gen(41)
    nb, l, c = 1, 256, 512
    u = torch.randint(0, 2, (c,), generator=g).float() * 2 - 1
    q = 4.0 * torch.randn(nb, l, c, generator=g)
    k = torch.randn(nb, l, c, generator=g)
    v = torch.randn(nb, l, c, generator=g)
    hard = [5, 40, 77, 200]
    q[0, hard] = 3.0 * u
    k[0, :64] = -2.0 * u + 0.1 * torch.randn(64, c, generator=g)
    k[0, 150] = u                                 # logit +67.9 for the chosen queries
    q, k, v = q16(q), q16(k), q16(v)
    logits = (q[0, hard] @ k[0].T) * c ** -0.5
    assert logits[:, :64].max() < -100.0 and logits[:, 150].min() > 60.0
    ref = attn_ref(q, k, v, 1).reshape(nb * l, c)
    assert torch.isfinite(ref).all()
    got = ops.attention(h16(q.reshape(-1, c)), h16(k.reshape(-1, c)), h16(v.reshape(-1, c)), nb=nb, lq=l, lk=l, heads=1)
    err = rel_l2(got, ref)
    err_hard = rel_l2(got[hard], ref[hard])
    print(f"dh512 first tile < -100 nats: rel-L2 {err:.3e}, chosen rows {err_hard:.3e}")
    assert torch.isfinite(got).all()
    assert err < TOL_OP and err_hard < TOL_OP


# ------------------------------------------------------------------ production shape
def test_attention_dh512_production_shape(ops):
    """The VSR VAE's mid block on one 320x512 latent frame: NB 1, L 163,840, one 512-wide head.  256 seeded query rows
    against the reference computed for those rows only (fp64 on the device, from the same fp16 values); two runs bit-equal."""
    l, c = 163840, 512
    g = torch.Generator(device="cuda").manual_seed(9)
    qkv = torch.randn(l, 3 * c, generator=g, device="cuda")
    qkv[:, :c] *= 4.0
    d = qkv.to(torch.float16)
    del qkv
    got = ops.attention(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], nb=1, lq=l, lk=l, heads=1)
    again = ops.attention(d[:, :c], d[:, c:2 * c], d[:, 2 * c:], nb=1, lq=l, lk=l, heads=1)
    assert torch.equal(got, again)
    rows = torch.randperm(l, generator=gen(10))[:256].cuda()
    qs = d[rows, :c].double()
    p = torch.softmax(qs @ d[:, c:2 * c].double().T * c ** -0.5, dim=-1)
    ref = p @ d[:, 2 * c:].double()
    err = rel_l2(got[rows], ref)
    print(f"dh512 production shape, 256 rows: rel-L2 {err:.3e}")
    assert torch.isfinite(got).all()
    assert err < TOL_OP


# ------------------------------------------------------------------ the VAE on it
def counted(fn):
    """fn() with the attention class counted -> (result, launches of class 2)"""
    import bench
    from lavie_amd import _lib
    lib = _lib.load()
    bench.profile_begin(lib, 1 << KC_ATTENTION, 64)
    y = fn()
    rows = bench.profile_end(lib)
    return y, rows[KC_ATTENTION]["launches"]


@pytest.mark.parametrize("widths,size", [((128, 256, 512, 512), (2, 8, 16)), ((128, 256, 512), (1, 16, 24))])
def test_hip_vae_decoder_engine_attention(widths, size):
    from lavie_amd.autoencoder_kl import AutoencoderKL
    from lavie_amd.vae_hip import HipAutoencoderKL
    torch.manual_seed(3)
    vae = AutoencoderKL(block_out_channels=widths).cuda().eval()
    n, h, w = size
    z = torch.randn(n, 4, h, w, device="cuda")
    ref = vae.decode(z).sample
    got, launches = counted(lambda: HipAutoencoderKL(vae, attention="engine").decode(z).sample)
    err = ((got.float() - ref).norm() / ref.norm()).item()
    print(f"decode {widths}: rel-L2 {err:.3e}, engine attention launches {launches}")
    assert launches == 1
    assert err < 1e-2
    got2, launches2 = counted(lambda: HipAutoencoderKL(vae, attention="sdpa").decode(z).sample)
    assert launches2 == 0
    assert ((got2.float() - ref).norm() / ref.norm()).item() < 1e-2


def test_hip_vae_encoder_engine_attention():
    from lavie_amd.autoencoder_kl import AutoencoderKL
    from lavie_amd.vae_hip import HipAutoencoderKL
    torch.manual_seed(5)
    vae = AutoencoderKL().cuda().eval()
    x = torch.rand(2, 3, 64, 96, device="cuda") * 2 - 1
    ref = vae.encode(x).latent_dist
    got, launches = counted(lambda: HipAutoencoderKL(vae, attention="engine").encode(x).latent_dist)
    assert launches == 1
    assert ((got.mean - ref.mean).norm() / ref.mean.norm()).item() < 1e-2
    assert ((got.logvar - ref.logvar).norm() / ref.logvar.norm()).item() < 1e-2
    _, launches2 = counted(lambda: HipAutoencoderKL(vae, attention="sdpa").encode(x).latent_dist)
    assert launches2 == 0


def test_hip_vae_unserved_mid_width_falls_back_and_warns():
    """mid width 384: no engine attention at that head dim; "engine" mode decodes through SDPA and says so once."""
    from lavie_amd.autoencoder_kl import AutoencoderKL
    from lavie_amd.vae_hip import HipAutoencoderKL
    torch.manual_seed(7)
    vae = AutoencoderKL(block_out_channels=(128, 384)).cuda().eval()
    z = torch.randn(1, 4, 8, 12, device="cuda")
    ref = vae.decode(z).sample
    hip = HipAutoencoderKL(vae, attention="engine")
    with pytest.warns(UserWarning, match="384"):
        got, launches = counted(lambda: hip.decode(z).sample)
    assert launches == 0
    assert ((got.float() - ref).norm() / ref.norm()).item() < 1e-2
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # one-time: the second decode is silent
        hip.decode(z)
    with pytest.raises(ValueError):
        HipAutoencoderKL(vae, attention="flash")


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dh", [168, 520])
def test_attention_refuses_unsupported_head_dims(dh):
    from lavie_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, 3 * dh, dtype=torch.float16, device="cuda")
    o = torch.zeros(64, dh, dtype=torch.float16, device="cuda")
    vp = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 2 * off)
    rc = lib.lavie_attention_f16(vp(x), 3 * dh, vp(x, dh), 3 * dh, vp(x, 2 * dh), 3 * dh, vp(o), dh, 1, 64, 64, 1, dh, 1,
                                 ctypes.c_float(dh ** -0.5), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0
    msg = lib.lavie_last_error().decode()
    assert f"head dim {dh}" in msg and "160" in msg and "256" in msg and "512" in msg
