"""Operator-level entry points (the finer seam of SURVEY.md §8b) over the C ABI.

All tensors are CUDA(HIP) fp16, channels-last: a reference video tensor `[b, c, f, h, w]` is the
row-major matrix `[(b f h w), c]`, which is also the reference's token layout `(b f) (h w) c`.
Every function enqueues on torch's current stream and raises RuntimeError on failure."""
import ctypes
import math
from typing import Optional

import torch

from . import _lib
from .noise import NoiseKey


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk16(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()):
            raise ValueError("expected contiguous fp16 device tensors")


def _chk32(*ts):
    for t in ts:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("expected contiguous fp32 device tensors")


def _chk_cols16(*ts):
    """attention operands: column slices of wider row-major tensors are taken"""
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float16 and t.stride(1) == 1):
            raise ValueError("attention operands must be fp16 device tensors with unit column stride")


def _out(out, shape, dtype, device, what):
    """The caller's output tensor after the checks every `out=` gets (device, dtype, contiguity, exact shape), or a new one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (out.is_cuda and out.device == device and out.dtype == dtype and out.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous {dtype} tensor on {device}")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(out.shape)}")
    return out


def to_rows(x: torch.Tensor) -> torch.Tensor:
    """[b, c, f, h, w] -> channels-last rows [(b f h w), c] (a copy)."""
    b, c, f, h, w = x.shape
    return x.permute(0, 2, 3, 4, 1).reshape(b * f * h * w, c).contiguous()


def from_rows(rows: torch.Tensor, b: int, f: int, h: int, w: int) -> torch.Tensor:
    """channels-last rows [(b f h w), c] -> [b, c, f, h, w] (a copy)."""
    return rows.reshape(b, f, h, w, -1).permute(0, 4, 1, 2, 3).contiguous()


def linear(a, weight, bias=None, residual=None, bias2=None, rows_per_batch=0, geglu=False, out=None):
    """a[M,K] @ weight[N,K]^T (+bias fp32[N]) (+bias2 fp32[M/rows_per_batch, N]) (+residual[M,N])."""
    _chk16(a, weight, residual, out)
    _chk32(bias, bias2)
    M, K = a.shape
    N = weight.shape[0]
    n_out = N // 2 if geglu else N
    out = _out(out, (M, n_out), torch.float16, a.device, "linear: out")
    lib = _lib.load()
    _lib.check(lib.lavie_linear_f16(_p(a), K, _p(weight), _p(bias), _p(bias2), N, rows_per_batch, _p(residual), n_out,
                                    _p(out), n_out, M, N, K, int(geglu), _stream()), "lavie_linear_f16")
    return out


def _rows16(t, rows, cols, what):
    """leading dimension of a [rows, cols] fp16 operand that may be a column block of a wider row-major buffer"""
    if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1):
        raise ValueError(f"{what} must be a 2-D fp16 device tensor with unit column stride")
    if tuple(t.shape) != (rows, cols):
        raise ValueError(f"{what} must have shape {(rows, cols)}, got {tuple(t.shape)}")
    if t.stride(0) < cols:
        raise ValueError(f"{what}: rows {t.stride(0)} halfs apart overlap at {cols} columns")
    return t.stride(0)


def pinned_linear(a, weight, bias, residual=None, out=None):
    """a[M,K] @ weight[N,K]^T + bias fp32[N] (+ residual[M,N]) on the encoders' pinned plan (lavie_pinned_linear_f16): no planner, the
    same kernel and summation order at every M.  a, residual and out may be column blocks of wider buffers (unit column stride, any row
    stride); residual may be out itself."""
    _chk16(weight)
    _chk32(bias)
    if weight.dim() != 2 or a.dim() != 2 or bias is None or bias.numel() != weight.shape[0]:
        raise ValueError("pinned_linear: a must be [M, K], weight [N, K] and bias fp32 [N]")
    M, (N, K) = a.shape[0], weight.shape
    lda = _rows16(a, M, K, "pinned_linear: a")
    ldr = N if residual is None else _rows16(residual, M, N, "pinned_linear: residual")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=a.device)
    ldc = _rows16(out, M, N, "pinned_linear: out")
    _lib.check(_lib.load().lavie_pinned_linear_f16(_p(a), lda, _p(weight), _p(bias), _p(residual), ldr, _p(out), ldc, M, N, K, _stream()),
               "lavie_pinned_linear_f16")
    return out


def add_rows(x, pos, out=None):
    """fp16(float(x [b, l, c]) + float(pos [l, c])), one rounding (lavie_add_rows_f16): the mapper's target rows plus their positions."""
    _chk16(x, pos)
    if x.dim() != 3 or pos.dim() != 2 or tuple(pos.shape) != tuple(x.shape[1:]):
        raise ValueError(f"add_rows: x must be [b, l, c] and pos [l, c], got {tuple(x.shape)} and {tuple(pos.shape)}")
    b, l, c = x.shape
    out = _out(out, x.shape, torch.float16, x.device, "add_rows: out")
    _lib.check(_lib.load().lavie_add_rows_f16(_p(x), _p(pos), _p(out), b, l, c, _stream()), "lavie_add_rows_f16")
    return out


def linear_lnfold(a, weight_folded, bias, ln_s, ln_stats, geglu=False, out=None):
    """rstd_m (a @ weight_folded^T - mean_m ln_s) + bias: a projection behind a LayerNorm, the norm folded into the GEMM epilogue
    (weight_folded = W * gamma, ln_s = its row sums, bias = W beta (+ b), ln_stats [M, 2] = (mean, rstd) of the rows of `a`).
    geglu: h * gelu(gate) of that, [M, N / 2]; weight_folded, bias and ln_s in pack_geglu's row order."""
    _chk16(a, weight_folded, out)
    _chk32(bias, ln_s, ln_stats)
    M, K = a.shape
    N = weight_folded.shape[0]
    n_out = N // 2 if geglu else N
    out = _out(out, (M, n_out), torch.float16, a.device, "linear_lnfold: out")
    name = "lavie_linear_lnfold_geglu_f16" if geglu else "lavie_linear_lnfold_f16"
    _lib.check(getattr(_lib.load(), name)(_p(a), _p(weight_folded), _p(bias), _p(ln_s), _p(ln_stats), _p(out), M, N, K, _stream()), name)
    return out


def pack_geglu(weight, bias):
    """GEGLU projection [2*inner, K] -> the value/gate 16-row interleave the geglu epilogue expects."""
    _chk16(weight, bias)
    N, K = weight.shape
    w_out = torch.empty_like(weight)
    b_out = torch.empty(N, dtype=torch.float32, device=weight.device)
    _lib.check(_lib.load().lavie_pack_geglu_f16(_p(weight), _p(bias), _p(w_out), _p(b_out), N, K, _stream()))
    return w_out, b_out


def pack_geglu_mlp(w1, b1, w2):
    """ff.net.0.proj.weight [8C, C], .bias [8C], ff.net.2.weight [C, 4C] (fp16, device) -> (image, bias image) of the fused
    feed-forward kernel (lavie_geglu_mlp_f16).  Raises for a width the kernel is not built for."""
    _chk16(w1, b1, w2)
    C = w2.shape[0]
    lib = _lib.load()
    nbytes = lib.lavie_geglu_mlp_image_bytes(C)
    if nbytes == 0 or tuple(w1.shape) != (8 * C, C) or tuple(w2.shape) != (C, 4 * C):
        raise RuntimeError(f"geglu_mlp: width {C} is not built (or weight shapes do not match)")
    img = torch.empty(nbytes // 2, dtype=torch.float16, device=w1.device)
    b1img = torch.empty(lib.lavie_geglu_mlp_bias_floats(C), dtype=torch.float32, device=w1.device)
    _lib.check(lib.lavie_pack_geglu_mlp_f16(_p(w1), _p(b1), _p(w2), C, _p(img), _p(b1img), _stream()), "lavie_pack_geglu_mlp_f16")
    return img, b1img


def geglu_mlp(x, img, b1img, gamma, beta, b2, eps=1e-5, out=None):
    """x + FeedForward_GEGLU(LayerNorm(x)) in one kernel (attention.py:558); `out` may be x itself."""
    _chk16(x, img, out)
    _chk32(b1img, gamma, beta, b2)
    M, C = x.shape
    out = _out(out, x.shape, torch.float16, x.device, "geglu_mlp: out")
    _lib.check(_lib.load().lavie_geglu_mlp_f16(_p(x), _p(out), M, C, _p(img), _p(b1img), _p(gamma), _p(beta), _p(b2), eps,
                                               _stream()), "lavie_geglu_mlp_f16")
    return out


def pack_temporal_block(wq, wk, wv, wo, heads=8, frames=16, rot_dim=32):
    """attn_temp.to_q / to_k / to_v / to_out.0 weights [C, C] (fp16, device) -> the weight image of the fused temporal
    sub-block kernel (lavie_temporal_block_f16).  Raises for a configuration the kernel is not built for."""
    _chk16(wq, wk, wv, wo)
    C = wq.shape[0]
    lib = _lib.load()
    nbytes = lib.lavie_temporal_block_image_bytes(C, heads, frames, rot_dim)
    if nbytes == 0:
        raise RuntimeError(f"temporal_block: C={C} heads={heads} frames={frames} rot_dim={rot_dim} is not built")
    img = torch.empty(nbytes // 2, dtype=torch.float16, device=wq.device)
    _lib.check(lib.lavie_pack_temporal_block_f16(_p(wq), _p(wk), _p(wv), _p(wo), C, _p(img), _stream()), "lavie_pack_temporal_block_f16")
    return img


def temporal_block(x, img, gamma, beta, bo, relbias, rot_cos, rot_sin, B, F, D, heads, rot_dim, scale, eps=1e-5, out=None):
    """x + to_out(attn_temp(norm_temp(x))) on token rows [(b f) d, C] in one kernel (attention.py:548-555, 580-667)."""
    _chk16(x, img, out)
    _chk32(gamma, beta, bo, relbias, rot_cos, rot_sin)
    C = x.shape[1]
    out = _out(out, x.shape, torch.float16, x.device, "temporal_block: out")
    _lib.check(_lib.load().lavie_temporal_block_f16(_p(x), _p(out), B, F, D, C, heads, _p(img), _p(gamma), _p(beta), _p(bo),
                                                    _p(relbias), _p(rot_cos), _p(rot_sin), rot_dim, scale, eps, _stream()),
               "lavie_temporal_block_f16")
    return out


# The fused text cross-attention has two variants with images of their own layout (<= 80 keys, and `_long`: 81..160 keys); `name` is
# the variant's prefix in the C entry points and in the messages
def _pack_cross_block(name, wo1, wq2, wo2, heads):
    _chk16(wo1, wq2, wo2)
    C = wo1.shape[0]
    lib = _lib.load()
    nbytes = getattr(lib, f"lavie_{name}_image_bytes")(C, heads)
    if nbytes == 0:
        raise RuntimeError(f"{name}: C={C} heads={heads} is not built")
    tmpl = torch.empty(nbytes // 2, dtype=torch.float16, device=wo1.device)
    _lib.check(getattr(lib, f"lavie_pack_{name}_f16")(_p(wo1), _p(wq2), _p(wo2), C, _p(tmpl), _stream()), f"lavie_pack_{name}_f16")
    return tmpl


def _bind_cross_block(name, tmpl, kv, B, ctx_len):
    _chk16(tmpl, kv)
    C = kv.shape[1] // 2
    if tuple(kv.shape) != (B * ctx_len, 2 * C):
        raise RuntimeError(f"{name}: kv must be [B * ctx_len, 2C]")
    img = torch.empty(B * tmpl.numel(), dtype=torch.float16, device=tmpl.device)
    _lib.check(getattr(_lib.load(), f"lavie_bind_{name}_f16")(_p(tmpl), _p(kv), B, ctx_len, C, _p(img), _stream()), f"lavie_bind_{name}_f16")
    return img


def _cross_block(name, att, x, img, bo1, gamma, beta, bo2, rows_per_batch, ctx_len, heads, scale, eps, out):
    _chk16(att, x, img, out)
    _chk32(bo1, gamma, beta, bo2)
    M, C = x.shape
    out = _out(out, x.shape, torch.float16, x.device, f"{name}: out")
    _lib.check(getattr(_lib.load(), f"lavie_{name}_f16")(_p(att), _p(x), _p(out), M, rows_per_batch, C, heads, _p(img), _p(bo1), _p(gamma),
                                                         _p(beta), _p(bo2), ctx_len, scale, eps, _stream()), f"lavie_{name}_f16")
    return out


def pack_cross_block(wo1, wq2, wo2, heads=8):
    """attn1.to_out.0 / attn2.to_q / attn2.to_out.0 weights [C, C] (fp16, device) -> the weight part of the image of the fused
    text cross-attention kernel (lavie_cross_block_f16).  Raises for a configuration the kernel is not built for."""
    return _pack_cross_block("cross_block", wo1, wq2, wo2, heads)


def bind_cross_block(tmpl, kv, B, ctx_len):
    """Completes one image per video from kv [B * ctx_len, 2C] (attn2.to_k | to_v of the text context): once per context."""
    return _bind_cross_block("cross_block", tmpl, kv, B, ctx_len)


def cross_block(att, x, img, bo1, gamma, beta, bo2, rows_per_batch, ctx_len, heads, scale, eps=1e-5, out=None):
    """x + to_out1(att), then + to_out2(attn2(norm2(.), K, V)) in one kernel (attention.py:513-534); `out` may be x itself."""
    return _cross_block("cross_block", att, x, img, bo1, gamma, beta, bo2, rows_per_batch, ctx_len, heads, scale, eps, out)


def pack_cross_block_long(wo1, wq2, wo2, heads=8):
    """As pack_cross_block, for the long variant (81..160 keys, lavie_cross_block_long_f16): its own template layout."""
    return _pack_cross_block("cross_block_long", wo1, wq2, wo2, heads)


def bind_cross_block_long(tmpl, kv, B, ctx_len):
    """As bind_cross_block, for a long template and 81 <= ctx_len <= 160."""
    return _bind_cross_block("cross_block_long", tmpl, kv, B, ctx_len)


def cross_block_long(att, x, img, bo1, gamma, beta, bo2, rows_per_batch, ctx_len, heads, scale, eps=1e-5, out=None):
    """cross_block over 81..160 keys with long images (bind_cross_block_long); `out` may be x itself."""
    return _cross_block("cross_block_long", att, x, img, bo1, gamma, beta, bo2, rows_per_batch, ctx_len, heads, scale, eps, out)


def pack_conv3x3(weight, shortcut_weight=None):
    """[Cout, Cin, 3, 3] (+ optional 1x1 shortcut [Cout, Csc, 1, 1]) -> [Cout, 9*Cin (+ Csc)]."""
    _chk16(weight, shortcut_weight)
    cout, cin = weight.shape[:2]
    csc = 0 if shortcut_weight is None else shortcut_weight.shape[1]
    ld = 9 * cin + csc
    out = torch.empty(cout, ld, dtype=torch.float16, device=weight.device)
    _lib.check(_lib.load().lavie_pack_conv3x3_f16(_p(weight), _p(out), cout, cin, ld, 0, _stream()))
    if csc:
        out[:, 9 * cin:] = shortcut_weight.reshape(cout, csc)
    return out


_zero_pages = {}


def _zero_page(device):
    z = _zero_pages.get(device)
    if z is None:
        z = torch.zeros(256, dtype=torch.float16, device=device)
        _zero_pages[device] = z
    return z


def conv3x3(x1, wp, bias, ni, hi, wi, x2=None, sc1=None, sc2=None, bias2=None, rows_per_batch=0, residual=None,
            stride=1, ups=0, pad=None, out=None):
    """Per-frame 3x3 conv, pad 1, on channels-last rows [(ni hi wi), C]; see lavie_conv3x3_f16.
    pad = (lo, hi) chooses the padding instead: (1, 1) is the default geometry, (0, 1) with stride 2 the far-side pad of the
    AutoencoderKL downsampler (lavie_conv3x3_down_f16: one source, no shortcut / residual / bias2)."""
    _chk16(x1, x2, sc1, sc2, wp, residual)
    _chk32(bias, bias2)
    cout = wp.shape[0]
    if pad is not None:
        if tuple(pad) not in ((0, 1), (1, 1)):
            raise ValueError(f"conv3x3: pad must be (0, 1) or (1, 1), got {pad!r}")
        if any(t is not None for t in (x2, sc1, sc2, bias2, residual)) or ups:
            raise ValueError("conv3x3: pad= takes one source and no shortcut, residual, bias2 or upsample")
        lo = pad[0]
        ho, wo = (hi - 2 + lo) // stride + 1, (wi - 2 + lo) // stride + 1
        y = _out(out, (ni * max(ho, 0) * max(wo, 0), cout), torch.float16, x1.device, "conv3x3: out")
        _lib.check(_lib.load().lavie_conv3x3_down_f16(_p(x1), x1.shape[1], _p(wp), _p(bias), _p(y), ni, hi, wi, cout, stride, lo,
                                                      _p(_zero_page(x1.device)), _stream()), "lavie_conv3x3_down_f16")
        return y
    ho = hi * 2 if ups else (hi - 1) // stride + 1
    wo = wi * 2 if ups else (wi - 1) // stride + 1
    y = _out(out, (ni * ho * wo, cout), torch.float16, x1.device, "conv3x3: out")
    c = lambda t: 0 if t is None else t.shape[1]
    lib = _lib.load()
    _lib.check(lib.lavie_conv3x3_f16(_p(x1), c(x1), _p(x2), c(x2), _p(sc1), c(sc1), _p(sc2), c(sc2), _p(wp), _p(bias),
                                     _p(bias2), cout, rows_per_batch, _p(residual), _p(y), ni, hi, wi, cout, stride, ups,
                                     _p(_zero_page(x1.device)), _stream()), "lavie_conv3x3_f16")
    return y


def _edge_dtype(t, what):
    if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.float16, torch.float32)):
        raise ValueError(f"{what} must be a contiguous fp16 or fp32 device tensor")
    return 1 if t.dtype == torch.float32 else 0


def pack_conv_edge_in(weight):
    """[Cout, Cin <= 8, 3, 3] (fp16, device) -> the weight image of conv_edge_in (channel pairs interleaved, an odd Cin zero-padded)."""
    _chk16(weight)
    cout, cin = weight.shape[:2]
    out = torch.empty(9 * (cin + (cin & 1)) * cout, dtype=torch.float16, device=weight.device)
    _lib.check(_lib.load().lavie_pack_conv_edge_in_f16(_p(weight), _p(out), cout, cin, _stream()), "lavie_pack_conv_edge_in_f16")
    return out


def conv_edge_in(x, wp, bias, cout, tap_bias=None, out=None):
    """3x3 conv, pad 1, from an NCHW image x [n, cin <= 8, h, w] (fp16 or fp32, read in place) to channels-last fp16 rows
    [(n h w), cout]; tap_bias fp32 [9, cout] is added for the taps inside the image; see lavie_conv_edge_in_f16."""
    _chk16(wp)
    _chk32(bias, tap_bias)
    flag = _edge_dtype(x, "conv_edge_in: x")
    n, cin, h, w = x.shape
    if 1 <= cin <= 8 and cout % 8 == 0 and wp.numel() != 9 * (cin + (cin & 1)) * cout:      # (other counts: the library refuses them)
        raise ValueError(f"conv_edge_in: wp has {wp.numel()} halfs, not the pack_conv_edge_in image of Cin={cin} Cout={cout}")
    if (bias is not None and bias.numel() != cout) or (tap_bias is not None and tuple(tap_bias.shape) != (9, cout)):
        raise ValueError(f"conv_edge_in: bias must be [{cout}] and tap_bias [9, {cout}]")
    y = _out(out, (n * h * w, cout), torch.float16, x.device, "conv_edge_in: out")
    _lib.check(_lib.load().lavie_conv_edge_in_f16(_p(x), flag, _p(wp), _p(bias), _p(tap_bias), _p(y), n, cin, h, w, cout, _stream()),
               "lavie_conv_edge_in_f16")
    return y


def pack_conv_edge_out(weight):
    """[Cout <= 8, Cin, 3, 3] (fp16, device) -> the weight image of conv_edge_out (MFMA fragment order, rows padded to 8)."""
    _chk16(weight)
    cout, cin = weight.shape[:2]
    lib = _lib.load()
    out = torch.empty(max(lib.lavie_conv_edge_out_image_halfs(cin), 8), dtype=torch.float16, device=weight.device)
    _lib.check(lib.lavie_pack_conv_edge_out_f16(_p(weight), _p(out), cout, cin, _stream()), "lavie_pack_conv_edge_out_f16")
    return out


def conv_edge_out(x, wp, bias, n, h, w, cout, out_dtype=torch.float16, out=None):
    """3x3 conv, pad 1, from channels-last fp16 rows x [(n h w), cin] to an NCHW image [n, cout <= 8, h, w] written in `out_dtype`
    (fp16 or fp32) from fp32 accumulators; see lavie_conv_edge_out_f16."""
    _chk16(x, wp)
    _chk32(bias)
    if out_dtype not in (torch.float16, torch.float32):
        raise ValueError("conv_edge_out: out_dtype must be torch.float16 or torch.float32")
    if x.dim() != 2 or x.shape[0] != n * h * w:
        raise ValueError(f"conv_edge_out: x must be [{n * h * w}, cin] rows, got {tuple(x.shape)}")
    halfs = _lib.load().lavie_conv_edge_out_image_halfs(x.shape[1])
    if halfs and wp.numel() != halfs:                                                        # (halfs == 0: the library refuses Cin)
        raise ValueError(f"conv_edge_out: wp has {wp.numel()} halfs, not the pack_conv_edge_out image of Cin={x.shape[1]} ({halfs})")
    if bias is not None and bias.numel() != cout:
        raise ValueError(f"conv_edge_out: bias must be [{cout}]")
    y = _out(out, (n, cout, h, w), out_dtype, x.device, "conv_edge_out: out")
    _lib.check(_lib.load().lavie_conv_edge_out_f16(_p(x), _p(wp), _p(bias), _p(y), 1 if out_dtype == torch.float32 else 0, n,
                                                   x.shape[1], h, w, cout, _stream()), "lavie_conv_edge_out_f16")
    return y


def pack_conv3x3_parity(weight):
    """[C, C, 3, 3] (fp16, device) -> the four parity weight sets [4, C, 4C] of the upsample conv (lavie_upsample_conv3x3_f16)."""
    _chk16(weight)
    cout, cin = weight.shape[0], weight.shape[1]
    out = torch.empty(4, cout, 4 * cin, dtype=torch.float16, device=weight.device)
    _lib.check(_lib.load().lavie_pack_conv3x3_parity_f16(_p(weight.contiguous()), _p(out), cout, cin, _stream()), "lavie_pack_conv3x3_parity_f16")
    return out


def upsample_conv3x3(x, wpar, bias, ni, hi, wi, out=None):
    """conv3x3(nearest_x2(x)) + bias (Upsample3D, resnet.py:44-79) in parity form: x [ni*hi*wi, C] rows -> [ni*2hi*2wi, C] rows.
    Raises where the kernel's geometry does not hold (use conv3x3(..., ups=1) there)."""
    _chk16(x, wpar)
    _chk32(bias)
    c = x.shape[1]
    y = _out(out, (ni * 4 * hi * wi, c), torch.float16, x.device, "upsample_conv3x3: out")
    _lib.check(_lib.load().lavie_upsample_conv3x3_f16(_p(x), _p(wpar), _p(bias), _p(y), ni, hi, wi, c, _p(_zero_page(x.device)), _stream()),
               "lavie_upsample_conv3x3_f16")
    return y


def pack_temporal_conv(weight):
    """nn.Conv3d weight [Cout, Cin, T, 1, 1] (T = 3 or 5) -> [Cout, T*Cin] in the implicit GEMM's K order."""
    _chk16(weight)
    cout, cin, taps = weight.shape[:3]
    out = torch.empty(cout, taps * cin, dtype=torch.float16, device=weight.device)
    _lib.check(_lib.load().lavie_pack_temporal_conv_f16(_p(weight.contiguous()), _p(out), cout, cin, taps, _stream()),
               "lavie_pack_temporal_conv_f16")
    return out


def temporal_conv(x, wp, bias, b, frames, d, taps, bias2=None, residual=None, out=None):
    """Conv3d (taps, 1, 1), padding (taps // 2, 0, 0), over the frame axis of token rows [(b f d), C] (the VSR stage's
    ResnetBlock3DCNN convs); bias2 [b, Cout] = per-video time-embedding projection; see lavie_temporal_conv_f16."""
    _chk16(x, wp, residual)
    _chk32(bias, bias2)
    cout = wp.shape[0]
    y = _out(out, (b * frames * d, cout), torch.float16, x.device, "temporal_conv: out")
    _lib.check(_lib.load().lavie_temporal_conv_f16(_p(x), x.shape[1], _p(wp), _p(bias), _p(bias2), cout,
                                                   frames * d if bias2 is not None else 0, _p(residual), _p(y), b, frames, d,
                                                   cout, taps, _p(_zero_page(x.device)), _stream()),
               "lavie_temporal_conv_f16")
    return y


def group_norm(x1, gamma, beta, nb, groups, eps, silu, x2=None, out=None):
    """GroupNorm (+SiLU) over rows; `nb` batches share statistics over rows/nb rows each."""
    _chk16(x1, x2)
    _chk32(gamma, beta)
    rows = x1.shape[0]
    c1, c2 = x1.shape[1], 0 if x2 is None else x2.shape[1]
    y = _out(out, (rows, c1 + c2), torch.float16, x1.device, "group_norm: out")
    ws = torch.empty(_lib.load().lavie_group_norm_ws_floats(nb, groups), dtype=torch.float32, device=x1.device)
    _lib.check(_lib.load().lavie_group_norm_f16(_p(x1), c1, _p(x2), c2, nb, rows // nb, groups, _p(gamma), _p(beta),
                                                float(eps), int(silu), _p(ws), _p(y), _stream()), "lavie_group_norm_f16")
    return y


class op_statistics:
    """The statistics sink of the operator-level GEMM entry points (lavie_debug_op_statistics) for the duration of a `with` block:
    colstat / rowstat are fp32 device buffers (either may be None) that the launches inside write the producers' column / row
    statistics to.  plan=(colstat, rowstat) instead: launches inside are planned as if those kinds were armed and NOT run
    (lavie_debug_op_statistics_plan), to size the buffers from last()."""

    def __init__(self, colstat=None, rowstat=None, plan=None):
        _chk32(colstat, rowstat)
        self.colstat, self.rowstat, self.plan = colstat, rowstat, plan

    def __enter__(self):
        lib = _lib.load()
        if self.plan is not None:
            _lib.check(lib.lavie_debug_op_statistics_plan(int(self.plan[0]), int(self.plan[1])), "lavie_debug_op_statistics_plan")
        else:
            _lib.check(lib.lavie_debug_op_statistics(_p(self.colstat), 0 if self.colstat is None else self.colstat.numel(), _p(self.rowstat),
                                                     0 if self.rowstat is None else self.rowstat.numel()), "lavie_debug_op_statistics")
        return self

    def __exit__(self, *exc):
        lib = _lib.load()
        lib.lavie_debug_op_statistics_plan(0, 0)
        lib.lavie_debug_op_statistics(None, 0, None, 0)

    @staticmethod
    def last():
        """lavie_op_statistics_info of the last operator-level GEMM launch, as a dict"""
        info = _lib.OpStatisticsInfoC()
        info.struct_size = ctypes.sizeof(info)
        _lib.check(_lib.load().lavie_debug_op_statistics_last(ctypes.byref(info)), "lavie_debug_op_statistics_last")
        return {k: int(getattr(info, k)) for k, _ in info._fields_ if k != "struct_size"}


def producer_stats(partials, c, rows, nsets, set_blocks, span):
    """One lavie_gn_producer_stats descriptor of group_norm_stats: `partials` fp32 device, [nsets][set_blocks][c / 4][2][4]."""
    _chk32(partials)
    d = _lib.GnProducerStatsC()
    d.struct_size = ctypes.sizeof(d)
    d.C, d.partials, d.partials_floats = int(c), partials.data_ptr(), partials.numel()
    d.rows, d.nsets, d.set_blocks, d.span = int(rows), int(nsets), int(set_blocks), int(span)
    d._keep = partials
    return d


def group_norm_stats(x1, gamma, beta, nb, groups, eps, silu, x2=None, cs1=None, cs2=None, out=None, ws=None):
    """group_norm with the producers' column statistics of x1 / x2 (producer_stats() descriptors or None): a fold of the partials
    replaces the statistics pass where the descriptors can serve it (lavie_group_norm_stats_f16).  ws (optional): the fp32 scratch of
    lavie_group_norm_ws_floats(nb, groups) floats, whose first nb * groups * 2 hold (mean, rstd) per (batch, group) afterwards."""
    _chk16(x1, x2)
    _chk32(gamma, beta)
    rows = x1.shape[0]
    c1, c2 = x1.shape[1], 0 if x2 is None else x2.shape[1]
    y = _out(out, (rows, c1 + c2), torch.float16, x1.device, "group_norm_stats: out")
    ws_n = _lib.load().lavie_group_norm_ws_floats(nb, groups)
    ws = torch.empty(ws_n, dtype=torch.float32, device=x1.device) if ws is None else _out(ws, (ws_n,), torch.float32, x1.device, "group_norm_stats: ws")
    _lib.check(_lib.load().lavie_group_norm_stats_f16(_p(x1), c1, _p(x2), c2, nb, rows // nb, groups, _p(gamma), _p(beta), float(eps),
                                                      int(silu), _p(ws), _p(y), None if cs1 is None else ctypes.byref(cs1),
                                                      None if cs2 is None else ctypes.byref(cs2), _stream()), "lavie_group_norm_stats_f16")
    return y


def rowstat_finalize(partials, row_len, eps=1e-5, out=None):
    """Row statistics [M, slots, 2] (sum, sum of squares over row_len values per row) -> (mean, rstd) [M, 2] fp32: the ln_stats of
    linear_lnfold (lavie_rowstat_finalize_f32)."""
    _chk32(partials)
    m, slots, two = partials.shape
    if two != 2:
        raise ValueError("rowstat_finalize: partials must be [M, slots, 2]")
    out = _out(out, (m, 2), torch.float32, partials.device, "rowstat_finalize: out")
    _lib.check(_lib.load().lavie_rowstat_finalize_f32(_p(partials), slots, m, int(row_len), float(eps), _p(out), _stream()),
               "lavie_rowstat_finalize_f32")
    return out


def group_norm_affine(x, gamma, beta, nb, groups, eps, out=None):
    """GroupNorm statistics only: the normalisation as per-(batch, channel) pairs (a, b) with norm(x) = a x + b -> [nb, C, 2] fp32
    (lavie_group_norm_affine_f16; consumed by proj_qkv)."""
    _chk16(x)
    _chk32(gamma, beta)
    rows, c = x.shape
    ab = _out(out, (nb, c, 2), torch.float32, x.device, "group_norm_affine: out")
    ws = torch.empty(_lib.load().lavie_group_norm_ws_floats(nb, groups), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().lavie_group_norm_affine_f16(_p(x), c, nb, rows // nb, groups, _p(gamma), _p(beta), float(eps), _p(ws),
                                                       _p(ab), _stream()), "lavie_group_norm_affine_f16")
    return ab


def pack_proj_qkv(wpin, wqkv):
    """proj_in.weight [C, C] and the stacked attn1 to_q / to_k / to_v weights [3C, C] (fp16, device) -> the weight image of the fused
    block-head kernel (lavie_proj_qkv_f16).  Raises for a width the kernel is not built for."""
    _chk16(wpin, wqkv)
    C = wpin.shape[0]
    lib = _lib.load()
    nbytes = lib.lavie_proj_qkv_image_bytes(C)
    if nbytes == 0 or tuple(wpin.shape) != (C, C) or tuple(wqkv.shape) != (3 * C, C):
        raise RuntimeError(f"proj_qkv: width {C} is not built (or weight shapes do not match)")
    img = torch.empty(nbytes // 2, dtype=torch.float16, device=wpin.device)
    _lib.check(lib.lavie_pack_proj_qkv_f16(_p(wpin), _p(wqkv), C, _p(img), _stream()), "lavie_pack_proj_qkv_f16")
    return img


def proj_qkv(x, gn_ab, rows_per_domain, img, bpin, ln_gamma, ln_beta, eps=1e-5, tx=None, qkv=None):
    """tx = proj_in(GroupNorm(x)), qkv = to_qkv(LayerNorm(tx)) in one kernel (attention.py:369-373, 513-516) -> (tx [M, C], qkv [M, 3C])."""
    _chk16(x, img)
    _chk32(gn_ab, bpin, ln_gamma, ln_beta)
    M, C = x.shape
    tx = _out(tx, (M, C), torch.float16, x.device, "proj_qkv: tx")
    qkv = _out(qkv, (M, 3 * C), torch.float16, x.device, "proj_qkv: qkv")
    _lib.check(_lib.load().lavie_proj_qkv_f16(_p(x), _p(gn_ab), rows_per_domain, _p(img), _p(bpin), _p(ln_gamma), _p(ln_beta), eps,
                                              _p(tx), _p(qkv), M, C, _stream()), "lavie_proj_qkv_f16")
    return tx, qkv


def layer_norm(x, gamma, beta, eps=1e-5, out=None):
    _chk16(x)
    _chk32(gamma, beta)
    y = _out(out, x.shape, torch.float16, x.device, "layer_norm: out")
    _lib.check(_lib.load().lavie_layer_norm_f16(_p(x), _p(gamma), _p(beta), _p(y), x.shape[0], x.shape[1], float(eps),
                                                _stream()), "lavie_layer_norm_f16")
    return y


def attention(q, k, v, nb, lq, lk, heads, kv_batch_div=1, scale=None, out=None):
    """q [nb*lq, *], k/v [(nb/kv_batch_div)*lk, *] may be column slices of wider row-major tensors."""
    _chk_cols16(q, k, v)
    c = q.shape[1]
    dh = c // heads
    o = _out(out, (nb * lq, c), torch.float16, q.device, "attention: out")
    scale = dh ** -0.5 if scale is None else scale
    _lib.check(_lib.load().lavie_attention_f16(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), c, nb,
                                               lq, lk, heads, dh, kv_batch_div, float(scale), _stream()),
               "lavie_attention_f16")
    return o


def causal_attention(qkv, nb, l, heads, dh, scale=None, out=None):
    """Causal self-attention over packed rows: qkv [nb*l, ld] holds q | k | v (each heads*dh wide) in its first 3*heads*dh columns;
    row i of a batch entry attends to its rows j <= i.  out [nb*l, ldo >= heads*dh] (a new one is exactly heads*dh wide)."""
    if not (qkv.is_cuda and qkv.dtype == torch.float16 and qkv.dim() == 2 and qkv.stride(1) == 1):
        raise ValueError("causal_attention: qkv must be a 2-D fp16 device tensor with unit column stride")
    if out is None:
        out = torch.empty((max(nb * l, 0), heads * dh), dtype=torch.float16, device=qkv.device)
    elif not (out.is_cuda and out.device == qkv.device and out.dtype == torch.float16 and out.dim() == 2 and out.stride(1) == 1):
        raise ValueError("causal_attention: out must be a 2-D fp16 tensor with unit column stride on the device of qkv")
    if qkv.shape[0] < nb * l or out.shape[0] < nb * l:
        raise ValueError(f"causal_attention: nb * l = {nb * l} rows, but qkv has {qkv.shape[0]} and out {out.shape[0]}")
    scale = dh ** -0.5 if scale is None else scale
    _lib.check(_lib.load().lavie_causal_attention_f16(_p(qkv), qkv.stride(0), _p(out), out.stride(0), nb, l, heads, dh, float(scale),
                                                      _stream()), "lavie_causal_attention_f16")
    return out


def token_embed(ids, tok_table, pos_table, out=None):
    """CLIPTextEmbeddings: out [b*l, c] = fp16(tok_table[ids].float() + pos_table[position].float()).  ids [b, l] integers, on the
    host or the device; validated here (an id outside [0, V) raises; the kernel would clamp it)."""
    _chk16(tok_table, pos_table)
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError("token_embed: ids must be a [b, l] int32 / int64 tensor")
    b, l = ids.shape
    v, c = tok_table.shape
    if l > pos_table.shape[0]:
        raise ValueError(f"token_embed: l = {l} exceeds the {pos_table.shape[0]} rows of the position table")
    if pos_table.shape[1] != c:
        raise ValueError("token_embed: the two tables differ in width")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= v):
        raise ValueError(f"token_embed: ids must lie in [0, {v}), got [{int(ids.min())}, {int(ids.max())}]")
    ids32 = ids.to(device=tok_table.device, dtype=torch.int32).contiguous()
    out = _out(out, (b * l, c), torch.float16, tok_table.device, "token_embed: out")
    _lib.check(_lib.load().lavie_token_embed_f16(_p(ids32), _p(tok_table), _p(pos_table), _p(out), b, l, c, v, _stream()),
               "lavie_token_embed_f16")
    return out


ACT_KINDS = {"quick_gelu": 0, "gelu": 1}


def act(x, kind):
    """In place: kind "quick_gelu" = x * sigmoid(1.702 x), "gelu" = erf-GELU; fp32 arithmetic, one rounding.  Returns x."""
    if kind not in ACT_KINDS:
        raise ValueError(f"act: kind {kind!r} is not one of {sorted(ACT_KINDS)}")
    _chk16(x)
    _lib.check(_lib.load().lavie_act_f16(_p(x), x.numel(), ACT_KINDS[kind], _stream()), "lavie_act_f16")
    return x


def _chk_rows16(what, *ts):
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1):
            raise ValueError(f"{what} must be 2-D fp16 device tensors with unit column stride")


def short_attention(q, k, v, nb, lq, lk, heads, dh, scale=None, out=None):
    """Bidirectional attention over short sequences (lq, lk <= 320; dh 32 / 64): q [nb*lq, *], k and v [nb*lk, *] hold their heads
    in their first heads*dh columns and may be column slices of wider tensors, each with its own pitch (q | k | v of one fused
    tensor, or q from one tensor and k | v from another).  out [nb*lq, ldo >= heads*dh] (a new one is exactly heads*dh wide)."""
    _chk_rows16("short_attention: q, k and v", q, k, v)
    if out is None:
        out = torch.empty((max(nb * lq, 0), heads * dh), dtype=torch.float16, device=q.device)
    else:
        _chk_rows16("short_attention: out", out)
    if q.shape[0] < nb * lq or out.shape[0] < nb * lq or k.shape[0] < nb * lk or v.shape[0] < nb * lk:
        raise ValueError(f"short_attention: nb * lq = {nb * lq} query rows and nb * lk = {nb * lk} key rows, but q has {q.shape[0]}, "
                         f"out {out.shape[0]}, k {k.shape[0]}, v {v.shape[0]}")
    if min(q.shape[1], k.shape[1], v.shape[1], out.shape[1]) < heads * dh:
        raise ValueError(f"short_attention: every tensor needs heads * dh = {heads * dh} columns")
    scale = dh ** -0.5 if scale is None else scale
    _lib.check(_lib.load().lavie_short_attention_f16(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                                     nb, lq, lk, heads, dh, float(scale), _stream()), "lavie_short_attention_f16")
    return out


def pack_patch_embed(weight):
    """CLIPVisionEmbeddings.patch_embedding.weight [c, 3, p, p] -> [c, lavie_patch_embed_k(p)]: K = 3 p^2 zero-padded to a multiple of 64."""
    _chk16(weight)
    c, three, p, p2 = weight.shape
    if three != 3 or p != p2:
        raise ValueError(f"pack_patch_embed: weight must be [c, 3, p, p], got {tuple(weight.shape)}")
    lib = _lib.load()
    kp = lib.lavie_patch_embed_k(p)
    if kp < 0:
        raise ValueError(f"pack_patch_embed: patch size {p} is outside 1..64")
    out = torch.empty((c, kp), dtype=torch.float16, device=weight.device)
    _lib.check(lib.lavie_pack_patch_embed_f16(_p(weight), _p(out), c, p, _stream()), "lavie_pack_patch_embed_f16")
    return out


def patch_embed(pixel_values, wp, class_embedding, pos_table, patch, out=None):
    """CLIPVisionEmbeddings: pixel_values [b, 3, s, s] (fp16 or fp32, NCHW, read in place), wp from pack_patch_embed, class_embedding
    [c], pos_table [1 + (s/patch)^2, c] -> [b, 1 + (s/patch)^2, c] fp16; see lavie_patch_embed_f16."""
    _chk16(wp, class_embedding, pos_table)
    flag = _edge_dtype(pixel_values, "patch_embed: pixel_values")
    if pixel_values.dim() != 4 or pixel_values.shape[1] != 3 or pixel_values.shape[2] != pixel_values.shape[3]:
        raise ValueError(f"patch_embed: pixel_values must be [b, 3, s, s], got {tuple(pixel_values.shape)}")
    b, _, s, _ = pixel_values.shape
    c = class_embedding.numel()
    lib = _lib.load()
    nbytes = lib.lavie_patch_embed_workspace_bytes(b, s, patch)
    if nbytes < 0 or patch < 1 or patch > 64:
        raise ValueError(f"patch_embed: image size {s} is not a multiple of the patch size {patch}")
    g = s // patch
    if tuple(pos_table.shape) != (1 + g * g, c) or tuple(wp.shape) != (c, lib.lavie_patch_embed_k(patch)):
        raise ValueError(f"patch_embed: pos_table must be [{1 + g * g}, {c}] and wp the pack_patch_embed image of [{c}, 3, {patch}, {patch}]")
    ws = torch.empty(nbytes // 2, dtype=torch.float16, device=wp.device)
    y = _out(out, (b, 1 + g * g, c), torch.float16, wp.device, "patch_embed: out")
    _lib.check(lib.lavie_patch_embed_f16(_p(pixel_values), flag, _p(wp), _p(class_embedding), _p(pos_table), _p(y), _p(ws), b, s, patch, c,
                                         _stream()), "lavie_patch_embed_f16")
    return y


def relu(x):
    """In place: max(x, 0), exact (negative values become +0; -0, +0 and NaN keep their bits, as torch.relu).  Returns x."""
    _chk16(x)
    _lib.check(_lib.load().lavie_relu_f16(_p(x), x.numel(), _stream()), "lavie_relu_f16")
    return x


def sparse_causal_attention(q, k, v, nb, frames, d, heads, scale=None, out=None):
    """SparseCausalAttention core (interpolation/models/attention.py:609-665): q/k/v [nb*d, *] per-frame rows (column
    slices of a wider tensor allowed); frame f of a video attends to [first frame || frame max(f-1, 0)] of that video."""
    _chk_cols16(q, k, v)
    c = q.shape[1]
    dh = c // heads
    o = _out(out, (nb * d, c), torch.float16, q.device, "sparse_causal_attention: out")
    scale = dh ** -0.5 if scale is None else scale
    _lib.check(_lib.load().lavie_sparse_causal_attention_f16(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0),
                                                             _p(o), c, nb, frames, d, heads, dh, float(scale), _stream()),
               "lavie_sparse_causal_attention_f16")
    return o


def relpos_buckets(frames: int, num_buckets: int = 32, max_distance: int = 32) -> torch.Tensor:
    """Host-side bucket table [F, F] (query i, key j) — needs no GPU."""
    buf = (ctypes.c_int * (frames * frames))()
    _lib.check(_lib.load().lavie_relpos_buckets(frames, num_buckets, max_distance, buf), "lavie_relpos_buckets")
    return torch.tensor(list(buf), dtype=torch.int64).reshape(frames, frames)


def rotary_tables(frames: int, rot_dim: int = 32, theta: float = 10000.0, device="cuda"):
    """cos/sin [F, rot_dim/2] in fp32 (angles = frame * theta^(-2k/rot_dim))."""
    inv = theta ** (-torch.arange(0, rot_dim, 2, dtype=torch.float32) / rot_dim)
    ang = torch.arange(frames, dtype=torch.float32).reshape(-1, 1) * inv.reshape(1, -1)
    return ang.cos().to(device).contiguous(), ang.sin().to(device).contiguous()


def temporal_attention(qkv, b, frames, d, heads, bias, rot_cos, rot_sin, rot_dim=32, scale=None, out=None):
    """qkv [(b f d), 3C] (q | k | v) in (b, f, pixel) token order -> [(b f d), C]."""
    _chk16(qkv)
    _chk32(bias, *(() if rot_dim == 0 else (rot_cos, rot_sin)))      # rot_dim = 0: no rotary embedding, tables may be None
    c = qkv.shape[1] // 3
    dh = c // heads
    o = _out(out, (qkv.shape[0], c), torch.float16, qkv.device, "temporal_attention: out")
    scale = dh ** -0.5 if scale is None else scale
    _lib.check(_lib.load().lavie_temporal_attention_f16(_p(qkv), 3 * c, _p(o), c, b, frames, d, heads, dh, _p(bias),
                                                        _p(rot_cos), _p(rot_sin), rot_dim, float(scale), _stream()),
               "lavie_temporal_attention_f16")
    return o


def _step(entry, who, eps, x, aux, model_in, coeffs, next_input_scale, *, guidance=None, table=None, region=None, counts=True,
          pag_scale=None):
    """The body of every scheduler-step wrapper: dtype, element-count and shape checks, then the C entry `entry` with its operands
    in the order the entries share: eps, x, aux, model_in, n, [guidance | table, [per]], the five coefficients, next_input_scale,
    the stream, [the region].  The wrapper's name `who` says the form: cfg_ = eps / model_in hold both guidance halves, multistep =
    aux is the x0_prev history (else the step's noise, which may be None), _scaled = guidance from `table` [P, 2].
    region = (known, mask, noise_known, level) of a step around known latents.  pag_scale (the _pag_ wrappers): eps / model_in hold
    one part more, the perturbed prediction last, and the scale follows next_input_scale."""
    guided, multistep, scaled = who.startswith("cfg_"), "multistep" in who, who.endswith("_scaled")
    if pag_scale is not None:
        parts = 3 if guided else 2
        _chk16(eps, model_in)
        _chk32(x, aux)
        if multistep and aux is None:
            raise ValueError(f"{who}: x0_prev is needed")
        if eps.numel() != parts * x.numel() or model_in.numel() != parts * x.numel() or (aux is not None and aux.numel() != x.numel()):
            raise ValueError(f"{who}: eps / model_in must have {parts} times, " + ("x0_prev" if multistep else "noise") +
                             " as many elements as x")
        k_x, k_e, c_x0, c_xt, c4 = coeffs
        how = (float(guidance),) if guided else ()
        _lib.check(getattr(_lib.load(), entry)(_p(eps), _p(x), _p(aux), _p(model_in), x.numel(), *how, float(k_x), float(k_e), float(c_x0),
                                               float(c_xt), float(c4), float(next_input_scale), float(pag_scale), _stream()), entry)
        return
    if scaled and multistep and aux is None:
        raise ValueError(f"{who}: x0_prev is needed")
    _chk16(eps, model_in)
    _chk32(x, aux, table)
    n = x.numel()
    m = 2 * n if guided else n
    if counts and (eps.numel() != m or model_in.numel() != m or ((multistep or scaled) and aux is not None and aux.numel() != n)):
        if scaled:
            raise ValueError(f"{who}: eps2 / model_in2 must have twice, noise / x0_prev as many elements as x")
        if guided:
            raise ValueError(f"{who}: eps2 / model_in2 must have twice" + (", x0_prev" if multistep else "") + " as many elements as x")
        raise ValueError(f"{who}: eps / model_in" + (" / x0_prev" if multistep else "") + " must have as many elements as x")
    if scaled and (table is None or tuple(table.shape) != (x.shape[0], 2) or table.device != x.device):
        raise ValueError(f"{who}: table must be an fp32 tensor [{x.shape[0]}, 2] on {x.device}")
    k_x, k_e, c_x0, c_xt, c4 = coeffs
    if scaled:
        how = (_p(table), n // x.shape[0]) if region is None else (_p(table),)
    else:
        how = (float(guidance),) if guided else ()
    tail = () if region is None else (ctypes.byref(_known_region(who, x, *region)),)
    _lib.check(getattr(_lib.load(), entry)(_p(eps), _p(x), _p(aux), _p(model_in), n, *how, float(k_x), float(k_e), float(c_x0), float(c_xt),
                                           float(c4), float(next_input_scale), _stream(), *tail), entry)


def cfg_ddpm_step(eps2, x, noise, model_in2, guidance, coeffs, next_input_scale: float = 1.0):
    """Fused CFG + scheduler update; `coeffs` = (k_x, k_eps, c_x0, c_xt, sigma) from <scheduler>.coefficients;
    `next_input_scale` = the scheduler's scale_model_input factor of the next step (1 for DDPM / DDIM)."""
    _step("lavie_cfg_sampler_step", "cfg_ddpm_step", eps2, x, noise, model_in2, coeffs, next_input_scale, guidance=guidance, counts=False)


def latents_to_model_input(x, model_in2, input_scale: float = 1.0):
    _chk32(x)
    _chk16(model_in2)
    _lib.check(_lib.load().lavie_latents_to_scaled_model_input(_p(x), _p(model_in2), x.numel(), float(input_scale), _stream()))


def sampler_step(eps, x, noise, model_in, coeffs, next_input_scale: float = 1.0):
    """Scheduler update without classifier-free guidance (guidance_scale <= 1): eps / model_in are fp16 of x's size."""
    _step("lavie_sampler_step", "sampler_step", eps, x, noise, model_in, coeffs, next_input_scale)


def cfg_multistep_step(eps2, x, x0_prev, model_in2, guidance, coeffs, next_input_scale: float = 1.0):
    """Fused CFG + multistep (DPM-Solver++ 2M) update; `coeffs` = (k_x, k_eps, c_x0, c_xt, c_prev) from a multistep scheduler's
    `coefficients`; `x0_prev` = fp32 history of x's size, rewritten every step and read only when c_prev != 0."""
    _step("lavie_cfg_multistep_step", "cfg_multistep_step", eps2, x, x0_prev, model_in2, coeffs, next_input_scale, guidance=guidance)


def multistep_step(eps, x, x0_prev, model_in, coeffs, next_input_scale: float = 1.0):
    """The multistep update without classifier-free guidance (guidance_scale <= 1): eps / model_in are fp16 of x's size."""
    _step("lavie_multistep_step", "multistep_step", eps, x, x0_prev, model_in, coeffs, next_input_scale)


def cfg_pag_sampler_step(eps3, x, noise, model_in3, guidance, pag_scale, coeffs, next_input_scale: float = 1.0):
    """Fused CFG + perturbed-attention guidance + five-coefficient update (lavie_cfg_pag_sampler_step): eps3 / model_in3 fp16 [3, n] =
    [negative | prompt | perturbed], eps = u + g (c - u) + pag_scale (c - p); model_in3 gets the next input in all three parts."""
    _step("lavie_cfg_pag_sampler_step", "cfg_pag_sampler_step", eps3, x, noise, model_in3, coeffs, next_input_scale, guidance=guidance,
          pag_scale=pag_scale)


def pag_sampler_step(eps2, x, noise, model_in2, pag_scale, coeffs, next_input_scale: float = 1.0):
    """The same without classifier-free guidance: eps2 / model_in2 fp16 [2, n] = [prompt | perturbed], eps = c + pag_scale (c - p)."""
    _step("lavie_pag_sampler_step", "pag_sampler_step", eps2, x, noise, model_in2, coeffs, next_input_scale, pag_scale=pag_scale)


def cfg_pag_multistep_step(eps3, x, x0_prev, model_in3, guidance, pag_scale, coeffs, next_input_scale: float = 1.0):
    """cfg_pag_sampler_step for the multistep family (DPM-Solver++ 2M): `x0_prev` as in cfg_multistep_step."""
    _step("lavie_cfg_pag_multistep_step", "cfg_pag_multistep_step", eps3, x, x0_prev, model_in3, coeffs, next_input_scale,
          guidance=guidance, pag_scale=pag_scale)


def pag_multistep_step(eps2, x, x0_prev, model_in2, pag_scale, coeffs, next_input_scale: float = 1.0):
    """pag_sampler_step for the multistep family."""
    _step("lavie_pag_multistep_step", "pag_multistep_step", eps2, x, x0_prev, model_in2, coeffs, next_input_scale, pag_scale=pag_scale)


def _known_region(who, x, known, mask, noise_known, level):
    """The lavie_known_region of a step on latents x [P, C, ...]: known / noise_known shaped as x, mask [P, 1, ...] (None only for
    known_blend), level = (a_next, s_next) from <scheduler>.noise_level.  Returns the struct; it borrows the tensors."""
    _chk32(x, known, mask, noise_known)
    if x.dim() < 3:
        raise ValueError(f"{who}: latents must be [P, C, ...], got {tuple(x.shape)}")
    if known is None or tuple(known.shape) != tuple(x.shape):
        raise ValueError(f"{who}: known must have the latents' shape {tuple(x.shape)}")
    if noise_known is not None and tuple(noise_known.shape) != tuple(x.shape):
        raise ValueError(f"{who}: noise_known must have the latents' shape {tuple(x.shape)}")
    want = (x.shape[0], 1) + tuple(x.shape[2:])
    if mask is not None and tuple(mask.shape) != want:
        raise ValueError(f"{who}: mask must have shape {want}, got {tuple(mask.shape)}")
    a, s = level
    r = _lib.KnownRegionC()
    r.struct_size = ctypes.sizeof(_lib.KnownRegionC)
    r.channels = x.shape[1]
    r.inner = math.prod(x.shape[2:])
    r.known, r.mask, r.noise_known = known.data_ptr(), (mask.data_ptr() if mask is not None else None), \
        (noise_known.data_ptr() if noise_known is not None else None)
    r.a_next, r.s_next = float(a), float(s)
    return r


def known_blend(x, model_in, known, mask, noise_known, level, input_scale: float = 1.0):
    """x <- select(mask, x, a known + s noise_known) in place, level = (a, s), and model_in <- fp16(x input_scale): as many
    elements as x, or twice as many ([x | x], the guided model input).  mask None = 1 everywhere: the scheduler's add_noise."""
    _chk16(model_in)
    n = x.numel()
    if model_in.numel() not in (n, 2 * n):
        raise ValueError("known_blend: model_in must have as many elements as x, or twice as many")
    r = _known_region("known_blend", x, known, mask, noise_known, level)
    _lib.check(_lib.load().lavie_known_blend_f32(_p(x), _p(model_in), int(model_in.numel() == 2 * n), n, float(input_scale),
                                                 _stream(), ctypes.byref(r)), "lavie_known_blend_f32")


def cfg_sampler_step_known(eps2, x, noise, model_in2, guidance, coeffs, next_input_scale, known, mask, noise_known, level):
    """cfg_ddpm_step around known latents: after the update, x <- select(mask, x', a known + s noise_known) with level = (a, s)
    = <scheduler>.noise_level of the timestep the step lands on; model_in2 = fp16 of that x, both halves equal."""
    _step("lavie_cfg_sampler_step_known", "cfg_sampler_step_known", eps2, x, noise, model_in2, coeffs, next_input_scale,
          guidance=guidance, region=(known, mask, noise_known, level))


def sampler_step_known(eps, x, noise, model_in, coeffs, next_input_scale, known, mask, noise_known, level):
    """sampler_step (no guidance) around known latents; see cfg_sampler_step_known."""
    _step("lavie_sampler_step_known", "sampler_step_known", eps, x, noise, model_in, coeffs, next_input_scale,
          region=(known, mask, noise_known, level))


def cfg_multistep_step_known(eps2, x, x0_prev, model_in2, guidance, coeffs, next_input_scale, known, mask, noise_known, level):
    """cfg_multistep_step around known latents; the history written is select(mask, x0, known): a pinned element's x0 is known."""
    _step("lavie_cfg_multistep_step_known", "cfg_multistep_step_known", eps2, x, x0_prev, model_in2, coeffs, next_input_scale,
          guidance=guidance, region=(known, mask, noise_known, level))


def multistep_step_known(eps, x, x0_prev, model_in, coeffs, next_input_scale, known, mask, noise_known, level):
    """multistep_step (no guidance) around known latents; see cfg_multistep_step_known."""
    _step("lavie_multistep_step_known", "multistep_step_known", eps, x, x0_prev, model_in, coeffs, next_input_scale,
          region=(known, mask, noise_known, level))


def guidance_partials_floats(latents: int, per: int) -> int:
    """fp32 elements of the workspace `guidance_table` needs for `latents` latents (windows x P) of `per` elements each."""
    n = _lib.load().lavie_guidance_partials_floats(int(latents), int(per))
    if n < 0:
        raise ValueError(f"guidance_partials_floats: latents={latents} per={per} out of range (latents >= 1, per >= 2)")
    return n


def guidance_table(eps2, latents, guidance, rescale, workspace=None, out=None, moments_out=None):
    """The per-latent (guidance scale, rescale factor) table the `*_scaled` steps read (lavie_guidance_table, csrc/sampler_guidance.hip).
    eps2: the fp16 model output [2 P, ...] = [negative | prompt] of P = `latents` latents, or a list of W of them (one per frame window,
    each with statistics of its own).  guidance: one number for every latent, or P of them: a sequence, or an fp32 device tensor [P]
    (a sequence is copied to the device on every call; a loop passes the tensor).  rescale = phi in [0, 1]: f_p = phi std(ec) / std(e)
    + (1 - phi) with e = the guided prediction; 0 writes f_p = 1 without reading eps2.  workspace: fp32 device tensor of at least
    guidance_partials_floats(W P, per) elements (allocated when None and rescale != 0).  out: fp32 [P, 2], or [W, P, 2] for a list;
    moments_out: fp64 of out's shape with 4 in place of 2, receives the double sums of ec, ec^2, e, e^2.  Returns the table.
    No host synchronisation; with workspace and out given and guidance no host sequence, no allocation either."""
    windows = isinstance(eps2, (list, tuple))
    eps = list(eps2) if windows else [eps2]
    _chk16(*eps)
    p = int(latents)
    if not eps or p < 1 or any(t is None or t.shape[0] != 2 * p or t.numel() != eps[0].numel() or t.device != eps[0].device for t in eps):
        raise ValueError(f"guidance_table: every eps2 must be an fp16 device tensor [2 * {p}, ...] of one size")
    dev, per = eps[0].device, eps[0].numel() // (2 * p)
    phi = float(rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_table: rescale={rescale} must be in [0, 1]")
    g_dev, g = None, 1.0
    if isinstance(guidance, torch.Tensor):
        g_dev = guidance
    elif isinstance(guidance, (list, tuple)):
        g_dev = torch.tensor([float(v) for v in guidance], dtype=torch.float32, device=dev)
    else:
        g = float(guidance)
    if g_dev is not None:
        _chk32(g_dev)
        if g_dev.numel() != p or g_dev.device != dev:
            raise ValueError(f"guidance_table: got {g_dev.numel()} guidance scales for {p} latents")
    shape = (len(eps), p) if windows else (p,)
    table = _out(out, shape + (2,), torch.float32, dev, "guidance_table: out")
    if moments_out is not None:
        _out(moments_out, shape + (4,), torch.float64, dev, "guidance_table: moments_out")
    need = guidance_partials_floats(len(eps) * p, per) if phi != 0.0 else 0
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.float32, device=dev)
    if need:
        _chk32(workspace)
        if workspace.numel() < need or workspace.device != dev:
            raise ValueError(f"guidance_table: workspace has {workspace.numel()} elements, {need} needed")
    a = _lib.GuidanceTableArgsC()
    a.struct_size = ctypes.sizeof(_lib.GuidanceTableArgsC)
    a.W, a.P, a.per = len(eps), p, per
    eps_c = (ctypes.c_void_p * len(eps))(*[t.data_ptr() for t in eps])
    a.eps_host = eps_c
    a.guidance_dev, a.guidance, a.rescale = (g_dev.data_ptr() if g_dev is not None else None), g, phi
    a.partials, a.partials_floats = (workspace.data_ptr() if need else None), (workspace.numel() if need else 0)
    a.table, a.moments = table.data_ptr(), (moments_out.data_ptr() if moments_out is not None else None)
    _lib.check(_lib.load().lavie_guidance_table(ctypes.byref(a), _stream()), "lavie_guidance_table")
    return table


def cfg_sampler_step_scaled(eps2, x, noise, model_in2, table, coeffs, next_input_scale: float = 1.0):
    """cfg_ddpm_step with latent p's guidance scale and rescale factor read from table[p] (`guidance_table`): eps = f_p e.
    x [P, ...], noise and model_in2 are the plain step's operands, updated in place."""
    _step("lavie_cfg_sampler_step_scaled", "cfg_sampler_step_scaled", eps2, x, noise, model_in2, coeffs, next_input_scale, table=table)


def cfg_multistep_step_scaled(eps2, x, x0_prev, model_in2, table, coeffs, next_input_scale: float = 1.0):
    """cfg_multistep_step with (guidance, rescale factor) per latent from `table`; see cfg_sampler_step_scaled."""
    _step("lavie_cfg_multistep_step_scaled", "cfg_multistep_step_scaled", eps2, x, x0_prev, model_in2, coeffs, next_input_scale, table=table)


def cfg_sampler_step_known_scaled(eps2, x, noise, model_in2, table, coeffs, next_input_scale, known, mask, noise_known, level):
    """cfg_sampler_step_known with (guidance, rescale factor) per latent from `table`; see cfg_sampler_step_scaled."""
    _step("lavie_cfg_sampler_step_known_scaled", "cfg_sampler_step_known_scaled", eps2, x, noise, model_in2, coeffs, next_input_scale,
          table=table, region=(known, mask, noise_known, level))


def cfg_multistep_step_known_scaled(eps2, x, x0_prev, model_in2, table, coeffs, next_input_scale, known, mask, noise_known, level):
    """cfg_multistep_step_known with (guidance, rescale factor) per latent from `table`; see cfg_sampler_step_scaled."""
    _step("lavie_cfg_multistep_step_known_scaled", "cfg_multistep_step_known_scaled", eps2, x, x0_prev, model_in2, coeffs, next_input_scale,
          table=table, region=(known, mask, noise_known, level))


def _unipc(entry, who, eps, x, history, model_in, coeffs, next_input_scale, guidance=1.0, table=None):
    """The body of the three UniPC step wrappers (csrc/sampler_unipc.hip): `history` = (x_last, m1, m2), fp32 tensors of x's size
    that the launch rewrites; `coeffs` = (k_x, k_eps, corr, c_l, c_0, c_1, c_2, p_x, p_0, p_1), UniPCMultistepScheduler.coefficients."""
    guided = who.startswith("cfg_")
    if history is None or len(history) != 3 or any(t is None for t in history):
        raise ValueError(f"{who}: history must be the three fp32 tensors (x_last, m1, m2)")
    x_last, m1, m2 = history
    _chk16(eps, model_in)
    _chk32(x, x_last, m1, m2, table)
    n = x.numel()
    m = 2 * n if guided else n
    if eps.numel() != m or model_in.numel() != m or any(t.numel() != n for t in history):
        raise ValueError(f"{who}: eps / model_in must have " + ("twice" if guided else "as many elements as x") +
                         (", x_last / m1 / m2 as many elements as x" if guided else ", and so must x_last / m1 / m2"))
    if table is not None and (tuple(table.shape) != (x.shape[0], 2) or table.device != x.device):
        raise ValueError(f"{who}: table must be an fp32 tensor [{x.shape[0]}, 2] on {x.device}")
    k_x, k_e, corr, c_l, c_0, c_1, c_2, p_x, p_0, p_1 = coeffs
    c = _lib.UnipcCoeffsC(ctypes.sizeof(_lib.UnipcCoeffsC), int(bool(corr)), float(guidance), float(k_x), float(k_e), float(c_l),
                          float(c_0), float(c_1), float(c_2), float(p_x), float(p_0), float(p_1), float(next_input_scale))
    how = () if table is None else (_p(table), n // x.shape[0])
    _lib.check(getattr(_lib.load(), entry)(_p(eps), _p(x), _p(x_last), _p(m1), _p(m2), _p(model_in), n, *how, c, _stream()), entry)


def unipc_step(eps, x, history, model_in, coeffs, next_input_scale: float = 1.0):
    """The fused UniPC predictor-corrector step without classifier-free guidance: eps / model_in are fp16 of x's size."""
    _unipc("lavie_unipc_step", "unipc_step", eps, x, history, model_in, coeffs, next_input_scale)


def cfg_unipc_step(eps2, x, history, model_in2, guidance, coeffs, next_input_scale: float = 1.0):
    """Fused CFG + UniPC step: guidance, x0 prediction, corrector, predictor, the three history writes and the next fp16 model
    input [x' | x'] in one launch.  A history tensor is read only when a coefficient that multiplies it is non-zero."""
    _unipc("lavie_cfg_unipc_step", "cfg_unipc_step", eps2, x, history, model_in2, coeffs, next_input_scale, guidance=guidance)


def cfg_unipc_step_scaled(eps2, x, history, model_in2, table, coeffs, next_input_scale: float = 1.0):
    """cfg_unipc_step with (guidance, rescale factor) per latent from `table` [P, 2] (`guidance_table`)."""
    if table is None:
        raise ValueError("cfg_unipc_step_scaled: table is needed")
    _unipc("lavie_cfg_unipc_step_scaled", "cfg_unipc_step_scaled", eps2, x, history, model_in2, coeffs, next_input_scale, table=table)


def window_step(eps, x, aux, model_in, starts, profile, guidance, coeffs, next_input_scale: float = 1.0, multistep: bool = False):
    """One denoising step of a clip sampled as overlapping frame windows (lavie_window_step, csrc/sampler_window.hip).
    x fp32 [P, C, F, ...] is the whole clip, updated in place; eps / model_in are lists with one fp16 tensor [nb, C, L, ...] per
    window (the UNet's output for it / its next input), nb = 2 P = [negative | prompt] when `guidance` is a number, nb = P when it
    is None; window w covers frames [starts[w], starts[w] + L); profile = L positive weights (lavie_amd.windows).  The windows'
    predictions are averaged per frame with the normalised weights, the plain step of the family runs on the whole clip (`coeffs`
    as cfg_ddpm_step / cfg_multistep_step take them; aux = the step's noise, or the x0_prev history when `multistep`) and every
    window that covers a frame receives fp16(x' next_input_scale) in both guidance halves."""
    a, _keep = _window_args(eps, x, aux, model_in, starts, profile, guidance, coeffs, next_input_scale, multistep)
    _lib.check(_lib.load().lavie_window_step(ctypes.byref(a), _stream()), "lavie_window_step")


def window_step_scaled(eps, x, aux, model_in, starts, profile, table, coeffs, next_input_scale: float = 1.0, multistep: bool = False):
    """window_step under guidance with (guidance, rescale factor) of window w and latent p read from table[w, p] (`guidance_table` on
    the list of predictions): each window's guided prediction is multiplied by its own factor before the windows are averaged."""
    a, _keep = _window_args(eps, x, aux, model_in, starts, profile, 1.0, coeffs, next_input_scale, multistep)
    _chk32(table)
    if table is None or tuple(table.shape) != (a.W, a.P, 2) or table.device != x.device:
        raise ValueError(f"window_step_scaled: table must be an fp32 tensor [{a.W}, {a.P}, 2] on {x.device}")
    _lib.check(_lib.load().lavie_window_step_scaled(ctypes.byref(a), _p(table), _stream()), "lavie_window_step_scaled")


# ------------------------------------------------------------------ seeded engine noise (csrc/philox.h, csrc/sampler_noise.hip)
_U64 = (1 << 64) - 1


def philox4x32(key, counter):
    """Philox4x32-10 of (key[2], counter[4]) on the host (lavie_philox4x32_host): four 32-bit words.  Needs no device."""
    k, c, out = (ctypes.c_uint * 2)(*key), (ctypes.c_uint * 4)(*counter), (ctypes.c_uint * 4)()
    _lib.check(_lib.load().lavie_philox4x32_host(k, c, out), "lavie_philox4x32_host")
    return list(out)


def philox_normal(seeds, per: int, draw: int, first_element: int = 0, out=None, device="cuda"):
    """Standard normals fp32 [P, per]: row p = elements first_element .. first_element + per - 1 of the latent with seed seeds[p] at draw
    number `draw` (lavie_philox_normal_f32).  A value is a pure function of (seed, draw, element), so a row does not depend on the other
    rows, and a slice of a latent equals that range of the whole.  `out`: any fp32 tensor of P per elements whose memory is contiguous
    (its data pointer may be unaligned: every lane then makes one element, the same bits).  More than NOISE_MAX_SEEDS rows take one
    launch per sixteen."""
    seeds = [int(s) & _U64 for s in seeds]
    p, per = len(seeds), int(per)
    if p < 1 or per < 1:
        raise ValueError(f"philox_normal: {p} seeds and per={per} must be >= 1")
    if out is None:
        out = torch.empty((p, per), dtype=torch.float32, device=device)
    _chk32(out)
    if out.numel() != p * per:
        raise ValueError(f"philox_normal: out has {out.numel()} elements for {p} latents of {per}")
    for p0 in range(0, p, _lib.NOISE_MAX_SEEDS):
        part = seeds[p0:p0 + _lib.NOISE_MAX_SEEDS]
        _lib.check(_lib.load().lavie_philox_normal_f32(out.data_ptr() + 4 * p0 * per, (ctypes.c_ulonglong * len(part))(*part), len(part), per,
                                                       int(first_element), int(draw) & _U64, _stream()), "lavie_philox_normal_f32")
    return out


def _noise_key(who, key, latents: int, per: int):
    """lavie_noise_key of `key` (anything with `.seeds`, one per latent, and `.draw`: noise.NoiseKey) and the array it borrows."""
    seeds = [int(s) & _U64 for s in key.seeds]
    if len(seeds) != latents:
        raise ValueError(f"{who}: the noise key holds {len(seeds)} seeds for {latents} latents")
    if latents > _lib.NOISE_MAX_SEEDS:
        raise ValueError(f"{who}: a seeded step serves at most {_lib.NOISE_MAX_SEEDS} latents, got {latents}")
    k = _lib.NoiseKeyC()
    k.struct_size = ctypes.sizeof(_lib.NoiseKeyC)
    seeds_c = (ctypes.c_ulonglong * latents)(*seeds)
    k.count, k.seeds_host, k.per, k.draw = latents, seeds_c, per, int(key.draw) & _U64
    return k, seeds_c


def _step_seeded(entry, who, eps, x, key, model_in, coeffs, next_input_scale, guidance=None):
    guided = guidance is not None
    _chk16(eps, model_in)
    _chk32(x)
    n = x.numel()
    m = 2 * n if guided else n
    if eps.numel() != m or model_in.numel() != m:
        raise ValueError(f"{who}: eps / model_in must have {'twice ' if guided else ''}as many elements as x")
    k, _keep = _noise_key(who, key, x.shape[0], n // x.shape[0])
    k_x, k_e, c_x0, c_xt, c4 = coeffs
    how = (float(guidance),) if guided else ()
    _lib.check(getattr(_lib.load(), entry)(_p(eps), _p(x), _p(model_in), n, *how, float(k_x), float(k_e), float(c_x0), float(c_xt), float(c4),
                                           float(next_input_scale), _stream(), ctypes.byref(k)), entry)


def sampler_step_seeded(eps, x, key, model_in, coeffs, next_input_scale: float = 1.0):
    """sampler_step with the step's noise made inside the kernel from `key` (seeds of the latents x[p], draw number): x and model_in
    get the bits of `philox_normal(key.seeds, x[0].numel(), key.draw)` followed by sampler_step.  No noise tensor exists."""
    _step_seeded("lavie_sampler_step_seeded", "sampler_step_seeded", eps, x, key, model_in, coeffs, next_input_scale)


def cfg_sampler_step_seeded(eps2, x, key, model_in2, guidance, coeffs, next_input_scale: float = 1.0):
    """cfg_ddpm_step with the step's noise made inside the kernel from `key`, as sampler_step_seeded."""
    _step_seeded("lavie_cfg_sampler_step_seeded", "cfg_sampler_step_seeded", eps2, x, key, model_in2, coeffs, next_input_scale, guidance)


def window_step_seeded(eps, x, key, model_in, starts, profile, guidance, coeffs, next_input_scale: float = 1.0):
    """window_step of the five-coefficient family with the step's noise made inside the kernel from `key`: an element's index is its
    index in the whole clip, so x and model_in get the bits of window_step fed `philox_normal(key.seeds, x[0].numel(), key.draw)`."""
    a, _keep = _window_args(eps, x, None, model_in, starts, profile, guidance, coeffs, next_input_scale, False)
    k, _seeds = _noise_key("window_step_seeded", key, x.shape[0], x.numel() // x.shape[0])
    _lib.check(_lib.load().lavie_window_step_seeded(ctypes.byref(a), ctypes.byref(k), _stream()), "lavie_window_step_seeded")


# ------------------------------------------------------------------ the denoising objective evaluated forward (csrc/denoise_loss.hip)
LOSS_KINDS = {"epsilon": 0, "v_prediction": 1, "sample": 2}


def _denoise_args(who, x0, seeds, draw, levels, offset):
    """The checked (lavie_denoise_args, lavie_noise_key, P, per) of `noisy_latents` / `denoising_loss`, and the host arrays they borrow.
    levels: P pairs (a, s); offset: None or (coef, draw_offset, hw)."""
    if not (isinstance(x0, torch.Tensor) and x0.is_cuda and x0.dtype in (torch.float16, torch.float32) and x0.dim() >= 2):
        raise ValueError(f"{who}: x0 must be an fp16 or fp32 device tensor [P, ...]")
    if not x0.is_contiguous():
        raise ValueError(f"{who}: x0 must be contiguous")
    p = x0.shape[0]
    per = x0.numel() // p if p else 0
    if p < 1 or per < 1:
        raise ValueError(f"{who}: x0 {tuple(x0.shape)} holds no element")
    levels = [(float(a), float(s)) for a, s in levels]
    if len(levels) != p:
        raise ValueError(f"{who}: got {len(levels)} noise levels for {p} latents")
    key = NoiseKey([int(s) & _U64 for s in seeds], int(draw))
    k, seeds_c = _noise_key(who, key, p, per)
    a = _lib.DenoiseArgsC()
    a.struct_size = ctypes.sizeof(_lib.DenoiseArgsC)
    a.x0_dtype, a.x0 = int(x0.dtype == torch.float32), x0.data_ptr()
    a_c, s_c = (ctypes.c_float * p)(*[l[0] for l in levels]), (ctypes.c_float * p)(*[l[1] for l in levels])
    a.a_host, a.s_host = a_c, s_c
    if offset is not None:
        coef, draw_offset, hw = float(offset[0]), int(offset[1]) & _U64, int(offset[2])
        if hw < 1 or per % hw != 0:
            raise ValueError(f"{who}: offset hw={hw} must divide per={per}")
        if coef != 0.0:                            # coef == 0 adds nothing: the call without offset
            a.offset_coef, a.offset_draw, a.offset_hw = coef, draw_offset, hw
    return a, k, p, per, (seeds_c, a_c, s_c)


def noisy_latents(x0, seeds, draw, levels, offset=None, out=None):
    """The model input of the denoising objective (lavie_noisy_latents_seeded): out fp16, x0's shape [P, ...] = fp16(fma(s_p, n, a_p x0)),
    rounded once, with n the normal of (seeds[p], draw, element) made in the kernel (the bits of `philox_normal`) and levels[p] = (a_p,
    s_p) = (sqrt(abar_t), sqrt(1 - abar_t)).  offset = (coef, draw_offset, hw): n += coef m, m the normal of element e // hw of (seeds[p],
    draw_offset): one value per plane of hw elements.  x0 fp16 or fp32, at most NOISE_MAX_SEEDS latents.  No noise tensor exists."""
    a, k, p, per, _keep = _denoise_args("noisy_latents", x0, seeds, draw, levels, offset)
    if out is None:
        out = torch.empty(x0.shape, dtype=torch.float16, device=x0.device)
    if not (out.is_cuda and out.device == x0.device and out.dtype == torch.float16 and out.numel() == p * per and out.is_contiguous()):
        raise ValueError(f"noisy_latents: out must be a contiguous fp16 tensor of {p * per} elements on {x0.device}")
    _lib.check(_lib.load().lavie_noisy_latents_seeded(ctypes.byref(a), ctypes.byref(k), _p(out), _stream()), "lavie_noisy_latents_seeded")
    return out


def denoising_loss_workspace_floats(latents: int, per: int) -> int:
    """fp32 elements of the workspace `denoising_loss` needs for `latents` latents of `per` elements each."""
    n = _lib.load().lavie_denoising_loss_workspace_floats(int(latents), int(per))
    if n < 0:
        raise ValueError(f"denoising_loss_workspace_floats: latents={latents} per={per} out of range")
    return n


def denoising_loss(pred, x0, seeds, draw, levels, kind, offset=None, workspace=None, out=None):
    """fp32 [P]: the mean over latent p of (pred - target)^2 (lavie_denoising_loss_f32).  pred fp16 of x0's element count; target = n
    (`kind` "epsilon"), a_p n - s_p x0 ("v_prediction") or x0 ("sample"), with n regenerated in the kernel from (seeds, draw, offset): the
    bits `noisy_latents` used.  Sums in a fixed order: two calls agree bit for bit and a latent's value does not depend on P or on its
    position.  workspace: fp32 device tensor of at least denoising_loss_workspace_floats(P, per) elements (allocated when None)."""
    if kind not in LOSS_KINDS:
        raise ValueError(f"denoising_loss: kind {kind!r} is not one of {sorted(LOSS_KINDS)}")
    a, k, p, per, _keep = _denoise_args("denoising_loss", x0, seeds, draw, levels, offset)
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda and pred.device == x0.device and pred.dtype == torch.float16
            and pred.numel() == p * per and pred.is_contiguous()):
        raise ValueError(f"denoising_loss: pred must be a contiguous fp16 tensor of {p * per} elements on {x0.device}")
    need = denoising_loss_workspace_floats(p, per)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=x0.device)
    _chk32(workspace)
    if workspace.numel() < need or workspace.device != x0.device:
        raise ValueError(f"denoising_loss: workspace has {workspace.numel()} elements, {need} needed")
    out = _out(out, (p,), torch.float32, x0.device, "denoising_loss: out")
    _lib.check(_lib.load().lavie_denoising_loss_f32(ctypes.byref(a), ctypes.byref(k), _p(pred), LOSS_KINDS[kind], _p(out), _p(workspace),
                                                    workspace.numel(), _stream()), "lavie_denoising_loss_f32")
    return out


def _window_args(eps, x, aux, model_in, starts, profile, guidance, coeffs, next_input_scale, multistep):
    """The checked lavie_window_step_args of window_step / window_step_scaled, and the host arrays it borrows."""
    _chk32(x, aux)
    if x.dim() < 4:
        raise ValueError(f"window_step: latents must be [P, C, F, ...], got {tuple(x.shape)}")
    eps, model_in, starts, profile = list(eps), list(model_in), [int(s) for s in starts], [float(v) for v in profile]
    n_win, length = len(starts), len(profile)
    if not (len(eps) == len(model_in) == n_win) or n_win < 1:
        raise ValueError(f"window_step: {len(eps)} eps and {len(model_in)} model_in tensors for {n_win} window starts")
    _chk16(*eps, *model_in)
    cfg = guidance is not None
    p, c, f = x.shape[:3]
    want = ((2 * p if cfg else p), c, length) + tuple(x.shape[3:])
    for name, ts in (("eps", eps), ("model_in", model_in)):
        for w, t in enumerate(ts):
            if t is None or tuple(t.shape) != want or t.device != x.device:
                raise ValueError(f"window_step: {name}[{w}] must be an fp16 tensor of shape {want} on {x.device}")
    if aux is not None and (tuple(aux.shape) != tuple(x.shape) or aux.device != x.device):
        raise ValueError(f"window_step: aux must have the latents' shape {tuple(x.shape)} on {x.device}")
    k_x, k_e, c_x0, c_xt, c4 = coeffs
    a = _lib.WindowStepArgsC()
    a.struct_size = ctypes.sizeof(_lib.WindowStepArgsC)
    a.family, a.cfg = int(bool(multistep)), int(cfg)
    a.P, a.C, a.F, a.hw = p, c, f, math.prod(x.shape[3:])
    a.W, a.L = n_win, length
    starts_c, profile_c = (ctypes.c_int * n_win)(*starts), (ctypes.c_float * length)(*profile)
    eps_c = (ctypes.c_void_p * n_win)(*[t.data_ptr() for t in eps])
    min_c = (ctypes.c_void_p * n_win)(*[t.data_ptr() for t in model_in])
    a.starts_host, a.profile_host, a.eps_host, a.model_in_host = starts_c, profile_c, eps_c, min_c
    a.x, a.aux = x.data_ptr(), (aux.data_ptr() if aux is not None else None)
    a.guidance = float(guidance) if cfg else 1.0
    a.k_x, a.k_eps, a.c_x0, a.c_xt, a.c4 = float(k_x), float(k_e), float(c_x0), float(c_xt), float(c4)
    a.next_input_scale = float(next_input_scale)
    return a, (starts_c, profile_c, eps_c, min_c)


def latents_to_model_input1(x, model_in, input_scale: float = 1.0):
    _chk32(x)
    _chk16(model_in)
    _lib.check(_lib.load().lavie_latents_to_scaled_model_input1(_p(x), _p(model_in), x.numel(), float(input_scale), _stream()))


# ------------------------------------------------------------------ the forward's end and glue kernels, one wrapper per kernel
def timestep_sinusoid(t, dim, out=None):
    """Timesteps(dim, flip_sin_to_cos=True, freq_shift=0): t fp32 [B] -> fp32 [B, dim] = [cos(t w_k) | sin(t w_k)]."""
    _chk32(t)
    B = t.shape[0]
    out = _out(out, (B, dim), torch.float32, t.device, "timestep_sinusoid: out")
    _lib.check(_lib.load().lavie_timestep_sinusoid_f32(_p(t), _p(out), B, dim, _stream()), "lavie_timestep_sinusoid_f32")
    return out


def gemv(x, weight, bias=None, act_in=False, act_out=False, out=None):
    """act_out(act_in(x) @ weight^T + bias): x fp32 [B <= 8, K], weight fp16 [N, K], bias fp32 [N] -> fp32 [B, N]; act = SiLU."""
    _chk32(x, bias)
    _chk16(weight)
    B, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K or (bias is not None and bias.numel() != N):
        raise ValueError(f"gemv: x {tuple(x.shape)}, weight {tuple(weight.shape)} and bias do not fit")
    out = _out(out, (B, N), torch.float32, x.device, "gemv: out")
    _lib.check(_lib.load().lavie_gemv_f16(_p(x), _p(weight), _p(bias), _p(out), B, N, K, int(act_in), int(act_out), _stream()), "lavie_gemv_f16")
    return out


def pack_conv_in(weight, out=None):
    """[Cout, Cin, 3, 3] (fp16, device) -> the weight image of conv_in: 9 * Cin * Cout halfs, K pairs interleaved."""
    _chk16(weight)
    cout, cin = weight.shape[:2]
    out = _out(out, (9 * cin * cout,), torch.float16, weight.device, "pack_conv_in: out")
    _lib.check(_lib.load().lavie_pack_conv_in_f16(_p(weight), _p(out), cout, cin, _stream()), "lavie_pack_conv_in_f16")
    return out


def conv_in(x, wp, bias, cout, out=None):
    """3x3 conv, pad 1, from the NCFHW latent x [b, cin, f, h, w] (fp16) to channels-last rows [(b f h w), cout]; wp from pack_conv_in."""
    _chk16(x, wp)
    _chk32(bias)
    b, cin, f, h, w = x.shape
    if wp.numel() != 9 * cin * cout or bias is None or bias.numel() != cout:
        raise ValueError(f"conv_in: wp must be the pack_conv_in image of Cin={cin} Cout={cout} and bias [{cout}]")
    y = _out(out, (b * f * h * w, cout), torch.float16, x.device, "conv_in: out")
    _lib.check(_lib.load().lavie_conv_in_f16(_p(x), _p(wp), _p(bias), _p(y), b, cin, f, h, w, cout, _stream()), "lavie_conv_in_f16")
    return y


def pack_conv_out(weight, out=None):
    """[Cout, Cin, 3, 3] (fp16, device) -> [Cout, 9 * Cin] in (tap, channel) order: the weights of conv_out."""
    _chk16(weight)
    cout, cin = weight.shape[:2]
    out = _out(out, (cout, 9 * cin), torch.float16, weight.device, "pack_conv_out: out")
    _lib.check(_lib.load().lavie_pack_conv_out_f16(_p(weight), _p(out), cout, cin, _stream()), "lavie_pack_conv_out_f16")
    return out


def conv_out(x, wp, bias, b, f, h, w, out=None):
    """3x3 conv, pad 1, from channels-last rows x [(b f h w), cin] to the NCFHW output [b, cout <= 8, f, h, w] (fp16); wp from pack_conv_out."""
    _chk16(x, wp)
    _chk32(bias)
    cin, cout = x.shape[1], wp.shape[0]
    if x.shape[0] != b * f * h * w or tuple(wp.shape) != (cout, 9 * cin) or bias is None or bias.numel() != cout:
        raise ValueError(f"conv_out: x must be [{b * f * h * w}, cin] rows, wp [cout, 9 cin] and bias [cout]")
    y = _out(out, (b, cout, f, h, w), torch.float16, x.device, "conv_out: out")
    _lib.check(_lib.load().lavie_conv_out_f16(_p(x), _p(wp), _p(bias), _p(y), b, cin, f, h, w, cout, _stream()), "lavie_conv_out_f16")
    return y


def add_class_emb_silu(emb, table, labels):
    """emb[b] = silu(emb[b] + table[labels[b]]) in place: emb fp32 [B <= 8, N], table fp16 [num_classes, N], labels a sequence of ints."""
    _chk32(emb)
    _chk16(table)
    B, N = emb.shape
    labels = [int(v) for v in labels]
    if len(labels) != B or table.shape[1] != N:
        raise ValueError(f"add_class_emb_silu: emb {tuple(emb.shape)}, table {tuple(table.shape)} and {len(labels)} labels do not fit")
    arr = (ctypes.c_int * max(B, 1))(*labels)
    _lib.check(_lib.load().lavie_add_class_emb_silu_f32(_p(emb), _p(table), arr, B, N, table.shape[0], _stream()), "lavie_add_class_emb_silu_f32")
    return emb


def fill_relpos_bias(emb, frames, max_distance=128, buckets=None, out=None):
    """RelativePositionBias: emb fp16 [num_buckets, heads] -> fp32 [heads, F, F] = emb[bucket(i, j), h].  The bucket table is built
    here (relpos_buckets) and uploaded, so every index the kernel reads is in range; `buckets` (int32 device tensor [F, F]) is
    where the table is placed when the caller wants to own that buffer — its contents are overwritten with the table."""
    _chk16(emb)
    nb, heads = emb.shape
    table = relpos_buckets(frames, nb, max_distance).to(torch.int32)
    if buckets is None:
        buckets = table.to(emb.device)
    else:
        if not (buckets.dtype == torch.int32 and buckets.is_contiguous() and tuple(buckets.shape) == (frames, frames) and buckets.device == emb.device):
            raise ValueError(f"fill_relpos_bias: buckets must be a contiguous int32 [{frames}, {frames}] tensor on {emb.device}")
        buckets.copy_(table)
    out = _out(out, (heads, frames, frames), torch.float32, emb.device, "fill_relpos_bias: out")
    _lib.check(_lib.load().lavie_fill_relpos_bias_f32(_p(emb), _p(buckets), _p(out), heads, frames, nb, _stream()), "lavie_fill_relpos_bias_f32")
    return out


def ln_fold(weight, gamma, beta, bias=None, w_out=None, s_out=None, b_out=None):
    """The LayerNorm fold linear_lnfold consumes: (fp16(weight * gamma) [N, K], its fp32 row sums [N], weight @ beta (+ bias) [N]);
    weight fp16 [N, K], gamma / beta fp32 [K], bias fp16 [N] or None."""
    _chk16(weight, bias)
    _chk32(gamma, beta)
    N, K = weight.shape
    if gamma.numel() != K or beta.numel() != K or (bias is not None and bias.numel() != N):
        raise ValueError(f"ln_fold: weight {tuple(weight.shape)}, gamma, beta and bias do not fit")
    w_out = _out(w_out, (N, K), torch.float16, weight.device, "ln_fold: w_out")
    s_out = _out(s_out, (N,), torch.float32, weight.device, "ln_fold: s_out")
    b_out = _out(b_out, (N,), torch.float32, weight.device, "ln_fold: b_out")
    _lib.check(_lib.load().lavie_ln_fold_f16(_p(weight), _p(gamma), _p(beta), _p(bias), _p(w_out), _p(s_out), _p(b_out), N, K, _stream()),
               "lavie_ln_fold_f16")
    return w_out, s_out, b_out


def pack_geglu_vec(v, out=None):
    """pack_geglu's row permutation on an fp32 vector [N] (the folded bias and row sums of a GEGLU projection)."""
    _chk32(v)
    N = v.numel()
    out = _out(out, (N,), torch.float32, v.device, "pack_geglu_vec: out")
    _lib.check(_lib.load().lavie_pack_geglu_vec_f32(_p(v), _p(out), N, _stream()), "lavie_pack_geglu_vec_f32")
    return out


def copy_rows(src, dst, col0, cols=None):
    """dst[r, col0 + c] = src[r, c] for the first `cols` columns (default: all) of every row of src; fp16 [rows, ld] tensors."""
    _chk16(src, dst)
    rows, ld_src = src.shape
    cols = ld_src if cols is None else cols
    if dst.dim() != 2 or dst.shape[0] != rows:
        raise ValueError(f"copy_rows: dst must have the {rows} rows of src")
    _lib.check(_lib.load().lavie_copy_rows_f16(_p(src), ld_src, _p(dst), dst.shape[1], rows, cols, col0, _stream()), "lavie_copy_rows_f16")
    return dst


def f16_to_f32(a, b=None, out=None):
    """float(a) (+ float(b)): fp16 tensors -> fp32 of a's shape."""
    _chk16(a, b)
    if b is not None and b.shape != a.shape:
        raise ValueError("f16_to_f32: a and b must have one shape")
    out = _out(out, a.shape, torch.float32, a.device, "f16_to_f32: out")
    _lib.check(_lib.load().lavie_f16_to_f32(_p(a), _p(b), _p(out), a.numel(), _stream()), "lavie_f16_to_f32")
    return out


# ------------------------------------------------------------------ engine seams (sub-module forwards)
def unet_resnet_block(net, prefix: str, x1, x2, temb, b: int, f: int, h: int, w: int):
    """ResnetBlock3D.forward of `net`'s block `prefix` on channels-last rows (x2 = skip half or None).
    temb: fp32 [b, time_embed_dim] — the output of time_embedding (the block applies SiLU + its projection)."""
    _chk16(x1, x2)
    _chk32(temb)
    handle = net.engine_handle()
    cout = dict(net.named_parameters())[prefix + ".conv2.bias"].shape[0]
    y = torch.empty(x1.shape[0], cout, dtype=torch.float16, device=x1.device)
    _lib.check(_lib.load().lavie_unet_resnet_forward(handle, prefix.encode(), _p(x1), x1.shape[1], _p(x2),
                                                     0 if x2 is None else x2.shape[1], _p(temb), _p(y), b, f, h, w,
                                                     _stream()), "lavie_unet_resnet_forward")
    return y


def unet_transformer(net, prefix: str, x, ctx, b: int, f: int, h: int, w: int):
    """Transformer3DModel.forward of `net`'s block `prefix`; x rows are updated in place and returned."""
    _chk16(x, ctx)
    handle = net.engine_handle()
    _lib.check(_lib.load().lavie_unet_transformer_forward(handle, prefix.encode(), _p(x), _p(ctx), b, f, h, w,
                                                          ctx.shape[1], _stream()), "lavie_unet_transformer_forward")
    return x


def lora_merge(w0: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None):
    """fp16_rne(w0[N,K] + scale * b[N,r] @ a[r,K]) with a / b fp32 (lavie_lora_merge_f16: fp32 fmaf in ascending j, deterministic)."""
    _chk16(w0, out)
    _chk32(a, b)
    N, K = w0.shape
    r = a.shape[0]
    if a.shape != (r, K) or b.shape != (N, r):
        raise ValueError(f"lora_merge: w0 {tuple(w0.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)} do not fit")
    out = _out(out, w0.shape, torch.float16, w0.device, "lora_merge: out")
    lib = _lib.load()
    _lib.check(lib.lavie_lora_merge_f16(_p(w0), _p(a), _p(b), _p(out), N, K, r, float(scale), _stream()), "lavie_lora_merge_f16")
    return out


def lora_merge_multi(w0: torch.Tensor, terms, out: Optional[torch.Tensor] = None):
    """fp16_rne(w0[N,K] + sum_i scale_i * b_i[N,r_i] @ a_i[r_i,K]) for `terms` = [(a, b, scale), ...] (1..8 of them, a / b fp32), in
    one pass (lavie_lora_merge_multi_f16): fp32 sum in list order, each b_i a_i by lora_merge's chain, one rounding.  One term gives
    lora_merge's bits; a term with scale 0 is skipped."""
    _chk16(w0, out)
    N, K = w0.shape
    terms = list(terms)
    arr = (_lib.LoraTermC * max(1, len(terms)))()
    for i, (a, b, scale) in enumerate(terms):
        _chk32(a, b)
        r = a.shape[0]
        if a.shape != (r, K) or b.shape != (N, r):
            raise ValueError(f"lora_merge_multi: term {i}: w0 {tuple(w0.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)} do not fit")
        arr[i].A, arr[i].B, arr[i].r, arr[i].scale = a.data_ptr(), b.data_ptr(), r, float(scale)
    out = _out(out, w0.shape, torch.float16, w0.device, "lora_merge_multi: out")
    lib = _lib.load()
    _lib.check(lib.lavie_lora_merge_multi_f16(_p(w0), arr, len(terms), _p(out), N, K, _stream()), "lavie_lora_merge_multi_f16")
    return out


def freeu(h: torch.Tensor, skip: torch.Tensor, ni: int, height: int, width: int, b: float, s: float, out=None):
    """FreeU on the two operands of a decoder concat (lavie_freeu_f16; diffusers' apply_freeu / fourier_filter).  h [(ni height width),
    C_h], skip [(ni height width), C2], fp16 rows.  Returns (h_out, skip_out): h with its first C_h / 2 channels scaled by b, skip with
    the four lowest modes of every (image, channel)'s 2-D spectrum scaled by s.  out = (h_out, skip_out), either None (a new tensor) or
    the input itself (in place)."""
    _chk16(h, skip)
    rows = ni * height * width
    if h.dim() != 2 or skip.dim() != 2 or h.shape[0] != rows or skip.shape[0] != rows:
        raise ValueError(f"freeu: h {tuple(h.shape)} / skip {tuple(skip.shape)} are not [{ni} * {height} * {width}, C] row matrices")
    h_out, skip_out = out if out is not None else (None, None)
    _chk16(h_out, skip_out)
    h_out = _out(h_out, h.shape, torch.float16, h.device, "freeu: h_out")
    skip_out = _out(skip_out, skip.shape, torch.float16, skip.device, "freeu: skip_out")
    lib = _lib.load()
    c_h, c2 = h.shape[1], skip.shape[1]
    ws_bytes = lib.lavie_freeu_workspace_bytes(c2, ni, height, width)
    ws = torch.empty(max(int(ws_bytes) // 4, 4), dtype=torch.float32, device=h.device)
    _lib.check(lib.lavie_freeu_f16(_p(h), c_h, _p(skip), c2, ni, height, width, float(b), float(s), _p(h_out), _p(skip_out), _p(ws),
                                   _stream()), "lavie_freeu_f16")
    return h_out, skip_out


def freq_mix_workspace_bytes(images: int, f: int, h: int, w: int) -> int:
    """Bytes of workspace `freq_mix` needs for `images` volumes [f, h, w]; 0 for a shape it refuses."""
    return int(_lib.load().lavie_freq_mix_workspace_bytes(int(images), int(f), int(h), int(w)))


def freq_mix(x0, e0, z, filt, a: float, s: float, r: float, out=None, model_in=None, input_scale: float = 1.0, workspace=None):
    """FreeInit's frequency mix (lavie_freq_mix_f32, csrc/freq_mix.hip): out = r z + Re IFFT3(filt .* FFT3(a x0 + s e0 - r z)) over the
    last three axes of fp32 [..., F, H, W] tensors x0 / e0 / z; `filt` fp32 [F, H, W] in FFT-native order, even in frequency
    (lavie_amd.free_init.freq_filter), shared by every leading index.  out: None (a new tensor), or an fp32 tensor of x0's shape,
    which may be x0 itself.  model_in: None, or an fp16 tensor holding 1 to 3 copies of x0's shape along its first axis
    ([dup * P, C, F, H, W] for latents [P, C, F, H, W]); every copy receives fp16(out input_scale), rounded once.  workspace: None, or a
    device tensor of at least freq_mix_workspace_bytes() bytes.  Returns out."""
    _chk32(x0, e0, z, filt, out)
    _chk16(model_in)
    if x0.dim() < 3:
        raise ValueError(f"freq_mix: the operands must be [..., F, H, W], got {tuple(x0.shape)}")
    f, h, w = x0.shape[-3:]
    images = math.prod(x0.shape[:-3])
    for name, t in (("e0", e0), ("z", z)):
        if tuple(t.shape) != tuple(x0.shape) or t.device != x0.device:
            raise ValueError(f"freq_mix: {name} must have x0's shape {tuple(x0.shape)} on {x0.device}")
    if tuple(filt.shape) != (f, h, w) or filt.device != x0.device:
        raise ValueError(f"freq_mix: the filter must be an fp32 tensor {(f, h, w)} on {x0.device}, got {tuple(filt.shape)}")
    out = _out(out, x0.shape, torch.float32, x0.device, "freq_mix: out")
    args = _lib.FreqMixArgsC()
    args.struct_size = ctypes.sizeof(_lib.FreqMixArgsC)
    args.images, args.F, args.H, args.W = images, f, h, w
    args.x0, args.e0, args.z, args.filter, args.out = x0.data_ptr(), e0.data_ptr(), z.data_ptr(), filt.data_ptr(), out.data_ptr()
    args.a, args.s, args.r = float(a), float(s), float(r)
    if model_in is not None:
        dup, rest = divmod(model_in.numel(), x0.numel())
        if model_in.device != x0.device or rest or not 1 <= dup <= 3:
            raise ValueError(f"freq_mix: model_in must hold 1 to 3 copies of {tuple(x0.shape)} on {x0.device}, got {tuple(model_in.shape)}")
        args.model_in, args.dup, args.dup_stride, args.input_scale = model_in.data_ptr(), dup, x0.numel(), float(input_scale)
    lib = _lib.load()
    need = int(lib.lavie_freq_mix_workspace_bytes(images, f, h, w))
    if workspace is None:
        workspace = torch.empty(max(need // 4, 4), dtype=torch.float32, device=x0.device)
    elif not (workspace.is_cuda and workspace.device == x0.device and workspace.is_contiguous()):
        raise ValueError(f"freq_mix: workspace must be a contiguous tensor on {x0.device}")
    args.workspace, args.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    _lib.check(lib.lavie_freq_mix_f32(ctypes.byref(args), _stream()), "lavie_freq_mix_f32")
    return out


# ------------------------------------------------------------------ CLIP image processor, feature heads, CLIPSIM
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess(images, size=224, crop=224, mean=CLIP_MEAN, std=CLIP_STD, dtype=torch.float32, out=None):
    """CLIPImageProcessor on the device (lavie_clip_preprocess_u8): images uint8 [b, h, w, 3] with unit stride over (w, 3) -- rows and
    images may be further apart, as views of a wider buffer are -- -> [b, 3, crop, crop]: fp32 with the stock processor's bits, or
    fp16, one rounding of those."""
    if not (images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3):
        raise ValueError("clip_preprocess: images must be a uint8 device tensor [b, h, w, 3]")
    b, h, w, _ = images.shape
    if b < 1:
        raise ValueError("clip_preprocess: empty batch")
    if images.stride(3) != 1 or images.stride(2) != 3:
        raise ValueError("clip_preprocess: the pixels of a row must be contiguous")
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"clip_preprocess: dtype {dtype} is not fp32 or fp16")
    lib = _lib.load()
    cfg = _lib.ClipPreprocessConfigC()
    cfg.struct_size, cfg.size, cfg.crop = ctypes.sizeof(cfg), int(size), int(crop)
    cfg.mean[:], cfg.std[:] = [float(v) for v in mean], [float(v) for v in std]
    nbytes = lib.lavie_clip_preprocess_workspace_bytes(b, h, w, int(size), int(crop))
    if nbytes < 0:
        _lib.check(-1, "lavie_clip_preprocess_workspace_bytes")
    with torch.cuda.device(images.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=images.device)
        out = _out(out, (b, 3, int(crop), int(crop)), dtype, images.device, "clip_preprocess: out")
        _lib.check(lib.lavie_clip_preprocess_u8(_p(images), b, h, w, images.stride(1), images.stride(0), _p(out), int(dtype == torch.float32),
                                                ctypes.byref(cfg), _p(ws), nbytes, _stream()), "lavie_clip_preprocess_u8")
    return out


def clip_embed(x, weight, ids=None, eos_token_id=2, row=0, ln_weight=None, ln_bias=None, eps=1e-5, normalize=True, out=None):
    """fp32 [b, d] = normalise?(weight LN?(x[b, row_b])) (lavie_clip_embed_f16): x fp16 [b, l, c], weight fp16 [d, c]; ids (integer
    [b, l]) picks the row CLIPTextTransformer pools, otherwise `row`; ln_weight / ln_bias [c]: post_layernorm."""
    _chk16(x, weight)
    if x.dim() != 3 or weight.dim() != 2 or weight.shape[1] != x.shape[2]:
        raise ValueError(f"clip_embed: x must be [b, l, c] and weight [d, c], got {tuple(x.shape)} and {tuple(weight.shape)}")
    b, l, c = x.shape
    d = weight.shape[0]
    if (ln_weight is None) != (ln_bias is None):
        raise ValueError("clip_embed: ln_weight and ln_bias come together")
    g = None if ln_weight is None else ln_weight.to(device=x.device, dtype=torch.float32).contiguous()
    bt = None if ln_bias is None else ln_bias.to(device=x.device, dtype=torch.float32).contiguous()
    if g is not None and (g.numel() != c or bt.numel() != c):
        raise ValueError(f"clip_embed: ln_weight and ln_bias must have {c} elements")
    ids32 = None
    if ids is not None:
        if tuple(ids.shape) != (b, l):
            raise ValueError(f"clip_embed: ids must be [{b}, {l}], got {tuple(ids.shape)}")
        ids32 = ids.to(device=x.device, dtype=torch.int32).contiguous()
    out = _out(out, (b, d), torch.float32, x.device, "clip_embed: out")
    _lib.check(_lib.load().lavie_clip_embed_f16(_p(x), b, l, c, _p(ids32), int(eos_token_id), int(row), _p(g), _p(bt), float(eps), _p(weight), d,
                                                int(bool(normalize)), _p(out), _stream()), "lavie_clip_embed_f16")
    return out


def clip_similarity(image_features, text_features, frames=0, scale=1.0, out=None):
    """frames = 0: fp32 [n, p] = scale <img_n, txt_p>; frames >= 1 (n = p frames): CLIPSIM [p] = (100 / frames) sum_f <img_{p frames + f},
    txt_p> in frame order (lavie_clip_similarity_f32)."""
    _chk32(image_features, text_features)
    if image_features.dim() != 2 or text_features.dim() != 2 or image_features.shape[1] != text_features.shape[1]:
        raise ValueError(f"clip_similarity: features must be [n, d] and [p, d], got {tuple(image_features.shape)} and {tuple(text_features.shape)}")
    n, d = image_features.shape
    p = text_features.shape[0]
    out = _out(out, (p,) if frames else (n, p), torch.float32, image_features.device, "clip_similarity: out")
    _lib.check(_lib.load().lavie_clip_similarity_f32(_p(image_features), _p(text_features), _p(out), n, p, d, int(frames), float(scale),
                                                     _stream()), "lavie_clip_similarity_f32")
    return out


# ------------------------------------------------------------------ FVD: 3-D convolutions, mean over rows, video processor
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def pack_conv3d(weight):
    """nn.Conv3d weight [cout, cin, kt, kh, kw] (fp16, device) -> [cout, kpad]: rows in [kt][kh][kw][cin] order, zero-padded to a
    multiple of 64 halfs (lavie_conv3d_pack)."""
    _chk16(weight)
    if weight.dim() != 5:
        raise ValueError(f"pack_conv3d: weight must be [cout, cin, kt, kh, kw], got {tuple(weight.shape)}")
    cout, cin, kt, kh, kw = weight.shape
    lib = _lib.load()
    halfs = lib.lavie_conv3d_packed_halfs(cout, cin, kt, kh, kw)
    if halfs < 0:
        raise ValueError(f"pack_conv3d: shape {tuple(weight.shape)} is outside what lavie_conv3d_pack takes")
    out = torch.empty((cout, halfs // cout), dtype=torch.float16, device=weight.device)
    _lib.check(lib.lavie_conv3d_pack(_p(weight), _p(out), cout, cin, kt, kh, kw, _stream()), "lavie_conv3d_pack")
    return out


def pack_conv3d_fold(weight, gamma, beta, mean, var, eps=1e-5, out=None, shift=None):
    """nn.Conv3d weight fp32 [cout, cin, kt, kh, kw] with the BatchNorm3d (gamma, beta, running mean, running var: fp32 [cout]) behind
    it folded in -> (pack_conv3d's image of fp16(weight * gamma / sqrt(var + eps)), one rounding from the double product, and the fp32
    bias beta - mean * gamma / sqrt(var + eps)) (lavie_conv3d_fold_pack_f32)."""
    _chk32(weight, gamma, beta, mean, var)
    if weight.dim() != 5:
        raise ValueError(f"pack_conv3d_fold: weight must be [cout, cin, kt, kh, kw], got {tuple(weight.shape)}")
    cout, cin, kt, kh, kw = weight.shape
    if any(t is None or tuple(t.shape) != (cout,) for t in (gamma, beta, mean, var)):
        raise ValueError(f"pack_conv3d_fold: gamma, beta, mean and var must each be fp32 [{cout}]")
    lib = _lib.load()
    halfs = lib.lavie_conv3d_packed_halfs(cout, cin, kt, kh, kw)
    if halfs < 0:
        raise ValueError(f"pack_conv3d_fold: shape {tuple(weight.shape)} is outside what lavie_conv3d_fold_pack_f32 takes")
    out = _out(out, (cout, halfs // cout), torch.float16, weight.device, "pack_conv3d_fold: out")
    shift = _out(shift, (cout,), torch.float32, weight.device, "pack_conv3d_fold: shift")
    _lib.check(lib.lavie_conv3d_fold_pack_f32(_p(weight), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), _p(out), _p(shift), cout, cin,
                                              kt, kh, kw, _stream()), "lavie_conv3d_fold_pack_f32")
    return out, shift


def conv3d(x, wp, bias, ksize=3, stride=1, residual=None, relu=False, out=None):
    """relu?(conv3d(x) + bias + residual) on channels-last rows (lavie_conv3d_f16): x fp16 [n, t, h, w, cin], wp from pack_conv3d,
    bias fp32 [cout], residual fp16 [n, to, ho, wo, cout] -> fp16 [n, to, ho, wo, cout].  ksize 3 (pad 1, stride 1 | 2) or 1 (stride 2)."""
    _chk16(x, wp, residual)
    _chk32(bias)
    if x.dim() != 5 or wp.dim() != 2 or bias.dim() != 1:
        raise ValueError(f"conv3d: x must be [n, t, h, w, cin], wp [cout, kpad] and bias [cout], got {tuple(x.shape)}, {tuple(wp.shape)}, "
                         f"{tuple(bias.shape)}")
    n, t, h, w, cin = x.shape
    cout = wp.shape[0]
    if bias.numel() != cout or wp.shape[1] != -(-(ksize ** 3 * cin) // 64) * 64:
        raise ValueError(f"conv3d: wp {tuple(wp.shape)} and bias {tuple(bias.shape)} do not belong to a ({ksize},{ksize},{ksize}) conv "
                         f"{cin} -> {cout}")
    if stride < 1 or min(n, t, h, w) < 1:
        raise ValueError(f"conv3d: bad stride {stride} or empty extent in {tuple(x.shape)}")
    shape = (n, (t - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1, cout)
    if residual is not None and tuple(residual.shape) != shape:
        raise ValueError(f"conv3d: residual must be {shape}, got {tuple(residual.shape)}")
    y = _out(out, shape, torch.float16, x.device, "conv3d: out")
    _lib.check(_lib.load().lavie_conv3d_f16(_p(x), _p(wp), _p(bias), _p(residual), int(bool(relu)), _p(y), n, t, h, w, cin, cout, int(ksize),
                                            int(stride), _stream()), "lavie_conv3d_f16")
    return y


def _stem_strides(pixels, layout, what):
    """(n, t, h, w, stride_n, stride_t, stride_c) of a pixel tensor read in place: rows contiguous, the other axes at any stride that
    holds a plane"""
    if layout not in ("ncthw", "ntchw"):
        raise ValueError(f"{what}: layout {layout!r} is neither 'ncthw' nor 'ntchw'")
    if not (pixels.is_cuda and pixels.dtype in (torch.float16, torch.float32) and pixels.dim() == 5):
        raise ValueError(f"{what}: pixels must be a 5-D fp16 or fp32 device tensor")
    v = pixels if layout == "ntchw" else pixels.permute(0, 2, 1, 3, 4)
    n, t, c, h, w = v.shape
    if c != 3:
        raise ValueError(f"{what}: pixels must have 3 channels ({layout}), got {tuple(pixels.shape)}")
    if min(n, t, h, w) < 1:
        raise ValueError(f"{what}: empty extent in {tuple(pixels.shape)}")
    if v.stride(4) != 1 or v.stride(3) != w or min(v.stride(0), v.stride(1), v.stride(2)) < h * w:
        raise ValueError(f"{what}: the h x w planes of pixels must be contiguous and must not overlap (strides {tuple(pixels.stride())})")
    return n, t, h, w, v.stride(0), v.stride(1), v.stride(2)


def conv3d_stem(pixels, wp, bias, relu=True, layout="ncthw", out=None):
    """The (3,7,7) / (1,2,2) / (1,3,3) stem conv 3 -> 64 (lavie_conv3d_stem_f16): pixels fp16 or fp32, [n, 3, t, h, w] ('ncthw') or
    [n, t, 3, h, w] ('ntchw'), read in place through their strides; wp = pack_conv3d of [64, 3, 3, 7, 7]; bias fp32 [64]
    -> fp16 rows [n, t, ceil(h / 2), ceil(w / 2), 64]."""
    _chk16(wp)
    _chk32(bias)
    n, t, h, w, sn, st, sc = _stem_strides(pixels, layout, "conv3d_stem")
    if tuple(wp.shape) != (64, 448) or bias.numel() != 64:
        raise ValueError(f"conv3d_stem: wp must be the pack_conv3d image [64, 448] of [64, 3, 3, 7, 7] and bias [64], got {tuple(wp.shape)}, "
                         f"{tuple(bias.shape)}")
    y = _out(out, (n, t, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64), torch.float16, pixels.device, "conv3d_stem: out")
    _lib.check(_lib.load().lavie_conv3d_stem_f16(_p(pixels), int(pixels.dtype == torch.float32), sn, st, sc, _p(wp), _p(bias), int(bool(relu)),
                                                 _p(y), n, t, h, w, _stream()), "lavie_conv3d_stem_f16")
    return y


def mean_rows(x, out=None):
    """fp16 [n, rows, c] -> fp32 [n, c], the mean over rows in a fixed order (lavie_mean_rows_f32)."""
    _chk16(x)
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"mean_rows: x must be a non-empty [n, rows, c], got {tuple(x.shape)}")
    n, rows, c = x.shape
    out = _out(out, (n, c), torch.float32, x.device, "mean_rows: out")
    _lib.check(_lib.load().lavie_mean_rows_f32(_p(x), _p(out), n, rows, c, _stream()), "lavie_mean_rows_f32")
    return out


def video_preprocess(frames, crop=270, size=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32, out=None):
    """Per frame: centre crop of crop x crop, Pillow's bilinear resize to size x size, (v / 255 - mean) / std
    (lavie_video_preprocess_u8): frames uint8 [b, h, w, 3] with unit stride over (w, 3) -> [b, 3, size, size], fp32 with the bits of
    Pillow + fp32 normalisation, or fp16, one rounding of those."""
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
        raise ValueError("video_preprocess: frames must be a uint8 device tensor [b, h, w, 3]")
    b, h, w, _ = frames.shape
    if b < 1:
        raise ValueError("video_preprocess: empty batch")
    if frames.stride(3) != 1 or frames.stride(2) != 3:
        raise ValueError("video_preprocess: the pixels of a row must be contiguous")
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"video_preprocess: dtype {dtype} is not fp32 or fp16")
    lib = _lib.load()
    mean3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    std3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    nbytes = lib.lavie_video_preprocess_workspace_bytes(b, h, w, int(crop), int(size))
    if nbytes < 0:
        _lib.check(-1, "lavie_video_preprocess_workspace_bytes")
    with torch.cuda.device(frames.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=frames.device)
        out = _out(out, (b, 3, int(size), int(size)), dtype, frames.device, "video_preprocess: out")
        _lib.check(lib.lavie_video_preprocess_u8(_p(frames), b, h, w, frames.stride(1), frames.stride(0), _p(out), int(dtype == torch.float32),
                                                 int(crop), int(size), mean3, std3, _p(ws), nbytes, _stream()), "lavie_video_preprocess_u8")
    return out
