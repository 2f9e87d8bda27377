"""VAE encoder and decoder on the engine's operators: the 3x3 convolutions, GroupNorm + SiLU, nearest-x2
upsampling and the linear projections of `AutoencoderKL.encode` / `.decode` run through the C-ABI kernels of liblavie_hip.so
(`lavie_conv3x3_f16` with the fused shortcut / folded upsample, `lavie_group_norm_f16`, `lavie_linear_f16`) on channels-last fp16
rows, the mid block's single-head attention product can run through `lavie_attention_f16` (head dims 512 / 256:
csrc/attention_wide.hip), and the 3 / 4 / 8-channel edge convolutions and the encoder's asymmetric stride-2 downsamplers can run
through `lavie_conv_edge_in_f16` / `lavie_conv_edge_out_f16` (csrc/conv_edge.hip) and `lavie_conv3x3_down_f16`.  What stays on
stock PyTorch ops is by the two constructor switches only: with attention="engine" and edges="engine" no stock convolution and no
stock attention runs in `encode` or `decode`, and both are bit-reproducible.

`HipAutoencoderKL(vae, attention="engine" | "sdpa", edges="engine" | "stock")`.
attention: "engine" takes q | k | v as column slices of the fused projection output
(one launch, nb = n, lq = lk = h w, heads = 1); "sdpa" is `F.scaled_dot_product_attention`, kept so both can be timed in one
process (tools/bench_vae_attention.py) and for mid widths the kernel does not serve, where "engine" falls back to it with a
one-time warning.  The default is the measured faster one at the production shape (profiles/vae_attention.json).
edges: "engine" reads the caller's NCHW image / latent in its own dtype (fp16 or fp32) and writes `.sample` as NCHW in the wrapped
VAE's dtype and the moments as fp32 straight from the kernels, with no layout copy or cast in between; the two 1x1 convolutions
are folded on the host in fp32 at pack time and rounded to fp16 once: quant_conv into the encoder's conv_out (W' = W_quant W_out
per tap, b' = W_quant b_out + b_quant), post_quant_conv into the decoder's conv_in (W'[co, c, tap] = sum_m W_in[co, m, tap]
W_pq[m, c]; its bias becomes a per-tap bias, added for the taps inside the image only, because the stock module zero-pads AFTER
post_quant_conv).  "stock" is the `torch.nn.Conv2d` path (MIOpen) as before, kept so both can be timed in one process
(tools/bench_vae_edges.py -> profiles/vae_edges.json); DEFAULT_EDGES is "engine": measured at or below "stock" in every launch
at its production shape, in the decode and in the encode.

Why: in the full cascade (tools/bench_cascade.py) the stock fp32 decode of 61 frames at 1280x2048 took 321 s of 525 s.
`HipAutoencoderKL(vae)` wraps a `lavie_amd.autoencoder_kl.AutoencoderKL` (same weights, same `decode(z).sample` /
`encode` / `config` surface) and can be passed wherever the pipelines take a `vae`.  Parity: against the wrapped stock module
(tests/test_gpu_cascade.py); the stock module itself is parity-unpinned (see its header)."""
import warnings
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import ops


def _rows(x: torch.Tensor) -> torch.Tensor:
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


class _Res:
    def __init__(self, r, dev):
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        h16 = lambda t: t.detach().to(dev, torch.float16).contiguous()
        self.cin, self.cout = r.conv1.in_channels, r.conv1.out_channels
        self.g1, self.b1, self.g2, self.b2 = f32(r.norm1.weight), f32(r.norm1.bias), f32(r.norm2.weight), f32(r.norm2.bias)
        self.w1, self.c1 = ops.pack_conv3x3(h16(r.conv1.weight)), f32(r.conv1.bias)
        if r.conv_shortcut is None:
            self.w2, self.c2, self.short = ops.pack_conv3x3(h16(r.conv2.weight)), f32(r.conv2.bias), False
        else:       # 1x1 shortcut fused as extra K columns of conv2 (as the UNet's resnets do)
            self.w2 = ops.pack_conv3x3(h16(r.conv2.weight), h16(r.conv_shortcut.weight))
            self.c2, self.short = f32(r.conv2.bias + r.conv_shortcut.bias), True

    def __call__(self, x, n, h, w):
        a = ops.group_norm(x, self.g1, self.b1, n, 32, 1e-6, True)
        a = ops.conv3x3(a, self.w1, self.c1, n, h, w)
        a = ops.group_norm(a, self.g2, self.b2, n, 32, 1e-6, True)
        if self.short:
            return ops.conv3x3(a, self.w2, self.c2, n, h, w, sc1=x)
        return ops.conv3x3(a, self.w2, self.c2, n, h, w, residual=x)


ENGINE_ATTENTION_WIDTHS = (256, 512)      # head dims lavie_attention_f16 serves beyond its <= 160 range
DEFAULT_ATTENTION = "engine"              # tools/bench_vae_attention.py at NB 1 x 163,840 x 512: 55.2 ms against 178.6 ms (SDPA)
DEFAULT_EDGES = "engine"                  # tools/bench_vae_edges.py: at or below "stock" in every launch, decode 85.6 / 87.8 ms, encode 15.8 / 18.3 ms
EDGE_MAX_CHANNELS = 8                     # the narrow side of lavie_conv_edge_in_f16 / lavie_conv_edge_out_f16


def _edge_image(x: torch.Tensor) -> torch.Tensor:
    """the caller's NCHW tensor as the edge kernel reads it: in place when it is contiguous fp16 / fp32"""
    return (x if x.dtype in (torch.float16, torch.float32) else x.float()).contiguous()


def fold_quant_conv(w_out, b_out, w_quant, b_quant):
    """quant_conv (1x1, behind) folded into the encoder's conv_out, fp32: (W' [M, C, 3, 3], b' [M]) with
    W' = W_quant W_out per tap and b' = W_quant b_out + b_quant."""
    wq = w_quant.float().reshape(w_quant.shape[0], w_quant.shape[1])
    return torch.einsum("om,mcyx->ocyx", wq, w_out.float()).contiguous(), (wq @ b_out.float() + b_quant.float()).contiguous()


def fold_post_quant_conv(w_in, w_pq, b_pq):
    """post_quant_conv (1x1, in front) folded into the decoder's conv_in, fp32: (W' [C, L, 3, 3], tap_bias [9, C]) with
    W'[co, c, tap] = sum_m W_in[co, m, tap] W_pq[m, c] and tap_bias[tap][co] = sum_m W_in[co, m, tap] b_pq[m]: the stock pair
    zero-pads between the two convolutions, so a pixel sees b_pq through the taps that fall inside the image only."""
    wi, wp = w_in.float(), w_pq.float().reshape(w_pq.shape[0], w_pq.shape[1])
    return (torch.einsum("omyx,mc->ocyx", wi, wp).contiguous(),
            torch.einsum("omyx,m->yxo", wi, b_pq.float()).reshape(9, -1).contiguous())


class HipAutoencoderKL(torch.nn.Module):
    def __init__(self, vae, attention=None, edges=None):
        super().__init__()
        attention = DEFAULT_ATTENTION if attention is None else attention
        if attention not in ("engine", "sdpa"):
            raise ValueError(f"HipAutoencoderKL: attention must be 'engine' or 'sdpa', got {attention!r}")
        edges = DEFAULT_EDGES if edges is None else edges
        if edges not in ("engine", "stock"):
            raise ValueError(f"HipAutoencoderKL: edges must be 'engine' or 'stock', got {edges!r}")
        self.attention = attention
        self.edges = edges
        self._warned_widths = set()
        self.vae = vae                                   # the stock module: encode(), the small edge convolutions, config
        self.config = vae.config
        self._packed = None
        self._packed_enc = None

    def _mid(self, p, x, n, h, w, c):
        """mid block: resnet, single-head attention (GroupNorm and the four projections on the engine; the (h w) x (h w)
        product with head dim C on the engine or on stock SDPA, see the module docstring), resnet."""
        x = p.mid[0](x, n, h, w)
        a = ops.group_norm(x, p.att_g, p.att_b, n, 32, 1e-6, False)
        qkv = ops.linear(a, p.att_wqkv, bias=p.att_bqkv)
        engine = self.attention == "engine"
        if engine and c not in ENGINE_ATTENTION_WIDTHS:
            if c not in self._warned_widths:
                self._warned_widths.add(c)
                warnings.warn(f"HipAutoencoderKL: mid-block width {c} is not served by the engine attention "
                              f"(head dims {ENGINE_ATTENTION_WIDTHS}); using scaled_dot_product_attention")
            engine = False
        if engine:
            o = ops.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], n, h * w, h * w, 1)
        else:
            t = qkv.reshape(n, h * w, 3, c)
            o = F.scaled_dot_product_attention(t[:, None, :, 0], t[:, None, :, 1], t[:, None, :, 2])[:, 0]
            o = o.reshape(n * h * w, c).contiguous()
        x = ops.linear(o, p.att_wo, bias=p.att_bo, residual=x)
        return p.mid[1](x, n, h, w)

    @staticmethod
    def _pack_mid(mid, dev):
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        h16 = lambda t: t.detach().to(dev, torch.float16).contiguous()
        att = mid.attentions[0]
        p = SimpleNamespace()
        p.mid = [_Res(mid.resnets[0], dev), _Res(mid.resnets[1], dev)]
        p.att_g, p.att_b = f32(att.group_norm.weight), f32(att.group_norm.bias)
        p.att_wqkv = h16(torch.cat([att.query.weight, att.key.weight, att.value.weight], 0))
        p.att_bqkv = f32(torch.cat([att.query.bias, att.key.bias, att.value.bias], 0))
        p.att_wo, p.att_bo = h16(att.proj_attn.weight), f32(att.proj_attn.bias)
        return p

    @torch.no_grad()
    def encode(self, x: torch.Tensor):
        """Encoder resnets / mid block / output norm on the engine.  edges="engine": the input convolution reads x in place
        (conv_edge_in), the stride-2 downsamplers go rows -> rows through the asymmetric-pad gather conv, and conv_out with
        quant_conv folded into it writes the fp32 moments in one conv_edge_out launch.  edges="stock": those convolutions run as
        torch.nn.Conv2d with a rows -> NCHW -> rows round trip around each."""
        from .autoencoder_kl import DiagonalGaussianDistribution
        dev = x.device
        e = self.vae.encoder
        if self._packed_enc is None or self._packed_enc[0] != dev:
            f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
            h16 = lambda t: t.detach().to(dev, torch.float16).contiguous()
            p = self._pack_mid(e.mid_block, dev)
            p.downs = [[_Res(r, dev) for r in blk.resnets] for blk in e.down_blocks]
            p.out_g, p.out_b = f32(e.conv_norm_out.weight), f32(e.conv_norm_out.bias)
            if self.edges == "engine":
                q = self.vae.quant_conv
                self._check_edges(e.conv_in.in_channels, q.out_channels)
                p.in_w, p.in_b = ops.pack_conv_edge_in(h16(e.conv_in.weight)), f32(e.conv_in.bias)
                p.down_w = [(ops.pack_conv3x3(h16(blk.downsamplers[0].conv.weight)), f32(blk.downsamplers[0].conv.bias))
                            if hasattr(blk, "downsamplers") else None for blk in e.down_blocks]
                mom_w, p.mom_b = fold_quant_conv(f32(e.conv_out.weight), f32(e.conv_out.bias), f32(q.weight), f32(q.bias))
                p.mom_w, p.mom_c = ops.pack_conv_edge_out(h16(mom_w)), q.out_channels     # folded in fp32, rounded to fp16 once
            self._packed_enc = (dev, p)
        p = self._packed_enc[1]
        if self.edges == "engine":
            x = _edge_image(x)
            n, _, h, w = x.shape
            c = e.conv_in.out_channels
            r = ops.conv_edge_in(x, p.in_w, p.in_b, c)
            for res, down in zip(p.downs, p.down_w):
                for rb in res:
                    r = rb(r, n, h, w)
                c = res[-1].cout
                if down is not None:
                    r = ops.conv3x3(r, down[0], down[1], n, h, w, stride=2, pad=(0, 1))
                    h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
            r = self._mid(p, r, n, h, w, c)
            r = ops.group_norm(r, p.out_g, p.out_b, n, 32, 1e-6, True)
            moments = ops.conv_edge_out(r, p.mom_w, p.mom_b, n, h, w, p.mom_c, torch.float32)
            return SimpleNamespace(latent_dist=DiagonalGaussianDistribution(moments))
        wdt = next(self.vae.parameters()).dtype
        t = e.conv_in(x.to(wdt)).to(torch.float16)
        n, c, h, w = t.shape
        r = _rows(t)
        for blk, res in zip(e.down_blocks, p.downs):
            for rb in res:
                r = rb(r, n, h, w)
            c = res[-1].cout
            if hasattr(blk, "downsamplers"):
                t = blk.downsamplers[0](r.reshape(n, h, w, c).permute(0, 3, 1, 2).to(wdt)).to(torch.float16)
                n, c, h, w = t.shape
                r = _rows(t)
        r = self._mid(p, r, n, h, w, c)
        r = ops.group_norm(r, p.out_g, p.out_b, n, 32, 1e-6, True)
        moments = self.vae.quant_conv(e.conv_out(r.reshape(n, h, w, c).permute(0, 3, 1, 2).to(wdt)))
        return SimpleNamespace(latent_dist=DiagonalGaussianDistribution(moments.float()))

    def _pack(self, dev):
        d = self.vae.decoder
        groups = d.conv_norm_out.num_groups
        if groups != 32:
            raise NotImplementedError("HipAutoencoderKL: norm_num_groups must be 32")
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        h16 = lambda t: t.detach().to(dev, torch.float16).contiguous()
        p = self._pack_mid(d.mid_block, dev)
        p.ups = []
        for blk in d.up_blocks:
            res = [_Res(r, dev) for r in blk.resnets]
            up = None
            if hasattr(blk, "upsamplers"):
                c = blk.upsamplers[0].conv
                up = (ops.pack_conv3x3(h16(c.weight)), f32(c.bias))
            p.ups.append((res, up))
        p.out_g, p.out_b = f32(d.conv_norm_out.weight), f32(d.conv_norm_out.bias)
        if self.edges == "engine":
            pq = self.vae.post_quant_conv
            self._check_edges(pq.in_channels, d.conv_out.out_channels)
            in_w, p.in_tap = fold_post_quant_conv(f32(d.conv_in.weight), f32(pq.weight), f32(pq.bias))
            p.in_w, p.in_b = ops.pack_conv_edge_in(h16(in_w)), f32(d.conv_in.bias)            # folded in fp32, rounded to fp16 once
            p.out_w, p.out_bias = ops.pack_conv_edge_out(h16(d.conv_out.weight)), f32(d.conv_out.bias)
        self._packed = (dev, p)
        return p

    @staticmethod
    def _check_edges(narrow_in, narrow_out):
        if narrow_in > EDGE_MAX_CHANNELS or narrow_out > EDGE_MAX_CHANNELS:
            raise NotImplementedError(f"HipAutoencoderKL: edges='engine' serves at most {EDGE_MAX_CHANNELS} image / latent / moment "
                                      f"channels (got {narrow_in} in, {narrow_out} out); use edges='stock'")

    @torch.no_grad()
    def decode(self, z: torch.Tensor):
        dev = z.device
        p = self._packed[1] if self._packed is not None and self._packed[0] == dev else self._pack(dev)
        d = self.vae.decoder
        wdt = next(self.vae.parameters()).dtype
        engine_edges = self.edges == "engine"
        if engine_edges:                                                     # post_quant_conv + conv_in: one launch on z as it is
            z = _edge_image(z)
            (n, _, h, w), c = z.shape, d.conv_in.out_channels
            x = ops.conv_edge_in(z, p.in_w, p.in_b, c, tap_bias=p.in_tap)
        else:
            x = d.conv_in(self.vae.post_quant_conv(z.to(wdt)))               # 4 -> 4 -> C channels: stock ops (K = 36)
            n, c, h, w = x.shape
            x = _rows(x.to(torch.float16))
        x = self._mid(p, x, n, h, w, c)
        for res, up in p.ups:
            for r in res:
                x = r(x, n, h, w)
            if up is not None:
                x = ops.conv3x3(x, up[0], up[1], n, h, w, ups=1)       # nearest x2 folded into the gather
                h, w = 2 * h, 2 * w
        x = ops.group_norm(x, p.out_g, p.out_b, n, 32, 1e-6, True)
        if engine_edges:     # C -> 3 channels, NCHW in the VAE's dtype from the kernel (a bf16 VAE: fp32 from the kernel, then one cast copy)
            odt = wdt if wdt in (torch.float16, torch.float32) else torch.float32
            return SimpleNamespace(sample=ops.conv_edge_out(x, p.out_w, p.out_bias, n, h, w, d.conv_out.out_channels, odt).to(wdt))
        x = x.reshape(n, h, w, -1).permute(0, 3, 1, 2)
        return SimpleNamespace(sample=d.conv_out(x.to(wdt)))             # C -> 3 channels: stock op
