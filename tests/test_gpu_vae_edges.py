"""-m gpu: the VAE's edge convolutions and asymmetric stride-2 downsamplers on the engine, through the C ABI:
the asymmetric-pad stride-2 3x3 conv (lavie_conv3x3_down_f16), conv_edge_in / conv_edge_out (csrc/conv_edge.hip) against
torch.nn.functional in fp32 on the fp16-rounded operands, their refusals, and HipAutoencoderKL(vae, edges="engine"): parity with
the stock module, no stock convolution in encode / decode, bit reproducibility of both and of the whole reduced cascade."""
import pytest
import torch
import torch.nn.functional as F

import golden_util as G
from gpu_util import TOL_OP, f32, h16, q16, rel_l2, rows, unrows

pytestmark = pytest.mark.gpu

TOL_VAE = 1e-2         # the bound of the existing VAE parity tests (tests/test_gpu_cascade.py)


def _conv_case(cout, cin, n, h, w, seed, scale=None):
    g = torch.Generator().manual_seed(seed)
    x = q16(torch.randn(n, cin, h, w, generator=g))
    wt = q16(torch.randn(cout, cin, 3, 3, generator=g) * (scale if scale is not None else (9 * cin) ** -0.5))
    b = torch.randn(cout, generator=g) * 0.5
    return x, wt, b


# ------------------------------------------------------------------ asymmetric stride-2 conv
# 1 x 13 x 18 and 2 x 64 x 96 (the issue's), odd x odd, even x odd, and 3 x 27 x 37: 3 * 13 * 18 = 702 output tokens, a multiple of
# none of the GEMM tiles' row counts (128, 160, 320)
@pytest.mark.parametrize("c", [128, 256, 512])
@pytest.mark.parametrize("n,h,w", [(1, 13, 18), (2, 64, 96), (1, 15, 21), (2, 16, 9), (3, 27, 37)])
def test_asymmetric_stride2_conv(c, n, h, w):
    from lavie_amd import ops
    x, wt, b = _conv_case(c, c, n, h, w, seed=c + h)
    wp = ops.pack_conv3x3(h16(wt))
    xr = h16(rows(x))
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)
    ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    assert ref.shape == (n, c, ho, wo)
    got = ops.conv3x3(xr, wp, f32(b), n, h, w, stride=2, pad=(0, 1))
    assert got.shape == (n * ho * wo, c)
    err = rel_l2(unrows(got.cpu().float(), n, ho, wo), ref)
    print(f"asymmetric stride-2 conv C={c} {n}x{h}x{w}: rel-L2 {err:.3e}")
    assert err < TOL_OP
    # the existing symmetric call on the same operands still matches ITS reference (pad_lo stays 1 by default) ...
    ref_sym = F.conv2d(x, wt, b, stride=2, padding=1)
    got_sym = ops.conv3x3(xr, wp, f32(b), n, h, w, stride=2)
    hs, ws = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert got_sym.shape == (n * hs * ws, c)
    assert rel_l2(unrows(got_sym.cpu().float(), n, hs, ws), ref_sym) < TOL_OP
    # ... and pad=(1, 1) through the new entry point is that same convolution
    assert torch.equal(ops.conv3x3(xr, wp, f32(b), n, h, w, stride=2, pad=(1, 1)), got_sym)


# ------------------------------------------------------------------ conv_edge_in
@pytest.mark.parametrize("cin", [3, 4, 8])
@pytest.mark.parametrize("cout", [128, 512])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("tap", [False, True])
def test_conv_edge_in(cin, cout, dtype, tap):
    from lavie_amd import ops
    n, h, w = 2, 11, 14
    x, wt, b = _conv_case(cout, cin, n, h, w, seed=cin * 7 + cout)
    ref = F.conv2d(x, wt, b, padding=1)
    tb = None
    if tap:
        # a per-tap bias of the size of the output itself: at pixel p it adds sum over the taps of p inside the image = a 3x3
        # conv of an all-ones single-channel image with weights tb[tap][co], zero-padded
        tb = torch.randn(9, cout, generator=torch.Generator().manual_seed(5)) * float(ref.std())
        ref = ref + F.conv2d(torch.ones(n, 1, h, w), tb.t().reshape(cout, 1, 3, 3).contiguous(), padding=1)
    wp = ops.pack_conv_edge_in(h16(wt))
    got = ops.conv_edge_in(x.to("cuda", dtype).contiguous(), wp, f32(b), cout, tap_bias=None if tb is None else f32(tb))
    assert got.shape == (n * h * w, cout) and got.dtype == torch.float16
    got = unrows(got.cpu().float(), n, h, w)
    border = torch.ones(h, w, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    e_border, e_inner = rel_l2(got[:, :, border], ref[:, :, border]), rel_l2(got[:, :, ~border], ref[:, :, ~border])
    print(f"conv_edge_in Cin={cin} Cout={cout} {dtype} tap_bias={tap}: border {e_border:.3e} interior {e_inner:.3e}")
    assert e_border < TOL_OP and e_inner < TOL_OP


# ------------------------------------------------------------------ conv_edge_out
@pytest.mark.parametrize("cin,cout", [(128, 3), (512, 8), (256, 4)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_conv_edge_out(cin, cout, dtype):
    from lavie_amd import ops
    n, h, w = 2, 13, 19            # 494 pixels: not a multiple of the kernel's 16-pixel tile (nor of a workgroup's 64)
    x, wt, b = _conv_case(cout, cin, n, h, w, seed=cin + cout)
    ref = F.conv2d(x, wt, b, padding=1)
    wp = ops.pack_conv_edge_out(h16(wt))
    xr = h16(rows(x))
    got = ops.conv_edge_out(xr, wp, f32(b), n, h, w, cout, dtype)
    assert got.shape == (n, cout, h, w) and got.dtype == dtype
    err = rel_l2(got, ref)
    print(f"conv_edge_out Cin={cin} Cout={cout} {dtype}: rel-L2 {err:.3e}")
    assert err < TOL_OP
    assert torch.equal(ops.conv_edge_out(xr, wp, f32(b), n, h, w, cout, dtype), got)


def test_conv_edge_out_narrow_and_ragged_channel_blocks():
    """Cin that is not a multiple of the 32-channel MFMA step (guarded last block), and one whole workgroup run of tiles."""
    from lavie_amd import ops
    for cin, cout, n, h, w in ((40, 3, 1, 9, 10), (8, 8, 1, 5, 7), (128, 3, 1, 64, 80)):
        x, wt, b = _conv_case(cout, cin, n, h, w, seed=cin)
        got = ops.conv_edge_out(h16(rows(x)), ops.pack_conv_edge_out(h16(wt)), f32(b), n, h, w, cout, torch.float32)
        assert rel_l2(got, F.conv2d(x, wt, b, padding=1)) < TOL_OP


# ------------------------------------------------------------------ refusals
def _launch_classes():
    """per-class launch counts seen by the library's profiling hook between two calls"""
    import ctypes
    from lavie_amd import _lib
    lib = _lib.load()
    n = 11
    launches, ms, fl, by = (ctypes.c_longlong * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    return lib, lambda: lib.lavie_profile_begin(0x7ff, 64), lambda: (lib.lavie_profile_end(None, launches, ms, fl, by), sum(launches))[1]


def test_refusals_name_the_argument_and_launch_nothing():
    from lavie_amd import ops
    lib, begin, end = _launch_classes()
    x9 = torch.zeros(1, 9, 4, 4, device="cuda", dtype=torch.float16)
    w = torch.zeros(2048, device="cuda", dtype=torch.float16)
    b = torch.zeros(64, device="cuda")
    xr = torch.zeros(16, 64, device="cuda", dtype=torch.float16)
    wp = torch.zeros(64, 9 * 64, device="cuda", dtype=torch.float16)
    begin()
    with pytest.raises(RuntimeError, match="Cin=9"):
        ops.conv_edge_in(x9, w, None, 8)
    with pytest.raises(RuntimeError, match="Cin=9"):
        ops.pack_conv_edge_in(torch.zeros(8, 9, 3, 3, device="cuda", dtype=torch.float16))
    with pytest.raises(RuntimeError, match="Cout=9"):
        ops.conv_edge_out(xr, torch.zeros(9 * 2 * 256, device="cuda", dtype=torch.float16), None, 1, 4, 4, 9)
    with pytest.raises(ValueError, match="wp has"):      # a weight image of another width never reaches the device
        ops.conv_edge_out(xr, w, None, 1, 4, 4, 3)
    with pytest.raises(ValueError, match="wp has"):
        ops.conv_edge_in(x9[:, :4].contiguous(), w, None, 128)
    with pytest.raises(ValueError, match="rows"):
        ops.conv_edge_out(xr, torch.zeros(9 * 2 * 256, device="cuda", dtype=torch.float16), None, 1, 4, 5, 3)
    with pytest.raises(RuntimeError, match="Cout=9"):
        ops.pack_conv_edge_out(torch.zeros(9, 64, 3, 3, device="cuda", dtype=torch.float16))
    with pytest.raises(RuntimeError, match="pad_lo"):
        ops.conv3x3(xr, wp, b, 1, 4, 4, stride=1, pad=(0, 1))
    with pytest.raises(RuntimeError, match="Cout=12"):
        ops.conv_edge_in(x9[:, :4].contiguous(), w, None, 12)
    with pytest.raises(RuntimeError, match="Cin=12"):
        ops.conv_edge_out(torch.zeros(16, 12, device="cuda", dtype=torch.float16), w, None, 1, 4, 4, 3)
    assert end() == 0                                    # the profiling hook saw no launch of any class
    begin()
    ops.conv3x3(xr, wp, b, 1, 4, 4, stride=2, pad=(0, 1))
    assert end() == 1                                    # ... and it does see one


# ------------------------------------------------------------------ the module
def _vae(widths, seed, dtype=torch.float32, big_bias=True):
    from lavie_amd.autoencoder_kl import AutoencoderKL
    torch.manual_seed(seed)
    vae = AutoencoderKL(block_out_channels=widths).cuda().eval()
    if big_bias:        # O(1) biases on the two 1x1 convolutions (zero-mean inits leave them ~0.3): the fold must carry them
        with torch.no_grad():
            vae.post_quant_conv.bias.copy_(torch.tensor([1.5, -1.0, 0.75, -2.0]))
            vae.quant_conv.bias.copy_(torch.tensor([1.0, -1.5, 0.5, 2.0, -0.75, 1.25, -2.0, 0.6]))
    return vae.to(dtype)


class _no_stock_conv:
    """torch.nn.Conv2d.forward and torch.nn.functional.conv2d raise while active"""

    def __enter__(self):
        def refuse(*a, **k):
            raise AssertionError("a stock convolution ran")
        self.saved = (torch.nn.Conv2d.forward, F.conv2d)
        torch.nn.Conv2d.forward = refuse
        F.conv2d = refuse
        torch.nn.functional.conv2d = refuse

    def __exit__(self, *exc):
        torch.nn.Conv2d.forward, F.conv2d = self.saved
        torch.nn.functional.conv2d = self.saved[1]


@pytest.mark.parametrize("widths,size", [((128, 256, 512, 512), (2, 8, 16)), ((128, 256, 512), (1, 16, 24))])
def test_engine_edges_decode_matches_stock_module(widths, size):
    from lavie_amd.vae_hip import HipAutoencoderKL
    vae = _vae(widths, 3)
    n, h, w = size
    z = torch.randn(n, 4, h, w, device="cuda")
    ref = vae.decode(z).sample
    hip = HipAutoencoderKL(vae, edges="engine")
    with _no_stock_conv():
        got = hip.decode(z).sample
        again = hip.decode(z).sample
    f = 2 ** (len(widths) - 1)
    assert got.shape == ref.shape == (n, 3, h * f, w * f) and got.dtype == torch.float32        # fp32 weights: an fp32 sample
    err = rel_l2(got, ref)
    print(f"decode edges=engine {widths}: rel-L2 {err:.3e}")
    assert err < TOL_VAE
    assert torch.equal(got, again)
    got16 = hip.decode(z.half()).sample                  # the latent is read in its own dtype
    assert got16.dtype == torch.float32 and rel_l2(got16, ref) < TOL_VAE


def test_engine_edges_decode_fp16_vae_writes_fp16():
    from lavie_amd.vae_hip import HipAutoencoderKL
    vae = _vae((128, 256, 512), 4)
    z = torch.randn(1, 4, 8, 12, device="cuda")
    ref = vae.decode(z).sample
    got = HipAutoencoderKL(vae.half(), edges="engine").decode(z.half()).sample
    assert got.dtype == torch.float16 and got.shape == ref.shape
    assert rel_l2(got, ref) < TOL_VAE


@pytest.mark.parametrize("widths,size", [((128, 256, 512, 512), (2, 64, 96)), ((128, 256, 512), (1, 32, 48)),
                                         ((128, 256, 512, 512), (1, 52, 76))])      # 52 -> 26 -> 13 -> 6: an odd intermediate size
def test_engine_edges_encode_matches_stock_module(widths, size):
    from lavie_amd.vae_hip import HipAutoencoderKL
    vae = _vae(widths, 5)
    n, h, w = size
    x = torch.rand(n, 3, h, w, device="cuda") * 2 - 1
    ref = vae.encode(x).latent_dist
    hip = HipAutoencoderKL(vae, edges="engine")
    with _no_stock_conv():
        got = hip.encode(x).latent_dist
        again = hip.encode(x).latent_dist
    assert got.mean.shape == ref.mean.shape and got.mean.dtype == torch.float32
    e_mean, e_logvar = rel_l2(got.mean, ref.mean), rel_l2(got.logvar, ref.logvar)
    print(f"encode edges=engine {widths} {size}: mean {e_mean:.3e} logvar {e_logvar:.3e}")
    assert e_mean < TOL_VAE and e_logvar < TOL_VAE
    assert torch.equal(got.mean, again.mean) and torch.equal(got.logvar, again.logvar)
    got16 = hip.encode(x.half()).latent_dist             # an fp16 image is read in place too
    assert rel_l2(got16.mean, ref.mean) < TOL_VAE


def test_engine_edges_chain_is_bit_reproducible():
    from lavie_amd.vae_hip import HipAutoencoderKL
    hip = HipAutoencoderKL(_vae((128, 256, 512, 512), 6), edges="engine")
    x = torch.rand(2, 3, 64, 64, device="cuda") * 2 - 1
    with _no_stock_conv():
        a = hip.decode(hip.encode(x).latent_dist.mode()).sample
        b = hip.decode(hip.encode(x).latent_dist.mode()).sample
    assert a.shape == x.shape and torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_stock_edges_path_is_unchanged():
    """edges="stock" is the path HipAutoencoderKL(vae) took before the switch existed: same bound against the wrapped module."""
    from lavie_amd.vae_hip import HipAutoencoderKL
    vae = _vae((128, 256, 512, 512), 7)
    hip = HipAutoencoderKL(vae, edges="stock")
    z = torch.randn(1, 4, 8, 16, device="cuda")
    x = torch.rand(1, 3, 64, 96, device="cuda") * 2 - 1
    assert rel_l2(hip.decode(z).sample, vae.decode(z).sample) < TOL_VAE
    got, ref = hip.encode(x).latent_dist, vae.encode(x).latent_dist
    assert rel_l2(got.mean, ref.mean) < TOL_VAE and rel_l2(got.logvar, ref.logvar) < TOL_VAE
    with pytest.raises(AssertionError, match="stock convolution"), _no_stock_conv():
        hip.decode(z)                                    # the guard of the tests above does catch this path
    with pytest.raises(ValueError, match="edges"):
        HipAutoencoderKL(vae, edges="miopen")


def test_cascade_reduced_models_is_bit_reproducible_with_engine_edges():
    """tests/test_gpu_cascade.py::test_cascade_reduced_models with engine-edge VAEs (widths the engine serves: multiples of 64,
    32 groups, a 256-wide mid block for the engine attention): two runs with the same seeds give the same final frames to the bit,
    which the stock-VAE cascade could only state to 2e-2."""
    from lavie_amd import spec
    from lavie_amd.autoencoder_kl import AutoencoderKL
    from lavie_amd.cascade import text_to_video_cascade
    from lavie_amd.config import UNetConfig
    from lavie_amd.interpolation import UNet3DConditionModel as InterpUNet
    from lavie_amd.interpolation import create_diffusion
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.unet import UNet3DConditionModel
    from lavie_amd.vae_hip import HipAutoencoderKL
    from lavie_amd.vsr import UNet3DVSRModel, VideoUpscalePipeline

    def load(net, cfg, seed):
        net.load_state_dict({k: v.half() for k, v in G.synth16(spec.param_shapes(cfg), seed).items()})
        return net.to("cuda", torch.float16)

    two = dict(down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
    base = load(UNet3DConditionModel(init_weights=False, sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128, **two),
                UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False)), 1)
    interp = load(InterpUNet(init_weights=False, sample_size=8, in_channels=8, block_out_channels=(256, 512), cross_attention_dim=128,
                             use_first_frame=True, **two),
                  UNetConfig(in_channels=8, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False),
                             sparse_causal_attn1=True, temporal_plain=True, ff_before_temporal=True), 2)
    vsr = load(UNet3DVSRModel(init_weights=False, sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
                              layers_per_block=1, down_block_types=("DownBlock3D", "CrossAttnDownBlock3D"),
                              up_block_types=("CrossAttnUpBlock3D", "UpBlock3D"), only_cross_attention=(True, False),
                              down_temporal_idx=(0, 1), mid_temporal=True, up_temporal_idx=(0, 1)),
               UNetConfig(in_channels=7, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(False, True),
                          layers_per_block=1, vsr_blocks=True, only_cross_attention=(True, False), vsr_temporal_modules=True,
                          num_class_embeds=1000), 3)
    torch.manual_seed(0)
    vae = HipAutoencoderKL(AutoencoderKL(block_out_channels=(64, 128, 256, 256), layers_per_block=1).cuda().eval(),
                           attention="engine", edges="engine")
    vsr_vae = HipAutoencoderKL(AutoencoderKL(block_out_channels=(64, 128, 256), layers_per_block=1, scaling_factor=0.08333).cuda().eval(),
                               attention="engine", edges="engine")
    g = torch.Generator().manual_seed(4)
    emb = lambda: torch.randn(1, 77, 128, generator=g)
    pe, ne, ipe, ine, vpe, vne = (emb() for _ in range(6))
    outs = []
    with _no_stock_conv():
        for _ in range(2):
            torch.manual_seed(11)          # the interpolation noise / VAE posterior samples are drawn on the device
            outs.append(text_to_video_cascade(
                VideoGenPipeline(unet=base), interp, create_diffusion("2"), VideoUpscalePipeline(unet=vsr, scheduler=DDIMScheduler()),
                vae, vsr_vae, pe, ne, vpe, vne, ipe, ine, height=64, width=64, base_steps=2, vsr_steps=2, noise_level=20,
                generator=torch.Generator().manual_seed(5)))
    b, i, u, frames = outs[0]
    assert frames.shape == (1, 3, 61, 256, 256) and torch.isfinite(frames).all()
    for got, want in zip(outs[1], outs[0]):
        assert torch.equal(got, want)
