"""CPU: the host side of the VAE edge convolutions: the two 1x1 folds are exact, the new C-ABI entry points refuse
bad channel counts / dtype flags / null tensors / pad_lo = 0 at stride 1 before any HIP call (so they can be exercised without a
GPU), the constructor switch validates, and the built library carries the conv_edge kernels and still passes the packed-FP32
op_sel disassembly guard."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from lavie_amd import _lib


def test_fold_quant_conv_is_the_conv_pair():
    from lavie_amd.vae_hip import fold_quant_conv
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 16, 7, 9, generator=g, dtype=torch.float64)
    w_out, b_out = torch.randn(8, 16, 3, 3, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    w_q, b_q = torch.randn(8, 8, 1, 1, generator=g, dtype=torch.float64), torch.randn(8, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.conv2d(x, w_out, b_out, padding=1), w_q, b_q)
    w, b = fold_quant_conv(w_out.float(), b_out.float(), w_q.float(), b_q.float())
    assert w.shape == (8, 16, 3, 3) and w.dtype == torch.float32
    got = F.conv2d(x, w.double(), b.double(), padding=1)
    assert ((got - ref).norm() / ref.norm()).item() < 1e-6


def test_fold_post_quant_conv_is_the_conv_pair_at_the_border_too():
    from lavie_amd.vae_hip import fold_post_quant_conv
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2, 4, 6, 5, generator=g, dtype=torch.float64)
    w_pq, b_pq = torch.randn(4, 4, 1, 1, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64) * 3
    w_in, b_in = torch.randn(32, 4, 3, 3, generator=g, dtype=torch.float64), torch.randn(32, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.conv2d(z, w_pq, b_pq), w_in, b_in, padding=1)
    w, tb = fold_post_quant_conv(w_in.float(), w_pq.float(), b_pq.float())
    assert w.shape == (32, 4, 3, 3) and tb.shape == (9, 32)
    # tap_bias as the kernel applies it: tap (ky, kx) contributes where it falls inside the image
    inside = F.conv2d(torch.ones(2, 1, 6, 5, dtype=torch.float64), tb.double().t().reshape(32, 1, 3, 3).contiguous(), padding=1)
    got = F.conv2d(z, w.double(), b_in, padding=1) + inside
    border = torch.ones(6, 5, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    for sel in (border, ~border):
        assert ((got[:, :, sel] - ref[:, :, sel]).norm() / ref[:, :, sel].norm()).item() < 1e-6
    # a bias added everywhere (the naive fold) is wrong at the border by far more than that
    naive = F.conv2d(z, w.double(), b_in + tb.double().sum(0), padding=1)
    assert ((naive[:, :, border] - ref[:, :, border]).norm() / ref[:, :, border].norm()).item() > 1e-2


def test_constructor_switch():
    from lavie_amd import vae_hip
    from lavie_amd.autoencoder_kl import AutoencoderKL
    vae = AutoencoderKL(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8)
    assert vae_hip.DEFAULT_EDGES in ("engine", "stock")
    assert vae_hip.HipAutoencoderKL(vae).edges == vae_hip.DEFAULT_EDGES
    assert vae_hip.HipAutoencoderKL(vae, edges="stock").edges == "stock"
    assert vae_hip.HipAutoencoderKL(vae, edges="engine", attention="sdpa").attention == "sdpa"
    with pytest.raises(ValueError, match="edges"):
        vae_hip.HipAutoencoderKL(vae, edges="miopen")


def test_entry_points_refuse_before_any_launch():
    """Every refusal below comes from an argument check in front of the first HIP call: it needs no device, names the argument, and
    returns a negative status."""
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    d = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc, needle):
        assert rc < 0
        msg = lib.lavie_last_error().decode()
        assert needle in msg, msg

    refused(lib.lavie_conv_edge_in_f16(d, 0, d, None, None, d, 1, 9, 4, 4, 128, None), "Cin=9")
    refused(lib.lavie_conv_edge_in_f16(d, 0, d, None, None, d, 1, 0, 4, 4, 128, None), "Cin=0")
    refused(lib.lavie_conv_edge_in_f16(d, 0, d, None, None, d, 1, 4, 4, 4, 100, None), "Cout=100")
    refused(lib.lavie_conv_edge_in_f16(d, 2, d, None, None, d, 1, 4, 4, 4, 128, None), "x_dtype=2")
    refused(lib.lavie_conv_edge_in_f16(None, 0, d, None, None, d, 1, 4, 4, 4, 128, None), "null")
    refused(lib.lavie_conv_edge_in_f16(d, 0, d, None, None, d, 1, 8, 4, 4, 1024, None), "LDS")
    refused(lib.lavie_pack_conv_edge_in_f16(d, d, 128, 9, None), "Cin=9")
    refused(lib.lavie_conv_edge_out_f16(d, d, None, d, 0, 1, 128, 4, 4, 9, None), "Cout=9")
    refused(lib.lavie_conv_edge_out_f16(d, d, None, d, 0, 1, 100, 4, 4, 3, None), "Cin=100")
    refused(lib.lavie_conv_edge_out_f16(d, d, None, d, 3, 1, 128, 4, 4, 3, None), "y_dtype=3")
    refused(lib.lavie_conv_edge_out_f16(d, None, None, d, 0, 1, 128, 4, 4, 3, None), "null")
    refused(lib.lavie_pack_conv_edge_out_f16(d, d, 9, 128, None), "Cout=9")
    assert lib.lavie_conv_edge_out_image_halfs(128) == 9 * 4 * 256 and lib.lavie_conv_edge_out_image_halfs(40) == 9 * 2 * 256
    assert lib.lavie_conv_edge_out_image_halfs(100) == 0 and lib.lavie_conv_edge_out_image_halfs(0) == 0
    refused(lib.lavie_conv3x3_down_f16(d, 64, d, None, d, 1, 8, 8, 64, 1, 0, d, None), "pad_lo=0")
    refused(lib.lavie_conv3x3_down_f16(d, 64, d, None, d, 1, 8, 8, 64, 2, 2, d, None), "pad_lo=2")
    refused(lib.lavie_conv3x3_down_f16(d, 64, d, None, d, 1, 8, 8, 64, 3, 1, d, None), "stride=3")
    refused(lib.lavie_conv3x3_down_f16(d, 60, d, None, d, 1, 8, 8, 64, 2, 0, d, None), "C=60")
    refused(lib.lavie_conv3x3_down_f16(d, 64, d, None, d, 1, 1, 8, 64, 2, 0, d, None), "1x8")
    refused(lib.lavie_conv3x3_down_f16(d, 64, d, None, d, 1, 8, 8, 64, 2, 0, None, None), "null")


def test_library_carries_the_edge_kernels_and_passes_the_op_sel_guard():
    import test_host_logic
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"conv_edge_in_kernel", b"conv_edge_out_kernel", b"pack_conv_edge_in_kernel", b"pack_conv_edge_out_kernel"):
        assert name in blob, name
    test_host_logic.test_device_code_has_no_op_sel_modified_packed_fp32()
