"""-m gpu: the forward's end and glue kernels per element (tests/opcheck.py), each through the entry point of its own: the
time-embedding chain (timestep_sinusoid, gemv, add_class_emb_silu), the NCFHW boundary (conv_in, conv_out4<5>, conv_out4<6>, the general
conv_out) and the load-time kernels (ln_fold, pack_conv_in, the unchunked pack_conv3x3, pack_geglu_vec, copy_rows, f16_to_f32,
fill_relpos_bias).  Same check as tests/test_gpu_ops_local.py: guarded operands, NaN then finite poison, inputs unchanged, two runs
bit-equal, |got - ref64| <= u |ref64| + c scale at every element (u = 2^-23 for fp32 outputs); pure moves and exact conversions bit
for bit, a sub-rectangle with every element around it still poisoned.  None of these kernels depends on the GEMM choice, so the
library is loaded once and nothing is forced.  Every refusal leaves every guard band intact."""
import pytest
import torch

import opcases as C
import opcheck as oc

pytestmark = pytest.mark.gpu
FAMILIES = C.ends_cases()
f16, f32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import _lib, ops as o
    _lib.load()
    return o


def family(name):
    return pytest.mark.parametrize("case", FAMILIES[name], ids=[c.name for c in FAMILIES[name]])


def check(ops, case):
    oc.check_case(ops, case, sync=torch.cuda.synchronize)


def refused(fn, inputs, outputs, match, alias=None):
    with pytest.raises(RuntimeError, match=match):
        oc.run_guarded(fn, inputs, outputs, alias=alias, sync=torch.cuda.synchronize)


@family("conv_out")
def test_conv_out(ops, case):
    check(ops, case)


@pytest.mark.parametrize("cin,cout", C.CONV_OUT_REFUSED)
def test_conv_out_refused(ops, cin, cout):
    ins = {"x": torch.zeros(2, cin, dtype=f16), "wp": torch.zeros(cout, 9 * cin, dtype=f16), "b": torch.zeros(cout)}
    refused(lambda i, o: ops.conv_out(i["x"], i["wp"], i["b"], 1, 1, 1, 2, out=o["y"]), ins, {"y": ((1, cout, 1, 1, 2), f16)}, "conv_out")


@family("conv_in")
def test_conv_in(ops, case):
    check(ops, case)


@pytest.mark.parametrize("cin,cout", C.CONV_IN_REFUSED)
def test_conv_in_refused(ops, cin, cout):
    assert cin % 2 or cout % 8 or not C.conv_in_fits(cin, cout)
    ins = {"x": torch.zeros(1, cin, 1, 1, 2, dtype=f16), "wp": torch.zeros(9 * cin * cout, dtype=f16), "b": torch.zeros(cout)}
    refused(lambda i, o: ops.conv_in(i["x"], i["wp"], i["b"], cout, out=o["y"]), ins, {"y": ((2, cout), f16)}, "conv_in")
    if cin % 2 or cout % 8:
        refused(lambda i, o: ops.pack_conv_in(i["w"], out=o["y"]), {"w": torch.zeros(cout, cin, 3, 3, dtype=f16)}, {"y": ((9 * cin * cout,), f16)},
                "pack_conv_in")


@family("pack")
def test_moves_and_conversions(ops, case):
    check(ops, case)


def test_pack_geglu_vec_refused(ops):
    refused(lambda i, o: ops.pack_geglu_vec(i["v"], out=o["y"]), {"v": torch.zeros(48)}, {"y": ((48,), f32)}, "multiple of 32")


@pytest.mark.parametrize("shape", C.COPY_ROWS_REFUSED)
def test_copy_rows_refused(ops, shape):
    nrows, cols, ld_src, ld_dst, col0 = shape
    refused(lambda i, o: ops.copy_rows(i["src"], o["y"], col0, cols=cols), {"src": torch.zeros(nrows, ld_src, dtype=f16)}, {"y": ((nrows, ld_dst), f16)},
            "copy_rows")


@family("ln_fold")
def test_ln_fold(ops, case):
    check(ops, case)


@family("gemv")
def test_gemv(ops, case):
    check(ops, case)


@pytest.mark.parametrize("B,N,K", C.GEMV_REFUSED)
def test_gemv_refused(ops, B, N, K):
    ins = {"x": torch.zeros(B, K), "w": torch.zeros(N, K, dtype=f16), "bias": torch.zeros(N)}
    refused(lambda i, o: ops.gemv(i["x"], i["w"], i["bias"], out=o["y"]), ins, {"y": ((B, N), f32)}, "gemv")


@family("timestep_sinusoid")
def test_timestep_sinusoid(ops, case):
    check(ops, case)


@family("add_class_emb_silu")
def test_add_class_emb_silu(ops, case):
    check(ops, case)


@pytest.mark.parametrize("B,N,labels", C.CLASS_EMB_REFUSED)
def test_add_class_emb_silu_refused(ops, B, N, labels):
    ins = {"emb": torch.zeros(B, N), "table": torch.zeros(5, N, dtype=f16)}
    refused(lambda i, o: ops.add_class_emb_silu(o["y"], i["table"], labels), ins, {"y": ((B, N), f32)}, "add_class_emb_silu", alias={"y": "emb"})


@family("fill_relpos_bias")
def test_fill_relpos_bias(ops, case):
    check(ops, case)
