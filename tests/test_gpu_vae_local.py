"""-m gpu: the autoencoder's own kernels per element (tests/opcheck.py; cases in opcases.vae_cases()) past the first tile of the first
workgroup: attention_wide_kernel<512 | 256> with two query blocks, twelve renumbered workgroups, two heads, kv_batch_div = 2 and four
to six 32-key tiles under the logit profiles laid out for that tile; conv_edge_out_kernel with a second quad per workgroup, the
in-loop break and a one-pixel last tile at 257 x 513, its rolled instantiations and the unrolled ones on interior pixels;
conv_edge_in_kernel with a second grid-stride step; GroupNorm at 128 channels.  Same check as tests/test_gpu_ops_local.py: guarded
operands, NaN then finite poison, two runs bit-equal, |got - ref64| <= u |ref64| + c scale at every element.  None of these kernels
depends on the GEMM choice: the library is loaded once, nothing is forced, each case runs once.  What each case's launch is — kernel
name, grid — is asserted on the CPU by tests/test_gemm_reach_host.py, the paths it walks by tests/test_opcheck_host.py."""
import pytest
import torch

import opcases as C
import opcheck as oc

pytestmark = pytest.mark.gpu

CASES = C.vae_cases()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import _lib, ops as o
    _lib.load()
    return o


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_autoencoder_kernel_past_one_workgroup(ops, case):
    oc.check_case(ops, case, sync=torch.cuda.synchronize)
