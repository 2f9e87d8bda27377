"""-m gpu: ops.attention and ops.sparse_causal_attention per element (tests/opcheck.py) on every kernel instantiation
lavie_amd/csrc/attention.hip can launch, each at the smallest shape that reaches it (the tables in tests/opcases.py name the
instantiation and the line that decides it), under the logit profiles of opcases.PROFILES: a first key tile far below the
matching key, a dominant key that is the last one, per-tile maxima that creep up below the rescale threshold, and one 16-row
group that holds one row of each kind.  Same check as tests/test_gpu_ops_local.py: guarded operands, NaN then finite poison, two
runs bit-equal, |got - ref64| <= 2^-11 |ref64| + c scale at every element.  Attention does not depend on the GEMM choice, so the
library is loaded once and nothing is forced."""
import pytest
import torch

import opcases as C
import opcheck as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import _lib, ops as o
    _lib.load()
    return o


def check(ops, case):
    oc.check_case(ops, case, sync=torch.cuda.synchronize)


def ident(shape, profile):
    return "x".join(str(v) for v in shape) + "-" + profile


@pytest.mark.parametrize("shape,profile", C.SELF_HARD_CASES, ids=[ident(*sp) for sp in C.SELF_HARD_CASES])
def test_self_attention(ops, shape, profile):
    """(nb, lq = lk, c), 8 heads"""
    check(ops, C.attention_case(*shape, profile=profile))


@pytest.mark.parametrize("shape,profile", C.CROSS_HARD_CASES, ids=[ident(*sp) for sp in C.CROSS_HARD_CASES])
def test_cross_attention(ops, shape, profile):
    """(nb, lq, lk, c, kv_batch_div), 8 heads"""
    nb, lq, lk, c, div = shape
    check(ops, C.attention_case(nb, lq, c, lk=lk, kv_div=div, profile=profile))


@pytest.mark.parametrize("shape,profile", C.WIDE_HARD_CASES, ids=[ident(*sp) for sp in C.WIDE_HARD_CASES])
def test_wide_head_attention(ops, shape, profile):
    """(lq = lk, head dim), one head: attention_wide.hip"""
    check(ops, C.attention_case(1, *shape, heads=1, profile=profile))


@pytest.mark.parametrize("shape,profile", C.SC_HARD_CASES, ids=[ident(*sp) for sp in C.SC_HARD_CASES])
def test_sparse_causal_attention(ops, shape, profile):
    """(frames, tokens per frame, c), two videos, 8 heads"""
    frames, dd, c = shape
    check(ops, C.sparse_causal_case(frames, dd, c=c, profile=profile))
