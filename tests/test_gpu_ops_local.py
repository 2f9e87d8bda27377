"""-m gpu: the operators of lavie_amd/ops.py per element (tests/opcheck.py, cases in tests/opcases.py).  Each case runs twice on guarded operands —
NaN-poisoned outputs between NaN bands, then finite-poisoned outputs with zero bands around the inputs — and must leave every
band and every input intact, write every output element, give the same bits both times, and meet
|got - ref64| <= 2^-11 |ref64| + c scale at every element ("Per-element operator checks").  No element is excluded."""
import pytest
import torch

import opcases as C
import opcheck as oc

pytestmark = pytest.mark.gpu

VARIANTS = C.VARIANTS
_forced = [0, 0]          # what the fixture set: a case that forces a kernel of its own restores this afterwards


@pytest.fixture(scope="module", params=list(VARIANTS))
def ops(request):
    """The six kernel choices of test_gpu_ops.py: automatic, the 128-row GEMM forced, split-K = 3, the 160x320 ping-pong kernel alone
    and with split-K = 2, the persistent ping-pong kernel.  Where a forced variant does not take a shape the planner falls back and
    the case runs anyway."""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import _lib, ops as o
    lib = _lib.load()
    tile, splits = VARIANTS[request.param]
    lib.lavie_debug_force_tile(tile)
    lib.lavie_debug_force_splits(splits)
    _forced[:] = [tile, splits]
    yield o
    _forced[:] = [0, 0]
    lib.lavie_debug_force_tile(0)
    lib.lavie_debug_force_splits(0)


def check(ops, case, refusal=None):
    """refusal: the case has a shape its kernel is known not to take: the call must raise the RuntimeError with that text (and
    run_guarded checks every band before it lets the error through).  Without it the call must run."""
    if refusal is not None:
        with pytest.raises(RuntimeError, match=refusal):
            check(ops, case)
        return
    oc.check_case(ops, case, forced=_forced, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("opt", C.LINEAR_OPTIONS)
@pytest.mark.parametrize("M,N,K", C.LINEAR_SHAPES)
def test_linear(ops, M, N, K, opt):
    check(ops, C.linear_case(M, N, K, opt))


@pytest.mark.parametrize("M,C_", [(129, 64), (154, 320)])
def test_geglu(ops, M, C_):
    check(ops, C.geglu_case(M, C_))


@pytest.mark.parametrize("M,N,K", [(154, 320, 320), (161, 192, 64)])
def test_linear_lnfold(ops, M, N, K):
    check(ops, C.lnfold_case(M, N, K))


def reach_runs():
    """(case, variant) of the reach tables of opcases.py: a small case under all six variants, a large one under those whose launch
    trace names its target kernel (tests/test_gemm_reach_host.py asserts the traces)"""
    return [pytest.param(c, v, id=f"{c.name}-{v}") for c in C.reach_cases() for v in (c.variants or C.VARIANTS)]


@pytest.mark.parametrize("case,variant", reach_runs())
def test_gemm_reach_case(case, variant):
    """sets its own variant (and puts back what the `ops` fixture of the surrounding tests had set)"""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import ops as o
    with C.forced(*C.VARIANTS[variant], tuple(_forced)):
        oc.check_case(o, case, forced=C.VARIANTS[variant], sync=torch.cuda.synchronize)


@pytest.mark.parametrize("taps", [3, 5])
@pytest.mark.parametrize("b,cin,cout,f,d", C.TCONV_FORCED)
def test_temporal_conv_halo_patch(ops, b, cin, cout, f, d, taps):
    check(ops, C.temporal_conv_case(b, cin, cout, f, d, taps, force=5))


@pytest.mark.parametrize("kw", C.CONV_CASES, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_conv3x3(ops, kw):
    check(ops, C.conv_case(**kw))


@pytest.mark.parametrize("force", [5, 3], ids=["pipelined-loop", "pingpong-loop"])
@pytest.mark.parametrize("kw", C.HALO_CASES, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_conv3x3_halo_patch(ops, kw, force):
    check(ops, C.conv_case(**kw, force=force))


@pytest.mark.parametrize("n,c,h,w", C.PARITY_CASES)
def test_upsample_conv3x3_parity(ops, n, c, h, w):
    from lavie_amd import _lib
    lib = _lib.load()
    assert lib.lavie_upsample_conv3x3_supported(n, h, w, c) == 1
    assert not any(lib.lavie_upsample_conv3x3_supported(n_, h_, w_, c_) for n_, c_, h_, w_ in C.PARITY_REFUSED)      # nothing smaller is taken
    check(ops, C.conv_case(n=n, c1=c, cout=c, h=h, w=w, ups=1, parity=True))


@pytest.mark.parametrize("n,c,h,w,splits", C.PARITY_SPLIT_CASES)
def test_upsample_conv3x3_parity_split(n, c, h, w, splits):
    """the parity form under the split-K factor its planner chooses (force_splits does not apply to it: one run, not six): fp32 slabs
    written from four parities, then the fixed-order reduce; y per element, the parity{py}{px}, border and seam regions on their own"""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import _lib, ops as o
    assert _lib.load().lavie_upsample_conv3x3_supported(n, h, w, c) == 1
    case = C.parity_case(n, c, h, w)
    assert {"parity00", "parity01", "parity10", "parity11", "border", "seams"} <= set(case.regions)
    with o.op_statistics(plan=(True, False)):            # the plan of this launch, from the library: nothing is launched
        case.run(o, {k: v.cuda() for k, v in case.inputs.items()}, {"y": torch.empty(case.outputs["y"][0], dtype=torch.float16, device="cuda")})
    assert o.op_statistics.last()["splits"] == splits
    check_local(case)


def deep_runs():
    """(case, variant, (tile, splits)) of opcases.deep_cases(): the forced cases under their own mode, the others under their variants"""
    return [pytest.param(c, v, fs, id=f"{c.name}-{v}") for c, v, fs in C.gemm_runs(C.deep_cases())]


@pytest.mark.parametrize("case,variant,fs", deep_runs())
def test_deep_reduction_case(case, variant, fs):
    """80 K-tiles under the automatic split-K factor and unsplit on each kernel; 3 + 2 slab segments with forced splits that begin inside
    a segment and at the shortcut segments (tests/test_gemm_reach_host.py asserts factor, grid and where each split begins)"""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import ops as o
    with C.forced(*fs, tuple(_forced)):
        oc.check_case(o, case, forced=fs, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("taps", [3, 5])
@pytest.mark.parametrize("b,cin,cout,f,d", C.TCONV_SHAPES)
def test_temporal_conv(ops, b, cin, cout, f, d, taps):
    check(ops, C.temporal_conv_case(b, cin, cout, f, d, taps))


@pytest.mark.parametrize("tap", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("n,cin,cout,h,w", C.EDGE_IN)
def test_conv_edge_in(ops, n, cin, cout, h, w, dtype, tap):
    check(ops, C.edge_in_case(n, cin, cout, h, w, dtype, tap))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("n,cin,cout,h,w", C.EDGE_OUT)
def test_conv_edge_out(ops, n, cin, cout, h, w, dtype):
    check(ops, C.edge_out_case(n, cin, cout, h, w, dtype))


@pytest.mark.parametrize("kw", C.GN_CASES, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_group_norm(ops, kw):
    check(ops, C.group_norm_case(**kw))


@pytest.mark.parametrize("M,C_,offset", C.LN_CASES)
def test_layer_norm(ops, M, C_, offset):
    check(ops, C.layer_norm_case(M, C_, offset))


@pytest.mark.parametrize("nb,l,c", C.SELF_ATTN)
def test_self_attention(ops, nb, l, c):
    check(ops, C.attention_case(nb, l, c))


@pytest.mark.parametrize("lk,div", C.CROSS_ATTN)
def test_cross_attention(ops, lk, div):
    check(ops, C.attention_case(3, 40, 320, lk=lk, kv_div=div))


@pytest.mark.parametrize("l,c", C.WIDE_ATTN)
def test_wide_head_attention(ops, l, c):
    check(ops, C.attention_case(1, l, c, heads=1))


@pytest.mark.parametrize("frames,d", C.SPARSE_CAUSAL)
def test_sparse_causal_attention(ops, frames, d):
    check(ops, C.sparse_causal_case(frames, d))


@pytest.mark.parametrize("tiled", [False, True], ids=["streaming", "tiled"])
@pytest.mark.parametrize("b,f,d,c", C.TATTN_SHAPES)
def test_temporal_attention(ops, b, f, d, c, tiled):
    check(ops, C.temporal_attention_case(b, f, d, c, tiled))


@pytest.mark.parametrize("tiled", [False, True], ids=["streaming", "tiled"])
def test_temporal_attention_plain(ops, tiled):
    check(ops, C.temporal_attention_case(1, 17, 5, 256, tiled, plain=True))


# the row-resident fused blocks: the smallest shapes their predicates take and one past a tile, out of place and with y aliasing
# x; a shape a predicate does not take (rows per video / frame that are no multiple of the 16-token tile) must be refused with the
# kernel's own message and nothing touched
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("M", [1, 129])
def test_geglu_mlp(ops, M, in_place):
    check(ops, C.geglu_mlp_case(M, in_place))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("B,D", [(1, 1), (2, 13)])
def test_temporal_block(ops, B, D, in_place):
    check(ops, C.temporal_block_case(B, D, in_place))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("B,P,L", C.CROSS_BLOCKS)
def test_cross_block(ops, B, P, L, in_place):
    check(ops, C.cross_block_case(B, P, L, in_place))


@pytest.mark.parametrize("B,P,L", C.CROSS_REFUSED)
def test_cross_block_refuses_ragged_videos(ops, B, P, L):
    check(ops, C.cross_block_case(B, P, L, False), refusal="rows_per_batch=1 is not built")


@pytest.mark.parametrize("D", [16, 48])
@pytest.mark.parametrize("NB", [1, 5])
def test_proj_qkv(ops, NB, D):
    check(ops, C.proj_qkv_case(NB, D))


@pytest.mark.parametrize("NB", [1, 5])
def test_proj_qkv_refuses_ragged_frames(ops, NB):
    check(ops, C.proj_qkv_case(NB, 1), refusal="1 rows per GroupNorm domain")


# ------------------------------------------------------------------ past one tile per workgroup
# None of these kernels depends on the GEMM choice: each case runs once, not under the six variants.
def check_local(case):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import ops as o
    oc.check_case(o, case, forced=tuple(_forced), sync=torch.cuda.synchronize)


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", C.multi_pass_cases() + C.multi_pass_cases(in_place=True), ids=_ids(C.multi_pass_cases() + C.multi_pass_cases(in_place=True)))
def test_row_resident_blocks_past_one_pass(case):
    """opcases.PATHS: second and later passes, idle waves, ragged and boundary-crossing passes under lavie_debug_rowfuse_grid, and the
    production grid at 2049 pixels; the cap is back at 0 afterwards."""
    check_local(case)
    from lavie_amd import _lib
    assert _lib.load().lavie_debug_rowfuse_grid(0) == 0


@pytest.mark.parametrize("in_place", [False, True])
def test_temporal_block_peaked(in_place):
    check_local(C.temporal_block_case(2, 13, in_place, profile="peaked"))


_TATTN_NEW = [c for c in C.temporal_attention_cases()
              if c.name not in {C.temporal_attention_case(*sh, t).name for sh in C.TATTN_SHAPES for t in (False, True)}
              and c.name not in {C.temporal_attention_case(1, 17, 5, 256, t, plain=True).name for t in (False, True)}]


@pytest.mark.parametrize("case", _TATTN_NEW, ids=_ids(_TATTN_NEW))
def test_temporal_attention_routes(case):
    """every instantiation launch_temporal_attention can launch (opcases.TATTN_ROUTES), at each head split, several tiles per workgroup"""
    check_local(case)


_GN_NEW = [C.group_norm_case(**k) for k in C.GN_PAST_SLAB]


@pytest.mark.parametrize("case", _GN_NEW, ids=_ids(_GN_NEW))
def test_group_norm_past_one_slab(case):
    check_local(case)


def test_rowfuse_grid_hook_contract():
    from lavie_amd import _lib
    lib = _lib.load()
    try:
        assert lib.lavie_debug_rowfuse_grid(3) == 0 and lib.lavie_debug_rowfuse_grid(256) == 0
        assert lib.lavie_debug_rowfuse_grid(257) != 0 and lib.lavie_debug_rowfuse_grid(-1) != 0
    finally:
        assert lib.lavie_debug_rowfuse_grid(0) == 0


@pytest.mark.parametrize("n", C.STEP_LENGTHS)
@pytest.mark.parametrize("kind", C.STEP_KINDS)
def test_sampler_steps(ops, kind, n):
    check(ops, C.step_case(kind, n))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("N,K,r", C.LORA_SHAPES)
def test_lora_merge(ops, N, K, r, in_place):
    check(ops, C.lora_case(N, K, r, in_place))


def test_worst_fractions_at_model_depth_are_reported(capsys):
    """runs last in this file: prints the worst observed |err| / bound of every case at model depth that ran (opcheck.WORST; nothing is
    asserted on it beyond what each check above already did)"""
    new = {c.name for c in C.deep_cases()} | {C.parity_case(*s[:4]).name for s in C.PARITY_SPLIT_CASES}
    new |= {C.conv_case(**C.SEG).name, C.conv_case(**C.SEG_SC).name, C.geglu_case(160, 1280).name}
    seen = {k: v for k, v in oc.WORST.items() if k.rsplit(":", 1)[0] in new}
    with capsys.disabled():
        for k, v in sorted(seen.items()):
            print(f"\nworst fraction of bound: {k}: {v:.3f}", end="")
    assert all(v <= 1.0 for v in seen.values())
