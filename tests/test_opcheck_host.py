"""The per-element operator check (tests/opcheck.py) before a GPU is involved: the torch fp32 model of every kernel — fp16 roundings
at the points counted in the kernel's source — meets the bound of its own case with zero offenders; injected defects are caught
and located where the whole-tensor rel-L2 criterion of the older operator tests passes them; the guard-band and poison logic
works on CPU tensors."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import opcases as C
import opcheck as oc
from gpu_util import TOL_OP, rel_l2

CASES = C.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fp32_model_meets_its_bound(case):
    """If this fails the rounding-point count n (or K_terms) of the case is wrong: fix the count, not the bound."""
    case.check(case.model(), label="model ")


# ------------------------------------------------------------------ the call descriptions of the GEMM-family cases
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lavie_hip.h")
REPLAYED = ("linear", "linear_lnfold", "linear_lnfold_geglu", "conv3x3", "conv3x3_down", "upsample_conv3x3", "temporal_conv",   # driver.cpp run_optrace
            "timestep_sinusoid", "gemv", "pack_conv_in", "conv_in", "pack_conv_out", "conv_out", "add_class_emb_silu", "fill_relpos_bias", "ln_fold",
            "pack_geglu_vec", "copy_rows", "f16_to_f32",
            "geglu_mlp", "temporal_block", "cross_block", "cross_block_long", "proj_qkv", "temporal_attention", "group_norm", "group_norm_affine",
            "conv_edge_in", "conv_edge_out", "attention", "sparse_causal_attention", "group_norm_stats", "rowstat_finalize")
OPTIONAL = ("bias", "bias2", "R", "x2", "sc1", "sc2", "bias_f16", "b", "tap_bias")
DESCRIPTORS = ("cs1", "cs2")          # lavie_gn_producer_stats operands: their integer fields are described as cs1_<field> / cs2_<field>
ALWAYS = {"conv_in": ("bias",), "conv_out": ("bias",), "temporal_attention": ("bias",)}          # operands of the new entries that are not optional there


def abi_parameters(entry):
    """[(name, is_int)] of lavie_<entry>_f16 as include/lavie_hip.h declares it"""
    with open(HEADER) as f:
        m = re.search(r"\bint lavie_%s(?:_f16|_f32)?\(([^)]*)\)" % entry, f.read())
    return [(p.split()[-1].lstrip("*"), p.split()[0] in ("int", "long")) for p in m.group(1).replace("\n", " ").split(",")]


class RecordingLib:
    """stands in for the loaded library: every entry point records its arguments and succeeds"""

    def __init__(self):
        self.recorded = []

    def __getattr__(self, name):
        if name.endswith(("_image_bytes", "_bias_floats", "_ws_floats")):          # size queries of the pack steps: any size will do
            return lambda *args: 64
        return lambda *args: self.recorded.append((name, args)) or 0


GEMM_CASES = C.gemm_family_cases()


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c.name for c in GEMM_CASES])
def test_call_description_is_what_run_passes(case, monkeypatch):
    """`case.calls` — what tests/test_gemm_reach_host.py replays on the host-only build — against what `case.run` really hands to
    the C ABI through lavie_amd/ops.py: the case runs on its CPU tensors with a recording library behind the wrappers (their
    device checks off, everything that derives an integer left as it is), and every integer and every optional operand of each
    replayed entry point must be the one the description names, in order."""
    from lavie_amd import _lib, ops
    lib = RecordingLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "check", lambda rc, *a: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_chk16", lambda *ts: None)
    monkeypatch.setattr(ops, "_chk32", lambda *ts: None)
    monkeypatch.setattr(ops, "_chk_cols16", lambda *ts: None)
    monkeypatch.setattr(ops, "_edge_dtype", lambda t, what: int(t.dtype == torch.float32))
    monkeypatch.setattr(ops, "_zero_pages", {})

    def out_as_given(out, shape, dtype, device, what):
        assert out is not None and tuple(out.shape) == tuple(shape) and out.dtype == dtype, what
        return out
    monkeypatch.setattr(ops, "_out", out_as_given)
    outs = {k: torch.empty(shape, dtype=dt) for k, (shape, dt) in case.outputs.items()}
    kind = getattr(case, "kind", "")                   # a statistics case: the sink's buffers are further outputs (sized by the plan on a GPU)
    if "cs" in kind:
        outs["cs"] = torch.empty(8)
    if "rs" in kind:
        outs["rs"] = torch.empty(1, 1, 2)
    case.run(ops, case.inputs, outs)
    armed = [args for name, args in lib.recorded if name == "lavie_debug_op_statistics"]
    assert {k: v for k, v in case.knobs.items() if k.startswith("stats_")} == ({} if not kind else {k: 1 for k, on in (("stats_cs", "cs" in kind), ("stats_rs", "rs" in kind)) if on})
    if kind:                                           # armed with exactly the kinds the knobs name, around the launch, then disarmed
        assert [(a[0] is not None and a[1] > 0, a[2] is not None and a[3] > 0) for a in armed] == [("cs" in kind, "rs" in kind), (False, False)]
        order = [name for name, _ in lib.recorded if name == "lavie_debug_op_statistics" or re.sub(r"^lavie_|_f16$", "", name) in REPLAYED]
        assert order[0] == order[-1] == "lavie_debug_op_statistics" and len(order) == 3, order
    else:
        assert armed == []
    passed = []
    for name, args in lib.recorded:
        entry = re.sub(r"^lavie_|_f16$|_f32$", "", name) if name != "lavie_f16_to_f32" else "f16_to_f32"
        if entry not in REPLAYED:
            continue                                   # the pack steps: no launch of the GEMM family
        params = abi_parameters(entry)
        assert len(params) == len(args), (name, len(params), len(args))
        ints = {p: int(a) for (p, is_int), a in zip(params, args) if is_int}
        ints.update({p: int(a is not None) for (p, _), a in zip(params, args) if p in OPTIONAL and p not in ALWAYS.get(entry, ())})
        for (p, _), a in zip(params, args):
            if p in DESCRIPTORS and a is not None:     # ctypes.byref(descriptor)
                d = a._obj
                assert d.struct_size == __import__("ctypes").sizeof(d) and d.partials and d.partials_floats > 0
                ints.update({f"{p}_{f}": int(getattr(d, f)) for f in ("C", "rows", "nsets", "set_blocks", "span")})
        passed.append((entry, ints))
    assert len(passed) == len(case.calls) >= 1, (passed, case.calls)
    for (entry, ints), (want_entry, want) in zip(passed, case.calls):
        assert entry == want_entry
        assert set(want) <= set(ints), sorted(set(want) - set(ints))
        assert ints == {**{p: 0 for p in ints if p in OPTIONAL}, **want}, (entry, ints, want)


# ------------------------------------------------------------------ injected defects
def fails_at(case, got, where_text):
    with pytest.raises(AssertionError) as e:
        case.check({"y": got})
    assert where_text in str(e.value), str(e.value)
    assert rel_l2(got, case.ref["y"][0]) < TOL_OP, "the whole-tensor criterion was expected to pass this defect"


def ulps16(v, n):
    """v moved by n fp16 units in the last place, away from zero"""
    bits = v.reshape(1).clone().view(torch.int16)
    return (bits + n).view(torch.float16)[0]


def worst_ref(case):
    return int(case.ref["y"][0].abs().reshape(-1).argmax())


@pytest.fixture(scope="module")
def gemm():
    case = C.linear_case(120001, 64, 128, "bias_residual")      # tall enough for the old criterion to miss one row
    return case, case.model()["y"]


def test_gemm_one_element_off_by_4_ulps(gemm):
    case, y = gemm
    i = worst_ref(case)
    bad = y.clone()
    bad.view(-1)[i] = ulps16(bad.view(-1)[i], 4)
    fails_at(case, bad, "1 of %d elements" % y.numel())
    fails_at(case, bad, "(row %d, column %d)" % divmod(i, 64))


def test_gemm_last_row_without_bias(gemm):
    case, y = gemm
    i = case.inputs
    bad = y.clone()
    bad[-1] = (i["a"][-1].float() @ i["w"].float().t() + i["r"][-1].float()).half()
    fails_at(case, bad, "(row 120000, column")


def test_gemm_dropped_k_tile(gemm):
    """the second 64-wide K-tile missing from the four columns one lane holds, in one row"""
    case, y = gemm
    i = case.inputs
    row, cols = 77777, slice(20, 24)
    bad = y.clone()
    bad[row, cols] = (i["a"][row, :64].float() @ i["w"][cols, :64].float().t() + i["bias"][cols] + i["r"][row, cols].float()).half()
    fails_at(case, bad, "(row 77777, column 2")


@pytest.fixture(scope="module")
def conv():
    case = C.conv_case(n=1, c1=64, cout=64, h=200, w=200)
    return case, case.model()["y"]


def test_conv_one_element_off_by_4_ulps(conv):
    case, y = conv
    i = worst_ref(case)
    bad = y.clone()
    bad.view(-1)[i] = ulps16(bad.view(-1)[i], 4)
    p, ch = divmod(i, 64)
    fails_at(case, bad, "(frame 0, y %d, x %d, channel %d)" % (p // 200, p % 200, ch))


def test_conv_corner_tap_from_wrong_neighbour(conv):
    """at pixel (0, 0) the tap (dy 0, dx +1) reads pixel (1, 1) instead of (0, 1)"""
    case, y = conv
    x, wt = case.inputs["x1"].float(), case.inputs["wt"].float()
    tap = wt[:, :, 1, 2]
    bad = y.clone()
    bad[0] = (y[0].float() - tap @ x[1] + tap @ x[200 + 1]).half()
    fails_at(case, bad, "(frame 0, y 0, x 0, channel")
    with pytest.raises(AssertionError, match=":border"):           # and the border region on its own names it too
        oc.assert_elementwise(bad, *case.ref["y"], case.c, where=case.where, label="x:border", mask=case.regions["border"])


def test_attention_one_element_off_by_4_ulps():
    case = C.attention_case(1, 1, 256)
    y = case.model()["y"]
    i = worst_ref(case)
    bad = y.clone()
    bad.view(-1)[i] = ulps16(bad.view(-1)[i], 4)
    fails_at(case, bad, "(token 0, head %d, dim %d)" % divmod(i, 32))


def test_attention_one_dropped_key():
    """query 5 of head 3 never sees the last key (a mask wrong for one key of the ragged last tile); host-only shape, long
    enough for the whole-tensor criterion to miss it"""
    case = C.attention_case(2, 300, 1280)
    bad = case.model()["y"].clone()
    dh = 160
    qkv = case.inputs["qkvw"].float()
    q, k, v = qkv[:, :1280], qkv[:, 1288:2568], qkv[:, 2576:]
    hs = slice(3 * dh, 4 * dh)
    s = (q[5, hs] * dh ** -0.5) @ k[:, hs].t()
    s = s[:300]
    s[299] = -float("inf")
    bad[5, hs] = (torch.softmax(s, 0) @ v[:300, hs]).half()
    fails_at(case, bad, "(token 5, head 3, dim")


def test_attention_cases_reach_every_instantiation():
    """the shape tables of opcases.py against the dispatch of attention.hip, as attention_route reads it"""
    reached = {c.route for c in CASES if hasattr(c, "route")}
    assert reached == set(C.ATT_ROUTES), (sorted(set(C.ATT_ROUTES) - reached), sorted(reached - set(C.ATT_ROUTES)))
    for profile in C.PROFILES:          # and each V2 instantiation under each profile it has room for (creep: three key tiles)
        got = {c.route for c in CASES if hasattr(c, "route") and c.name.endswith(profile + "]")}
        need = {r for r in C.ATT_ROUTES if "V2" in r and not (profile in ("creep", "mixed_wave") and "QT1" in r and "sc" in r)}
        # (sparse-causal QT 1 is d = 65: two key tiles a half, and token d - 2 lies in the first of them)
        assert need <= got, (profile, sorted(need - got))


@pytest.mark.skipif(__import__("shutil").which("hipcc") is None, reason="hipcc not on PATH")
def test_attention_cases_launch_the_kernel_their_route_names():
    """opcases.attention_route against the library itself: every attention case's call is replayed on the host-only build (`hostcheck
    optrace`), and the one kernel launch_attention launched under the stub is the instantiation the route names (route_kernel)."""
    cases = [c for c in CASES if hasattr(c, "route")]
    assert {c.route for c in cases} == set(C.ATT_ROUTES) and all(c.calls and len(c.calls) == 1 for c in cases)
    reach = C.gemm_reach(cases)
    for c in cases:
        launches = reach[(c.name, "auto")]
        assert launches is not None and len(launches) == 1, (c.name, launches)
        assert C.launch_name(launches[0]) == C.route_kernel(c.route, c.calls[0][1]["dh"]), (c.name, c.route, launches[0])
    assert len({C.launch_name(reach[(c.name, "auto")][0]) for c in cases}) == len(C.ATT_ROUTES) + 1      # "wide" is two kernels


@pytest.fixture(scope="module")
def far_below():
    case = C.attention_case(1, 193, 320, profile="far_below")
    assert case.route == "dma<5,QT2,V2,4 waves>" and case.hard["far"] == [0, 21, 101, 192]
    return case, case.model()["y"]


def test_attention_far_below_rows_nan(far_below):
    """what 0 * exp2(+huge) in the first key tile leaves in O and l: the hard rows NaN, everything else right"""
    case, y = far_below
    bad = y.clone()
    bad[case.hard["far"]] = float("nan")
    with pytest.raises(AssertionError) as e:
        case.check({"y": bad})
    assert "%d of %d elements" % (4 * 320, y.numel()) in str(e.value), str(e.value)
    assert any("(token %d, head" % r in str(e.value) for r in case.hard["far"]), str(e.value)


@pytest.mark.parametrize("n_rows", [4, 1])
def test_attention_far_below_rows_never_rescaled(far_below, n_rows):
    """The hard rows are the softmax over the first key tile alone (a kernel that never moved its running maximum): the check
    fails at a hard row and names it.  This defect is NOT one the whole-tensor criterion passes, with four hard rows or with one:
    a hard row's right output is the matching key's V row (|v| ~ 1 per element) and the other 189 rows are averages over ~190
    keys (~0.1 per element), so the hard rows carry most of the tensor's norm: rel_l2 = 0.81 with four rows, 0.40 with one,
    against TOL_OP = 2e-3.  rel-L2 never saw the first-tile defect because no input of the suite had such rows; it is asserted
    here as what it is, far above TOL_OP."""
    case, y = far_below
    rows = case.hard["far"][:n_rows]
    qkv = case.inputs["qkvw"].float()
    q, k, v = qkv[:, :320], qkv[:, 328:648], qkv[:, 656:]
    bad = y.clone()
    for r in rows:
        for h in range(8):
            hs = slice(40 * h, 40 * h + 40)
            bad[r, hs] = (torch.softmax((q[r, hs] * 40 ** -0.5) @ k[:64, hs].t(), 0) @ v[:64, hs]).half()
    with pytest.raises(AssertionError) as e:
        case.check({"y": bad})
    assert any("(token %d, head" % r in str(e.value) for r in rows), str(e.value)
    bad_tokens = (~((bad.double() - case.ref["y"][0]).abs() <= oc.U16 * case.ref["y"][0].abs() + case.c * case.ref["y"][1])).any(1).nonzero().flatten().tolist()
    assert bad_tokens == rows, bad_tokens                       # the hard rows and nothing else
    assert rel_l2(bad, case.ref["y"][0]) > 100 * TOL_OP


# ------------------------------------------------------------------ split-K and multi-slab segments at model depth
def nchw(rows_, n, h, w):
    return rows_.reshape(n, h, w, -1).permute(0, 3, 1, 2).to(torch.float64)


def ktile_term(x, wt, c_off, a_slab, a_tap, w_slab, w_tap):
    """One K-tile of a 3x3 conv as rows [n h w, cout], float64: the 64 channels of slab `a_slab` of source x [n, c, h, w] read at tap
    `a_tap` (ky * 3 + kx, zeros outside the image), times the weights wt[:, c_off + 64 w_slab ..., w_tap]."""
    n, _, h, w = x.shape
    dy, dx = a_tap // 3 - 1, a_tap % 3 - 1
    xs = F.pad(x[:, 64 * a_slab:64 * a_slab + 64], (1, 1, 1, 1))[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    wk = wt[:, c_off + 64 * w_slab:c_off + 64 * w_slab + 64, w_tap // 3, w_tap % 3].to(torch.float64)
    return torch.einsum("nchw,oc->nhwo", xs, wk).reshape(n * h * w, -1)


def rejected(case, bad64):
    with pytest.raises(AssertionError, match="outside the bound"):
        case.check({"y": bad64.half()})
    return offenders(case, bad64.half())


def test_split_k_range_without_its_first_k_tile():
    """conv 192 + 128 with both shortcuts under 3 splits: the second range begins at K-tile 16 = (segment 0, slab 1, tap 7).  A cursor that
    starts one tile late (or a prologue that never issues tile t_begin) leaves that tile's products out: every output with that
    neighbour inside the image is off."""
    case = C.conv_case(**C.SEG_SC, force=1, splits=3)
    ints = case.calls[0][1]
    segs = C.kloop_segments(ints)
    assert C.kloop_position(segs, C.split_begins(50, 3)[1]) == (0, 1, 7)
    x1 = nchw(case.inputs["x1"], 1, 5, 7)
    ref = case.ref["y"][0]
    case.check({"y": ref.half()})
    off = rejected(case, ref - ktile_term(x1, case.inputs["wt"], 0, 1, 7, 1, 7))
    pix = off.reshape(5, 7, -1)
    assert pix[:4].any(-1).all() and pix[:4].float().mean() > 0.5 and not pix[4].any()      # tap 7 = (dy +1, dx 0): the bottom row has no such neighbour


def transposed_segment_1(case, n, h, w, c1, c2):
    """The reference with segment 1 (the second 9-tap source) gathered tap-major, slab-minor against weights packed slab-major,
    tap-minor: K-tile j of the segment reads (tap j // nslab, slab j % nslab) where the weights hold (slab j // 9, tap j % 9)."""
    x2, wt, nslab = nchw(case.inputs["x2"], n, h, w), case.inputs["wt"], c2 // 64
    bad = case.ref["y"][0].clone()
    for j in range(9 * nslab):
        bad -= ktile_term(x2, wt, c1, j // 9, j % 9, j // 9, j % 9)
        bad += ktile_term(x2, wt, c1, j % nslab, j // nslab, j // 9, j % 9)
    return bad


def test_slab_and_tap_order_transposed_within_the_second_segment():
    """Caught at the 192 + 128 cases, split or not; NOT caught by the 64 + 64 case the suite had, whose segments are one slab each:
    there the transposed order is the same order, and the defective reference is the reference."""
    for case in (C.conv_case(**C.SEG_SC, force=1, splits=1), C.conv_case(**C.SEG)):
        off = rejected(case, transposed_segment_1(case, 1, 5, 7, 192, 128))
        assert off.float().mean() > 0.9
    old = C.conv_case(n=2, c1=64, c2=64, cout=64, h=3, w=5, csc=64)
    assert old in [C.conv_case(**k) for k in C.CONV_CASES]
    same = transposed_segment_1(old, 2, 3, 5, 64, 64)
    assert float((same - old.ref["y"][0]).abs().max()) <= 1e-12 * float(old.ref["y"][0].abs().max())
    old.check({"y": same.half()})                           # passes: the old case cannot tell the two orders apart


@pytest.fixture(scope="module")
def parity4():
    n, c, h, w, splits = C.PARITY_SPLIT_CASES[0]
    assert splits == 4
    return C.parity_case(n, c, h, w), (n, c, h, w)


def test_reduce_that_leaves_out_one_of_four_slabs(parity4):
    """The 4-split parity case: slab 3 holds the products of slabs 15..19 of the source = channels 960..1279.  A reduce that sums three
    slabs (a slab stride or a loop bound off by one) leaves them out of every output element."""
    case, (n, c, h, w) = parity4
    x = nchw(case.inputs["x1"], n, h, w).float()
    up = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    lo = c - c // 4
    part = C.rows(F.conv2d(up[:, lo:], case.inputs["wt"][:, lo:].float(), padding=1)).to(torch.float64)
    ref = case.ref["y"][0]
    case.check({"y": ref.half()})
    off = rejected(case, ref - part)
    assert off.float().mean() > 0.9
    for r in ("parity00", "parity01", "parity10", "parity11"):       # and each parity region names it on its own
        with pytest.raises(AssertionError, match=":" + r):
            oc.assert_elementwise((ref - part).half(), *case.ref["y"], case.c, where=case.where, label="x:" + r, mask=case.regions[r])


def test_parity_split_statistics_as_four_sets_instead_of_one(parity4):
    """Behind a split parity launch the reduce writes 32-row blocks of output rows in one set.  The unsplit parity kernel's layout
    — four sets, one per output parity — fills a buffer of the same size with other sums: rejected by check_colstat."""
    import statcheck as S
    case, (n, c, h, w) = parity4
    y = case.ref["y"][0].half()
    M = y.shape[0]
    plan = {"rows": 32, "span": 32, "sets": 1, "set_blocks": M // 32, "contiguous": 1, "blocks_stored": M // 32, "cs_floats": M // 32 * 2 * c}
    S.check_colstat(y, S.model_colstat(y, plan), plan)
    four = dict(plan, sets=4, set_blocks=M // 4 // 32)
    bad = S.model_colstat(y, four, parity=(2 * h, 2 * w))
    assert bad.numel() == plan["cs_floats"]
    with pytest.raises(AssertionError, match="span sums"):
        S.check_colstat(y, bad, plan)


# ------------------------------------------------------------------ the persistent kernel past its first tile
def ppx_tile_lists(tiles, nwg=256):
    """The tile ids each workgroup of the persistent GEMM walks, in order: a mirror of igemm_ppx.hip:162-182 (and its header,
    :32-34) for tiles > nwg.  Tile id = m_tile * n_tiles + n_tile; the ids are cut into 8 contiguous chunks, one per XCD label
    (blockIdx % 8), and workgroup j = blockIdx / 8 of a chunk takes its tiles j, j + nwg / 8, j + 2 nwg / 8, ..."""
    assert tiles > nwg and nwg % 8 == 0
    per, qq, r = nwg // 8, tiles // 8, tiles % 8
    lists = []
    for b in range(nwg):
        xcd, j = b % 8, b // 8
        start = xcd * (qq + 1) if xcd < r else r * (qq + 1) + (xcd - r) * qq
        size = qq + (1 if xcd < r else 0)
        lists.append([start + k for k in range(j, size, per)])
    assert sorted(t for l in lists for t in l) == list(range(tiles))
    return lists


def offending_tiles(case, got, bn):
    ref, scale = case.ref["y"]
    bad = ~((got.double() - ref).abs() <= oc.U16 * ref.abs() + case.c * scale)
    n_tiles = ref.shape[1] // bn
    per_tile = bad.reshape(ref.shape[0] // 160, 160, n_tiles, bn).permute(0, 2, 1, 3).reshape(-1, 160 * bn)
    return {int(t): int(c) for t, c in enumerate(per_tile.sum(1)) if c}


def test_ppx_second_tile_with_the_other_aux_parity():
    """Every workgroup's second tile finished with the bias / ln_s / (mean, rstd) rows of the other aux buffer, which still holds
    its first tile's: the check fails at those tiles and nowhere else.  lnfold 13760x960x320: 86 x 3 = 258 tiles, so the first
    workgroup of XCD 0 and of XCD 1 run two tiles each (33 tiles in their chunks) and every other workgroup one.  With three
    column tiles the second tile (id + 32) is in another row tile and another column tile than the first, so all three pieces
    of the defect — bias, ln_s and the (mean, rstd) rows — are wrong values, each of which alone must be caught."""
    case = C.lnfold_case(13760, 960, 320)
    i, bn, n_tiles = case.inputs, 320, 3
    lists = ppx_tile_lists(258)
    second = {l[1]: l[0] for l in lists if len(l) > 1}
    assert second == {32: 0, 65: 33}
    assert all(t // n_tiles != p // n_tiles and t % n_tiles != p % n_tiles for t, p in second.items())
    y = case.model()["y"]
    for stale in (("bias", "s", "stats"), ("bias",), ("s",), ("stats",)):
        bad = y.clone()
        for t, prev in second.items():
            (m0, n0), (pm0, pn0) = ((x // n_tiles * 160, x % n_tiles * bn) for x in (t, prev))
            acc = i["a"][m0:m0 + 160].float() @ i["wf"][n0:n0 + bn].float().t()
            st = i["stats"][pm0:pm0 + 160] if "stats" in stale else i["stats"][m0:m0 + 160]
            s = i["s"][pn0:pn0 + bn] if "s" in stale else i["s"][n0:n0 + bn]
            bias = i["bias"][pn0:pn0 + bn] if "bias" in stale else i["bias"][n0:n0 + bn]
            bad[m0:m0 + 160, n0:n0 + bn] = (st[:, 1:] * (acc - st[:, :1] * s) + bias).half()
        with pytest.raises(AssertionError):
            case.check({"y": bad})
        off = offending_tiles(case, bad, bn)
        assert set(off) == set(second), (stale, off)
        assert len(stale) < 3 or all(c > 0.9 * 160 * bn for c in off.values()), off


def test_ppx_steady_state_tile_with_the_previous_tiles_residual():
    """The residual rows of a steady-state tile (neither the first nor the last of its workgroup) are those prefetched for the
    workgroup's previous tile.  linear 20640x1280x320: 516 tiles, the first workgroup of XCDs 0 - 3 runs three.  Caught at exactly
    those tiles.  The whole-tensor criterion does NOT pass this defect, not even on one tile: a tile of N(0, 1) residual rows
    exchanged for another is an error of norm sqrt(2 * 160 * 320) = 320 beside an output of norm sqrt(3 * 20640 * 1280) = 8.9e3:
    rel_l2 = 3.6e-2 measured on one tile, against TOL_OP = 2e-3 — asserted as what it is."""
    case = C.linear_case(20640, 1280, 320, "bias_residual")
    i, bn, n_tiles = case.inputs, 320, 4
    lists = ppx_tile_lists(516)
    steady = {l[k]: l[k - 1] for l in lists for k in range(1, len(l) - 1)}
    assert steady == {32: 0, 97: 65, 162: 130, 227: 195}
    y = case.model()["y"]
    ref = case.ref["y"][0]
    for n_defects in (4, 1):
        bad = y.clone()
        for t, prev in list(steady.items())[:n_defects]:
            (m0, n0), (pm0, pn0) = ((x // n_tiles * 160, x % n_tiles * bn) for x in (t, prev))
            acc = i["a"][m0:m0 + 160].float() @ i["w"][n0:n0 + bn].float().t() + i["bias"][n0:n0 + bn]
            bad[m0:m0 + 160, n0:n0 + bn] = (acc + i["r"][pm0:pm0 + 160, pn0:pn0 + bn].float()).half()
        with pytest.raises(AssertionError):
            case.check({"y": bad})
        off = offending_tiles(case, bad, bn)
        assert set(off) == set(list(steady)[:n_defects]) and all(c > 0.9 * 160 * bn for c in off.values()), off
    assert 3e-2 < rel_l2(bad, ref) < 4e-2 and rel_l2(bad, ref) > 10 * TOL_OP


# ------------------------------------------------------------------ injected defects of the end and glue kernels
def offenders(case, got, k="y"):
    """bool tensor, shaped like the output: the elements outside the case's bound"""
    ref, scale = case.ref[k]
    c = case.c[k] if isinstance(case.c, dict) else case.c
    u = case.u[k] if isinstance(case.u, dict) else case.u
    return ~((got.double() - ref).abs() <= u * ref.abs() + c * scale)


def test_conv_out_without_the_sixth_register_slot():
    """Cin = 320 computed as conv_out4<5> would: slots 320..359 = the whole tap (+1, +1) dropped.  Caught at every pixel that has
    that neighbour and nowhere else.  Not a defect the whole-tensor criterion passes: a ninth of the terms is missing."""
    case = C.conv_out_case(320, 4, (2, 3, 3, 5))
    bad = case.model(drop_from=320)["y"]
    with pytest.raises(AssertionError, match="conv_out"):
        case.check({"y": bad})
    off = offenders(case, bad).any(1)                                  # [B, F, H, W]: pixels with an offending channel
    want = torch.zeros(2, 3, 3, 5, dtype=torch.bool)
    want[:, :, :-1, :-1] = True
    assert torch.equal(off, want)
    assert rel_l2(bad, case.ref["y"][0]) > 10 * TOL_OP
    assert not offenders(case, case.model(drop_from=360)["y"]).any()    # (nothing past slot 359: the same as the model)


def test_gemv_clamped_row_stored_past_the_end():
    """rows 28..31 of the last wave are clamped to row N - 1 = 30; stored unguarded, the clamped row lands at column N: for the
    last batch entry one element past the tensor.  The values are all right (rel-L2 = 0): only the guard band sees it."""
    case = C.gemv_case(2, 31, 320, False, False, True)
    y = case.model()["y"]

    def fn(i, o):
        o["y"].copy_(y)
        torch.as_strided(o["y"], (2 * 31 + 1,), (1,))[2 * 31] = y[1, 30]
    with pytest.raises(AssertionError, match=r"y .*guard band damaged in 1 elements, first at offset 62 .*row 2, column 0"):
        oc.run_guarded(fn, case.inputs, case.outputs, device="cpu")
    assert rel_l2(y, case.ref["y"][0]) < TOL_OP


def test_gemv_batch_row_reads_another_rows_vector():
    case = C.gemv_case(3, 64, 520, True, False, True)
    bad = case.model(row_from={1: 0})["y"]
    with pytest.raises(AssertionError, match=r"\(row 1, column"):
        case.check({"y": bad})
    off = offenders(case, bad)
    assert not off[0].any() and not off[2].any() and off[1].sum() >= 60         # row 1 and nothing else
    assert rel_l2(bad, case.ref["y"][0]) > 100 * TOL_OP                          # a whole row of three is wrong: not a defect rel-L2 passes


def test_sinusoid_halves_swapped_and_frequency_off_by_one():
    case = C.sinusoid_case(8, 320)
    t = case.inputs["t"]
    assert t[0] == 0
    swapped = case.model(swap=True)["y"]
    off = offenders(case, swapped)
    assert off[0].all()                                                          # t = 0: cos = 1 and sin = 0 everywhere
    assert off[:, :160].any(1).all() and off[:, 160:].any(1).all() and off.float().mean() > 0.9
    assert rel_l2(swapped, case.ref["y"][0]) > 100 * TOL_OP
    shifted = case.model(shift=1)["y"]
    off = offenders(case, shifted)
    assert not off[0].any()                                                      # t = 0: the angle is 0 whatever the frequency
    assert off[1:].any(1).all()                                                  # every other timestep, 0.001 included
    big = (t >= 1)
    assert off[big].float().mean() > 0.9
    assert rel_l2(shifted, case.ref["y"][0]) > 10 * TOL_OP
    with pytest.raises(AssertionError, match="timestep_sinusoid"):
        case.check({"y": shifted})


def test_ln_fold_row_sums_taken_before_the_fp16_rounding():
    """s summed from fp32 W gamma instead of the stored fp16 weight: outside the depth-aware bound on nearly every row, inside the
    GEMM family's (K + 8) 2^-23 on nearly every row, and far inside rel-L2."""
    case = C.ln_fold_case(130, 320, True)
    bad = case.model(unrounded_s=True)
    with pytest.raises(AssertionError, match=r"ln_fold\[130x320,bias1\]:s"):
        case.check(bad)
    assert offenders(case, bad["s"], "s").float().mean() > 0.8
    assert not offenders(case, bad["b"], "b").any() and torch.equal(bad["wout"], case.exact["wout"])
    ref, scale = case.ref["s"]
    loose = ~((bad["s"].double() - ref).abs() <= oc.U32 * ref.abs() + oc.gemm_c(320) * scale)
    assert loose.float().mean() < 0.05                                           # the GEMM family's constant passes nearly every row
    assert rel_l2(bad["s"], ref) < TOL_OP
    # the exact product rounded once to fp16 (numpy converts float64 directly) is not the stored weight: what a fused multiply-convert
    # gives, and what Wout's bit-for-bit comparison tells from fp16(fp32(W gamma)), over the (N, K) of all ln_fold cases
    diff = total = 0
    for n, k in C.LN_FOLD:
        cs = C.ln_fold_case(n, k, True)
        once = torch.from_numpy((cs.inputs["w"].double() * cs.inputs["gamma"].double()).numpy().astype("float16"))
        diff, total = diff + int((once != cs.exact["wout"]).sum()), total + once.numel()
    assert 0 < diff < 0.001 * total, (diff, total)


def test_copy_rows_column_offset_off_by_one():
    case = C.copy_rows_case(5, 7, 9, 31, 11)
    src = case.inputs["src"]

    def fn(i, o):
        o["y"][:, 12:19] = i["src"][:, :7]
    with pytest.raises(AssertionError, match=r"y: 5 elements outside the written region were stored to, first at offset 18 .*row 0, column 18"):
        oc.run_guarded(fn, case.inputs, case.outputs, device="cpu", partial=case.partial)

    def short(i, o):                                                             # one column too few
        o["y"][:, 11:17] = i["src"][:, :6]
    with pytest.raises(AssertionError, match=r"y: 5 elements never written, first at offset 17 .*row 0, column 17"):
        oc.run_guarded(short, case.inputs, case.outputs, device="cpu", partial=case.partial)
    got = oc.run_guarded(lambda i, o: o["y"][:, 11:18].copy_(i["src"][:, :7]), case.inputs, case.outputs, device="cpu", partial=case.partial)
    case.check(got)
    assert torch.equal(got["y"][:, 11:18], src[:, :7])


def test_conv_in_channels_of_one_pair_swapped():
    """K pair 1 = tap (-1, -1), channels 2 and 3, exchanged on the activation side: wrong at the pixels that have that neighbour"""
    case = C.conv_in_case(4, 8, (2, 3, 3, 5))
    bad = case.model(swap_pair=1)["y"]
    with pytest.raises(AssertionError, match="conv_in"):
        case.check({"y": bad})
    off = offenders(case, bad).reshape(6, 3, 5, 8).any(-1)
    want = torch.zeros(6, 3, 5, dtype=torch.bool)
    want[:, 1:, 1:] = True
    assert torch.equal(off, want)
    assert rel_l2(bad, case.ref["y"][0]) > 10 * TOL_OP


def test_every_listed_case_of_the_end_families_is_present():
    """the shape lists of the issue, as counts: dropping a case changes one of them"""
    fam = C.ends_cases()
    assert {k: len(v) for k, v in fam.items()} == {"conv_out": 7 * 4, "conv_in": 9 * 4, "pack": 9 + 3 + 3 + 4 + 8, "ln_fold": 10, "gemv": 5 * 8 + 1,
                                                  "timestep_sinusoid": 3, "add_class_emb_silu": 3, "fill_relpos_bias": 6}
    assert len({c.name for cs in fam.values() for c in cs}) == sum(len(v) for v in fam.values())
    assert {c.name for cs in fam.values() for c in cs} <= {c.name for c in CASES}


# ------------------------------------------------------------------ past one tile per workgroup: paths, routes, slabs
def test_multi_pass_cases_contain_every_path():
    """The share-rule mirror (opcases.rowfuse_walk) on every capped and natural-grid block case: the case set as a whole contains
    every path of opcases.PATHS, per block, and the candidates that do not are known not to."""
    got = {}
    for case in C.multi_pass_cases() + C.multi_pass_cases(in_place=True):
        fam, walk, paths = C.case_walk(case)
        got.setdefault(fam, set()).update(paths)
        assert sorted(t for t, _ in enumerate(walk)) == list(range(len(walk)))
    assert set(got) == set(C.PATHS)
    for fam, need in C.PATHS.items():
        assert need <= got[fam], (fam, sorted(need - got[fam]))
    # the share rule itself, on the figures of the kernels' comments: 81920 rows on 256 workgroups = 20 tiles each = passes 8 + 8 + 4
    walk = C.rowfuse_walk(81920 // 16, 256)
    assert [sum(1 for w, p, _ in walk if (w, p) == (0, k)) for k in range(3)] == [8, 8, 4] and max(p for _, p, _ in walk) == 2
    walk = C.rowfuse_walk(50, 3)
    assert [sum(1 for w, _, _ in walk if w == b) for b in range(3)] == [17, 17, 16] and walk[49] == (2, 1, 7) and walk[16] == (0, 2, 0)
    # B = 2, D = 25 cuts its passes at the video boundary and B = 4, P = 208 has equal pass counts: why neither is the case used
    assert "pass_spans_batches" not in C.walk_paths(C.rowfuse_walk(50, 3), batch_of=lambda t: t // 25)
    assert "pass_counts_differ" not in C.walk_paths(C.rowfuse_walk(52, 3, 13), batch_of=lambda t: t // 13)
    # cross_block: workgroup 0's second pass is cut at the end of video 0 and its third streams video 1's image
    walk = C.rowfuse_walk(56, 3, 14)
    assert [walk[t] for t in (7, 8, 13, 14, 18, 19, 27, 28)] == [(0, 0, 7), (0, 1, 0), (0, 1, 5), (0, 2, 0), (0, 2, 4), (1, 0, 0), (1, 1, 0), (1, 2, 0)]
    # the natural-grid case: 2049 pixels on 256 workgroups, workgroup 0 alone has a second pass
    fam, walk, _ = C.case_walk(C.temporal_block_case(3, 683, False))
    assert fam == "temporal_block" and len(walk) == 2049 and walk[8] == (0, 1, 0) and walk[9] == (1, 0, 0)
    assert C.temporal_block_case(3, 683, False).name.startswith(C.NATURAL_GRID)


def test_temporal_cases_reach_every_route_and_walk_several_tiles():
    """temporal_route on every temporal attention case: the reached set is TATTN_ROUTES; every streaming instantiation runs at
    each head split of the models' widths, with a masked tail and without, and in at least one case with a workgroup of three
    tiles beside one of two; the tile kernel runs forced and unforced, with a ragged pixel tile and with a halved head group."""
    cases = C.temporal_attention_cases()
    assert len({c.name for c in cases}) == len(cases) and {c.name for c in cases} <= {c.name for c in CASES}
    routes = {}
    for c in cases:
        routes.setdefault(c.troute["kernel"], []).append(c)
    assert set(routes) == set(C.TATTN_ROUTES), sorted(set(routes) ^ set(C.TATTN_ROUTES))
    dims = lambda c: dict(c.calls[0][1])
    for name, cs in routes.items():
        if name.startswith("temporal_stream_kernel"):
            group = int(name.split(",")[1])
            splits = {c.troute["heads_per_group"] for c in cs if dims(c)["heads"] == 8}
            assert splits >= ({8, 4, 2} if group >= 256 else {4, 2, 1}), (name, splits)
            multi = [c for c in cs if c.troute["fullest"] >= 3 and c.troute["emptiest"] < c.troute["fullest"]]
            assert len(multi) == C.TATTN_MULTI[name] >= 1, (name, [c.name for c in multi])
            assert any(dims(c)["B"] >= 2 and c.troute["tiles"] // dims(c)["B"] < c.troute["per_group"] * 2 for c in multi)     # the walk crosses a video
            frames = {dims(c)["F"] for c in cs}
            need = {17, 61, 64} if name.startswith("temporal_stream_kernel<4") else {8, 5} if name.endswith("2>") else {16, 13}
            assert need <= frames, (name, frames)
        else:
            forced = [c for c in cs if c.knobs.get("temporal_budget")]
            natural = [c for c in cs if not c.knobs.get("temporal_budget")]
            assert forced and natural, name
            assert any(dims(c)["D"] % c.troute["PT"] for c in cs) and any(c.troute["HG"] < dims(c)["heads"] for c in cs), name
    peaked = [c for c in CASES if c.name.endswith(",peaked]") or ",peaked]" in c.name]
    assert {c.troute["kernel"] for c in peaked if hasattr(c, "troute")} == {"temporal_stream_kernel<1, 320, 1>", "temporal_stream_kernel<4, 160, 1>"}
    assert any(c.name.startswith("temporal_block") for c in peaked)
    assert C.peaked_rows(16) == [5] and C.peaked_rows(17) == [5, 16] and C.peaked_rows(64) == [5, 21, 37, 53]


def test_group_norm_cases_run_past_one_slab():
    """opcases.gn_slabs / gn_geometry on the GroupNorm cases: three slabs with a ragged last one, the cap_total / NB clamp with more
    than one whole unrolled iteration and a remainder, two sources and the affine form past one slab, every geometry of GN_WIDTHS."""
    old = [C.group_norm_case(**k) for k in C.GN_CASES]
    new = [C.group_norm_case(**k) for k in C.GN_PAST_SLAB + C.GN_VAE]
    assert C.gn_geometry(128) == (16, 1, 16) and 128 not in C.GN_WIDTHS and [(k["silu"], k["eps"], k["P"]) for k in C.GN_VAE] == [(True, 1e-6, 145), (False, 1e-6, 145)]
    shape = lambda c: (C.gn_geometry(c.gn[2]), C.gn_slabs(c.gn[1], c.gn[0], C.gn_geometry(c.gn[2])[2]))
    assert all(shape(c)[1][0] <= 2 and not shape(c)[1][2] for c in old)              # what the suite had: one slab (two at ty = 1), never clamped
    for c in new:
        (tx, vpt, ty), (slabs, rps, clamped) = shape(c)
        nb, P, _ = c.gn
        assert slabs >= 2 and P % rps != 0, c.name                                    # more than one slab, the last ragged
        assert slabs >= 3 or clamped, c.name
    clamped = [c for c in new if shape(c)[1][2]]
    assert clamped
    for c in clamped:
        (_, _, ty), (slabs, rps, _) = shape(c)
        last = c.gn[1] - (slabs - 1) * rps
        per_lane = last // ty
        assert rps // (ty * C.GN_UNROLL) >= 2 and per_lane // C.GN_UNROLL >= 1 and per_lane % C.GN_UNROLL, c.name      # whole iterations and a remainder
        assert (last // ty) // C.GN_UNROLL >= 2, c.name
    assert {C.gn_geometry(w) for w in C.GN_WIDTHS} <= {shape(c)[0] for c in new}
    assert {C.gn_geometry(w)[1:] for w in C.GN_WIDTHS} == {(1, 8), (1, 6), (1, 4), (1, 3), (1, 2), (1, 1), (2, 1)}
    assert any(c.calls[0][1].get("x2") for c in new) and any(c.calls[0][0] == "group_norm_affine" for c in new)
    assert C.gn_slabs(10, 2, 6) == (1, 24, False) and C.gn_slabs(23, 700, 1) == (2, 12, True) and C.gn_slabs(4096, 2, 6)[0] == 171


# ------------------------------------------------------------------ injected defects past the first tile of a workgroup
def bad_rows(case, got, k="y"):
    return offenders(case, got, k).any(1).nonzero().flatten().tolist()


def test_geglu_mlp_second_pass_with_the_first_passes_residual():
    """Workgroup 1 of the capped case adds, in its second pass, the residual rows it loaded for its first (R[] not renewed): the
    rows of tiles 25..32 = 400..527 carry x[row - 128] instead of x[row].  Caught at exactly those 128 rows.  Not a defect rel-L2
    passes: a sixth of the rows is off by a whole residual — asserted as what it is."""
    case = C.geglu_mlp_case(795, False, cap=3)
    _, walk, _ = C.case_walk(case)
    tiles = [t for t, (w, p, _) in enumerate(walk) if (w, p) == (1, 1)]
    assert tiles == list(range(25, 33))
    rows = [16 * t + r for t in tiles for r in range(16)]
    y, x = case.model()["y"], case.inputs["x"].float()
    bad = y.clone()
    bad[rows] = (y[rows].float() - x[rows] + x[[r - 128 for r in rows]]).half()
    with pytest.raises(AssertionError, match=r"geglu_mlp\[M795,cap3\]"):
        case.check({"y": bad})
    assert bad_rows(case, bad) == rows
    assert rel_l2(bad, case.ref["y"][0]) > 100 * TOL_OP


def test_cross_block_tiles_behind_the_video_boundary_on_the_previous_image():
    """Workgroup 0's third pass (tiles 14..18, the first of video 1) computed against video 0's K | V — `imgb` not moved on after
    the cut pass.  Caught at exactly those 80 rows, for the short and the long variant.  Not a defect rel-L2 passes at this size:
    80 rows of 896 with another video's attention term measure 4e-2 against TOL_OP = 2e-3 — asserted as what it is."""
    for L in (77, 160):
        case = C.cross_block_case(4, 224, L, False, cap=3)
        _, walk, _ = C.case_walk(case)
        tiles = [t for t, (w, p, _) in enumerate(walk) if (w, p) == (0, 2)]
        assert tiles == list(range(14, 19))
        rows = [16 * t + r for t in tiles for r in range(16)]
        y = case.model()["y"]
        stale = case.chain(lambda t: t.float(), C.h_, video_of=(0, 0, 2, 3))["y"][0].half()
        bad = y.clone()
        bad[rows] = stale[rows]
        with pytest.raises(AssertionError, match="cross_block"):
            case.check({"y": bad})
        assert bad_rows(case, bad) == rows
        assert rel_l2(bad, case.ref["y"][0]) > 5 * TOL_OP


def test_temporal_stream_third_tile_stored_to_the_second_tiles_rows():
    """temporal_stream_kernel<1, 320, 1> at C = 1280, B = 2, D = 129, F = 13: head group 0's workgroup 0 walks tiles 0, 128, 256 =
    (video 0, pixel 0), (0, 128), (1, 127).  Its third tile's output lands on the second tile's rows (obase taken from the previous
    n) and its own rows keep what they held (zeros here; on the GPU the poison, which run_guarded reports as never written).
    Caught at exactly the 2 x 13 rows of the two tiles, in the 320 columns of head group 0."""
    b, f, dd, c = 2, 13, 129, 1280
    case = C.temporal_attention_case(b, f, dd, c, False)
    rt = case.troute
    assert rt["kernel"] == "temporal_stream_kernel<1, 320, 1>" and (rt["per_group"], rt["tiles"], rt["fullest"]) == (128, 258, 3)
    walk = list(range(0, rt["tiles"], rt["per_group"]))
    assert walk == [0, 128, 256]
    rows_of = lambda t: [((t // dd) * f + fr) * dd + t % dd for fr in range(f)]
    second, third = rows_of(walk[1]), rows_of(walk[2])
    y = case.model()["y"]
    bad = y.clone()
    bad[second, :320] = y[third, :320]
    bad[third, :320] = 0
    with pytest.raises(AssertionError, match="temporal_attention"):
        case.check({"y": bad})
    off = offenders(case, bad)
    assert off.any(1).nonzero().flatten().tolist() == sorted(second + third)
    assert not off[:, 320:].any() and off[sorted(second + third), :320].float().mean() > 0.9
    assert rel_l2(bad, case.ref["y"][0]) > 10 * TOL_OP            # 26 rows of 3354, each wholly wrong in a quarter of its columns: 5e-2


def test_group_norm_last_slab_left_out_of_the_sums():
    """gn_finalize_kernel folds slabs - 1 partials of batch entry 1 (61 rows = slabs of 24, 24 and 13): sums over 48 rows divided by
    the count of 61.  Every row of batch entry 1 is off and no row of batch entry 0."""
    case = C.group_norm_case(nb=2, P=61, c1=320, tag="slabs:")
    (_, _, ty), (slabs, rps, _) = C.gn_geometry(320), C.gn_slabs(61, 2, 6)
    assert (slabs, rps) == (3, 24)
    x, gamma, beta = case.inputs["x1"].float().reshape(2, 61, 32, 10), case.inputs["gamma"], case.inputs["beta"]
    part = x[1, :(slabs - 1) * rps]
    cnt = 61.0 * 10
    mean = part.sum((0, 2)) / cnt
    var = ((part * part).sum((0, 2)) / cnt - mean * mean).clamp_min(0)
    a = (var + 1e-5).rsqrt().repeat_interleave(10) * gamma
    bb = beta - mean.repeat_interleave(10) * a
    bad = case.model()["y"].clone()
    bad[61:] = torch.nn.functional.silu(case.inputs["x1"][61:].float() * a + bb).half()
    with pytest.raises(AssertionError, match="group_norm"):
        case.check({"y": bad})
    assert bad_rows(case, bad) == list(range(61, 122))
    assert rel_l2(bad, case.ref["y"][0]) > 10 * TOL_OP            # a fifth of the rows missing from the statistics: not a defect rel-L2 passes


# ------------------------------------------------------------------ the autoencoder's kernels past one workgroup: walks and injected defects
def test_wide_walk_is_a_bijection_and_the_cases_contain_every_path():
    """opcases.wide_walk (attention_wide.hip:175-187) maps blockIdx onto (batch, head, query block) one to one for every grid size and
    factorisation; the cases of WIDE_PAST contain, between them, a workgroup behind the uneven XCD labels (blockIdx % 8 >= nwg % 8 > 0),
    a query block >= 1, a head >= 1, a block with all four waves full and one with a single query, a ring refill at t >= 2 (five key
    tiles or more) with a last tile of one key, head dims 512 and 256, and kv_batch_div = 2 with lk != lq."""
    for nwg in range(1, 41):
        for nqblk in range(1, nwg + 1):
            for heads in range(1, nwg // nqblk + 1):
                if nwg % (nqblk * heads):
                    continue
                walk = C.wide_walk(nwg, nqblk, heads)
                assert sorted(walk) == [(b, h, q) for b in range(nwg // (nqblk * heads)) for h in range(heads) for q in range(nqblk)], (nwg, nqblk, heads)
    assert C.wide_walk(12, 2, 2) == [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1), (0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
    got = set()
    cases = C.wide_past_cases()
    assert {c.name for c in cases} <= {c.name for c in CASES} and len(cases) == 4 * 5           # every shape has room for every profile at tile 32
    for c in cases:
        a = c.calls[0][1]
        walk, ntile = C.wide_case_walk(c)
        nwg, xr = len(walk), len(walk) & 7
        assert C.key_tile(a["dh"]) == 32
        got |= {"uneven_xcd_labels"} if xr and any(bid & 7 >= xr for bid in range(nwg)) else set()
        got |= {"query_block_1"} if any(q >= 1 for _, _, q in walk) else set()
        got |= {"head_1"} if any(h >= 1 for _, h, _ in walk) else set()
        got |= {"four_full_waves"} if a["Lq"] >= C.WIDE_QBLK else set()
        got |= {"one_query_block"} if a["Lq"] % C.WIDE_QBLK == 1 else set()
        got |= {"refill_at_t2"} if ntile >= 5 else set()               # `if (t + 2 < ntile)` at t = 2: K(4) into the slot K(2) leaves, which held K(0)
        got |= {"last_tile_of_one_key"} if a["Lk"] % 32 == 1 else set()
        got |= {"kv_batch_div_2"} if a["kv_batch_div"] == 2 and a["Lk"] != a["Lq"] else set()
        got |= {f"dh{a['dh']}"}
        # creep has room at this kernel's tile in every shape (attention_case asserts through assert_profile, on the values the kernel gets, that
        # consecutive 32-key tile maxima rise by 3..8 log2 units and by more than 8 in all: a rescale deferred on some tiles, taken on others)
        assert C.profile_applies("creep", a["Lq"], a["Lk"], 32) and (a["Lk"] > 128 or not C.profile_applies("creep", a["Lq"], a["Lk"]))
        if c.hard and c.hard["creep"]:
            assert ntile >= 4 and c.hard["creep"] == C.hard_rows(a["Lq"])
    assert got == {"uneven_xcd_labels", "query_block_1", "head_1", "four_full_waves", "one_query_block", "refill_at_t2", "last_tile_of_one_key",
                   "kv_batch_div_2", "dh512", "dh256"}, sorted(got)
    assert sum(1 for c in cases if c.name.endswith(",creep]")) == 4
    # what the suite had: one workgroup, three key tiles at most
    old = [c for c in CASES if getattr(c, "route", None) == "wide" and c not in cases]
    assert old and all(len(C.wide_case_walk(c)[0]) == 1 and C.wide_case_walk(c)[1] <= 3 for c in old)


def test_edge_conv_cases_take_a_second_quad_and_a_second_step():
    """opcases.edge_out_walk / edge_in_walk on the new cases: quads_per_wg = 2 with the in-loop break and the one-pixel tile in the last
    workgroup; a second grid-stride step that is exactly the bottom image row; and what the older cases had."""
    assert C.edge_out_walk(131841) == (1031, 2) and C.edge_out_walk(131072) == (2048, 1) and C.edge_out_walk(131073) == (1025, 2)
    assert C.edge_out_walk(126) == (2, 1) and C.edge_out_walk(320) == (5, 1)
    where, breaks = C.edge_out_tiles(131841)
    assert len(where) == 8241 and 131841 - 8240 * 16 == 1 and where[8240] == (1030, 0, 0) and where[8239] == (1029, 1, 3)
    assert breaks[1030] == [1, 0, 0, 0] and all(breaks[b] == [None] * 4 for b in range(1030))
    big = [c for c in C.vae_cases() if c.name.startswith("conv_edge_out[") and C.edge_out_walk(c.edge[0])[1] == 2]
    assert {c.name for c in big} == {"conv_edge_out[1x128->3,257x513,float32]", "conv_edge_out[1x8->8,257x513,float16]"}
    old = [C.edge_out_case(*e, dt) for e in C.EDGE_OUT for dt in (C.f16, C.f32t)]
    assert all(C.edge_out_walk(c.edge[0])[1] == 1 and C.edge_out_walk(c.edge[0])[0] <= 2 for c in old)
    rolled = [c.calls[0][1]["Cin"] for c in C.vae_cases() if c.name.startswith("conv_edge_out[") and c.calls[0][1]["Cin"] not in (128, 256, 512)]
    assert sorted(set(rolled)) == [8, 40]                                # one partly guarded block; two blocks, the last of 8 channels
    grid, steps = C.edge_in_walk(16512, 512)
    assert grid == 4096 and steps == [2] * 32 + [1] * 4064
    assert 4096 * 256 // 64 == 16384 == 128 * 128 and 16512 * 64 - 4096 * 256 == 32 * 256     # the second step: the bottom row of 129 x 128, all of it
    assert all(max(C.edge_in_walk(*c.edge)[1]) == 2 for c in C.vae_cases() if c.name.startswith("conv_edge_in["))
    assert all(max(C.edge_in_walk(*C.edge_in_case(*e, dt, tap).edge)[1]) == 1 for e in C.EDGE_IN for dt in (C.f16, C.f32t) for tap in (False, True))


def test_conv_edge_out_second_quad_stored_to_the_first_quads_pixels():
    """Workgroup 515 of the 257 x 513 case stores its second quad (tiles 4124..4127) at the pixel offsets of its first (4120..4123):
    the first quad's 64 pixels hold the second's results and the second's keep what they held (zeros here; on the GPU the poison,
    which run_guarded reports as never written).  Caught at exactly those 128 pixels.  Not a defect rel-L2 passes: 128 of 131841
    pixels wholly wrong measure 3e-2 against TOL_OP = 2e-3 — asserted as what it is."""
    case = C.edge_out_case(1, 128, 3, 257, 513, C.f32t)
    where, _ = C.edge_out_tiles(case.edge[0])
    first, second = ([16 * t + i for t in sorted(t for t, (b, q, _) in where.items() if (b, q) == (515, k)) for i in range(16)] for k in (0, 1))
    assert first == list(range(515 * 128, 515 * 128 + 64)) and second == list(range(515 * 128 + 64, 516 * 128))
    y = case.model()["y"]
    bad = y.clone().reshape(3, -1)
    bad[:, first] = y.reshape(3, -1)[:, second]
    bad[:, second] = 0
    bad = bad.reshape(y.shape)
    with pytest.raises(AssertionError, match=r"conv_edge_out\[1x128->3,257x513,float32\]"):
        case.check({"y": bad})
    assert offenders(case, bad).reshape(3, -1).any(0).nonzero().flatten().tolist() == first + second
    assert 10 * TOL_OP < rel_l2(bad, case.ref["y"][0]) < 0.1


def test_conv_edge_in_second_grid_stride_step_skipped():
    """Workgroups 0..31 leave the loop after one step: items >= 4096 * 256 = the 128 pixels of the bottom image row are never written,
    which run_guarded reports at pixel 16384.  With zeros there instead of the poison rel-L2 measures 9e-2: not a defect it passes."""
    case = C.edge_in_case(1, 4, 512, 129, 128, C.f16, True)
    grid, steps = C.edge_in_walk(*case.edge)
    done = grid * 256 // (512 // 8)
    assert done == 16384 and max(steps) == 2
    y = case.model()["y"]

    def fn(i, o):
        o["y"][:done] = y[:done]
    with pytest.raises(AssertionError, match=r"y: %d elements never written, first at offset %d .*row 16384, column 0" % (128 * 512, 16384 * 512)):
        oc.run_guarded(fn, case.inputs, case.outputs, device="cpu")
    bad = y.clone()
    bad[done:] = 0
    assert bad_rows(case, bad) == list(range(16384, 16512))
    assert rel_l2(bad, case.ref["y"][0]) > 10 * TOL_OP


def test_wide_attention_wave_3_rows_taken_from_wave_2():
    """Query block 0 of the 161-token case: wave 3 (rows 96..127) stores what wave 2 computed (rows 64..95).  Caught at exactly those 32
    rows.  Not a defect rel-L2 passes: a fifth of the rows is another row's output — asserted as what it is."""
    for c in (512, 256):
        case = C.attention_case(1, 161, c, heads=1, tile=32)
        y = case.model()["y"]
        bad = y.clone()
        bad[96:128] = y[64:96]
        with pytest.raises(AssertionError, match=r"attention\[nb1,lq161"):
            case.check({"y": bad})
        assert bad_rows(case, bad) == list(range(96, 128))
        assert rel_l2(bad, case.ref["y"][0]) > 100 * TOL_OP


def test_wide_attention_key_tile_read_from_the_slots_previous_occupant():
    """The workgroup of query block 0 reads, for every key tile t >= 2, the K rows its ring slot held before: keys of tile t - 2 (the
    refill never landed); V and the mask of the last tile are right, so the single key of tile 5 scores as key 96.  Every row of query
    block 0 is off and the one row of query block 1 (another workgroup) is not.  Not a defect rel-L2 passes — asserted as what it is."""
    case = C.attention_case(1, 161, 512, heads=1, tile=32)
    walk, ntile = C.wide_case_walk(case)
    assert walk == [(0, 0, 0), (0, 0, 1)] and ntile == 6
    qkv = case.inputs["qkvw"]
    q, k, v = qkv[:, :512], qkv[:, 520:1032], qkv[:, 1040:]
    stale = k.clone()
    for t in range(2, ntile):
        n = min(32, 161 - 32 * t)
        stale[32 * t:32 * t + n] = k[32 * (t - 2):32 * (t - 2) + n]
    assert torch.equal(stale[160], k[96]) and torch.equal(stale[64:96], k[:32]) and torch.equal(stale[:64], k[:64])
    bad = case.model()["y"].clone()
    bad[:128] = C.attn_model(q[:128], stale, v, 512 ** -0.5, False)
    with pytest.raises(AssertionError, match=r"attention\[nb1,lq161"):
        case.check({"y": bad})
    assert bad_rows(case, bad) == list(range(128))
    assert rel_l2(bad, case.ref["y"][0]) > 100 * TOL_OP


# ------------------------------------------------------------------ bands and poison, on CPU tensors
def test_guard_geometry_and_patterns():
    for dtype, pattern in ((torch.float16, oc.NAN16), (torch.float32, oc.NAN32)):
        g = oc.guarded((3, 5), dtype, fill="nan", device="cpu")
        esz = g.t.element_size()
        assert g.lo * esz >= 64 * 1024 and g.lo * esz % 512 == 0 and g.hi * esz >= 64 * 1024 and g.hi * esz % 512 == 0
        assert g.t.is_contiguous() and g.t.shape == (3, 5) and g.t.isnan().all() and g.unwritten().numel() == 15
        assert int(g.buf[0]) & (0xFFFF if esz == 2 else 0xFFFFFFFF) == pattern
        g.check_bands()
        g.poison("finite")
        assert (g.t == torch.tensor(oc.SENTINEL, dtype=dtype)).all() and g.unwritten().numel() == 0
    x = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    gi = oc.guarded_like(x, band="zero", device="cpu")
    assert torch.equal(gi.t, x) and int(gi.buf[0]) == 0
    gi.check_unchanged()
    gi.t[1, 2] = 7
    with pytest.raises(AssertionError, match="row 1, column 2"):
        gi.check_unchanged("x")


def test_band_damage_is_located():
    g = oc.guarded((4, 8), torch.float16, device="cpu")
    g.buf[g.lo + 32 + 3] = 0                     # three elements past the end: "row 4, column 3"
    with pytest.raises(AssertionError, match=r"offset 35 .*row 4, column 3"):
        g.check_bands("y")
    g = oc.guarded((4, 8), torch.float16, device="cpu")
    g.buf[g.lo - 2] = 0
    with pytest.raises(AssertionError, match="offset -2 "):
        g.check_bands("y")


def run_cpu(fn, alias=None):
    x = torch.arange(12, dtype=torch.float16).reshape(3, 4)
    return oc.run_guarded(fn, {"x": x}, {"y": ((3, 4), torch.float16)}, alias=alias, device="cpu")


def test_run_guarded_accepts_a_correct_op_and_an_in_place_one():
    assert torch.equal(run_cpu(lambda i, o: o["y"].copy_(i["x"] * 2))["y"], torch.arange(12).reshape(3, 4) * 2.0)
    assert torch.equal(run_cpu(lambda i, o: o["y"].mul_(2), alias={"y": "x"})["y"], torch.arange(12).reshape(3, 4) * 2.0)


def test_run_guarded_catches_unwritten_rows_stray_stores_and_stray_reads():
    with pytest.raises(AssertionError, match="4 elements never written, first at offset 8 .*row 2, column 0"):
        run_cpu(lambda i, o: o["y"][:2].copy_(i["x"][:2]))

    def store_past_the_end(i, o):
        o["y"].copy_(i["x"])
        torch.as_strided(o["y"], (13,), (1,))[12] = 1.0
    with pytest.raises(AssertionError, match="y .*guard band damaged in 1 elements, first at offset 12 .*row 3, column 0"):
        run_cpu(store_past_the_end)

    def clobbers_its_input(i, o):
        o["y"].copy_(i["x"])
        i["x"][0, 1] = 9
    with pytest.raises(AssertionError, match="x: input changed in 1 elements, first at offset 1 "):
        run_cpu(clobbers_its_input)

    def reads_past_the_input(i, o):            # a halo read that should have been masked: the result depends on the band
        o["y"].copy_(i["x"])
        past = torch.as_strided(i["x"], (13,), (1,))[12]
        o["y"][2, 3] += 0.0 if past.isnan() else 1.0
    with pytest.raises(AssertionError, match="depend on what surrounds the operands.*row 2, column 3"):
        run_cpu(reads_past_the_input)

    def accumulates_into_its_output(i, o):     # a split-K slab that was never zeroed
        o["y"].add_(i["x"])
    with pytest.raises(AssertionError):
        run_cpu(accumulates_into_its_output)


def test_assert_elementwise_reports_count_and_worst_and_rejects_nan():
    ref = torch.ones(2, 3, dtype=torch.float64)
    got = ref.clone().half()
    oc.assert_elementwise(got, ref, ref, 0.0)
    got[1, 2] = 1.01
    got[0, 1] = 1.001
    with pytest.raises(AssertionError, match=r"2 of 6 elements.*\(row 1, column 2\)"):
        oc.assert_elementwise(got, ref, ref, 0.0, where=oc.loc_rows(3))
    got = ref.clone().half()
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 6 elements.*\(row 0, column 0\)"):
        oc.assert_elementwise(got, ref, ref, 1.0, where=oc.loc_rows(3))


# ------------------------------------------------------------------ the launches only the encoder and FVD objects reach (enccases.py)
import enccases as E            # noqa: E402


def pinned_offenders(case, bad64):
    """the defective float64 result, stored as the kernel stores it, is rejected by the case's own check; returns where"""
    got = bad64.half()
    with pytest.raises(AssertionError, match="outside the bound"):
        case.check({"y": got})
    return case.offenders(got)


def exactly(case, off, bad64, region):
    """Rejected at exactly the affected elements: no element outside `region`, and inside it every element the defect moves by more
    than the stored value can hide (its own rounding on top of the bound); what is left is a fraction of a percent whose defective
    value rounds to the right fp16 number or its neighbour."""
    ref, scale = case.ref
    visible = (bad64 - ref).abs() > 2.01 * oc.U16 * ref.abs() + case.c * scale
    assert not (off & ~region).any() and not (visible & ~region).any()
    assert (off | ~visible).all()
    assert off[region].float().mean() > 0.99 and off[region.any(1)].any(1).all() and off[:, region.any(0)].any(0).all()


def test_pinned_reference_passes_its_own_check_and_the_case_list_is_the_issues():
    for case in (E.pinned_case(77, 128, 256), E.pinned_case(77, 384, 128, "table"), E.pinned_case(77, 384, 128, "sigma8")):
        case.check({"y": case.ref[0].half()})
        case.check({"y": case.model()}, label="model ")
    names = [c.name for c in E.pinned_cases()]
    assert len(names) == len(set(names)) == 2 * 16 + 6 * 5 + 2 * 6 - 2          # (77, separate) of the two form pairs is a ragged case too
    assert len(E.ragged_cases()) == 32 and len(E.edge_cases()) == 30 and len(E.form_cases()) == 12
    assert {(c.N, c.K) for c in E.ragged_cases()} == {p for pairs in E.PAIRS.values() for p in pairs} and len(E.PAIRS) == 4
    assert max(c.K for c in E.ragged_cases()) == 4096 == max(c.N for c in E.ragged_cases())


def test_pinned_last_k_tile_dropped():
    """K = 256 = four K-tiles, the loop ending one tile early: every element misses 64 of its products"""
    case = E.pinned_case(77, 128, 256)
    a, w = case.inputs["a"].double(), case.inputs["w"].double()
    bad = case.ref[0] - a[:, 192:] @ w[:, 192:].t()
    exactly(case, pinned_offenders(case, bad), bad, torch.ones(77, 128, dtype=torch.bool))
    assert rel_l2(bad.half(), case.ref[0]) > 10 * TOL_OP        # (a quarter of the terms: not a defect rel-L2 passes)


def test_pinned_bias_of_the_neighbouring_column_tile():
    """the second 128-column tile finished with the first tile's bias quads: its columns and no others"""
    case = E.pinned_case(77, 384, 128)
    bias = case.inputs["bias"].double()
    bad = case.ref[0].clone()
    bad[:, 128:256] += bias[:128] - bias[128:256]
    region = torch.zeros(77, 384, dtype=torch.bool)
    region[:, 128:256] = True
    exactly(case, pinned_offenders(case, bad), bad, region)


def test_pinned_residual_row_of_the_next_block():
    """M = 2 x 77: block 0 adds the residual rows of block 1 (a row offset taken from the wrong image): rows 0..76 and no others"""
    case = E.pinned_case(154, 384, 128)
    r = case.inputs["r"].double()
    bad = case.ref[0].clone()
    bad[:77] += r[77:] - r[:77]
    region = torch.zeros(154, 384, dtype=torch.bool)
    region[:77] = True
    exactly(case, pinned_offenders(case, bad), bad, region)


def test_pinned_clamped_row_stored_to_the_row_behind_a_ragged_tile():
    """Rows 77..127 of the one tile are clamped to row M - 1 = 76 for their loads; stored unguarded, row 76's values land on row 77:
    behind the tensor.  Every value inside is right: only the guard band sees it, and names the row.  With the output a column block
    of a wider buffer the same store lands in the band too."""
    for form, width in (("separate", 128), ("c_block", 128 + 2 * E.BLOCK)):
        case = E.pinned_case(77, 128, 128, form)
        y = case.ref[0].half()
        col0 = E.BLOCK if form == "c_block" else 0

        def fn(i, o):
            o["y"][:, col0:col0 + 128] = y
            torch.as_strided(o["y"], (78, width), (width, 1))[77, col0:col0 + 128] = y[76]
        with pytest.raises(AssertionError, match=r"y .*guard band damaged in 128 elements, first at offset %d .*row 77, column %d" % (77 * width + col0, col0)):
            oc.run_guarded(fn, case.inputs, case.outputs, device="cpu", partial=case.partial)
        got = oc.run_guarded(lambda i, o: o["y"][:, col0:col0 + 128].copy_(y), case.inputs, case.outputs, device="cpu", partial=case.partial)
        case.check(got)                                           # without the stray store: nothing to report


def test_pinned_store_into_the_columns_beside_a_column_block():
    case = E.pinned_case(77, 128, 128, "c_block")
    y = case.ref[0].half()

    def fn(i, o):
        o["y"][:, E.BLOCK:E.BLOCK + 128] = y
        o["y"][5, E.BLOCK + 128] = 1.0
    with pytest.raises(AssertionError, match=r"y: 1 elements outside the written region were stored to, first at offset .*row 5, column %d" % (E.BLOCK + 128)):
        oc.run_guarded(fn, case.inputs, case.outputs, device="cpu", partial=case.partial)


def fold_bits_rejected(case, **defect):
    out, shift = E.fold_reference(**case["arrays"], **defect)
    cin = case["inputs"]["w"].shape[1]
    bad = torch.from_numpy(out)
    with pytest.raises(AssertionError, match="differ in their bits") as e:
        oc.assert_bits(bad, case["out"], where=E.loc_packed(cin, case["kpad"]), label="fold")
    return bad.view(torch.int16) != case["out"].view(torch.int16), torch.from_numpy(shift), str(e.value)


@pytest.mark.parametrize("label", [gm[0] for gm in E.FOLD_GEOMETRIES])
def test_fold_defects_are_rejected_bit_for_bit(label):
    case = E.fold_case(label)
    cout, cin = case["inputs"]["w"].shape[:2]
    taps = case["k"] // cin
    oc.assert_bits(torch.from_numpy(E.fold_reference(**case["arrays"])[0]), case["out"])
    assert case["double_rounding_differs"] >= 1
    # eps left out: the channel with var = 0 becomes inf (NaN where the weight is 0); the others move by 5e-6 relative: a few elements each
    diff, shift, _ = fold_bits_rejected(case, use_eps=False)
    assert diff[E.VAR0_CHANNEL, :case["k"]].all() and not diff[:, case["k"]:].any()
    assert (shift.view(torch.int32) != case["shift"].view(torch.int32))[E.VAR0_CHANNEL]
    # fp32 as an intermediate rounding: exactly the elements counted, the planted ones among them, and the shift untouched
    diff, shift, msg = fold_bits_rejected(case, via_fp32=True)
    assert int(diff.sum()) == case["double_rounding_differs"] and f"{case['double_rounding_differs']} of" in msg
    assert all(diff[co, 0] for co in (0, E.VAR0_CHANNEL, E.NEG_GAMMA_CHANNEL)) and "(cout 0, tap 0, cin 0)" in msg
    assert torch.equal(shift, case["shift"])
    # tap and ci exchanged: [Cout][Cin][taps] copied through.  One tap: the two orders are one order, the defect is none
    if taps == 1:
        oc.assert_bits(torch.from_numpy(E.fold_reference(**case["arrays"], swap=True)[0]), case["out"])
    else:
        diff, _, msg = fold_bits_rejected(case, swap=True)
        assert diff[:, :case["k"]].float().mean() > 0.9 and "(cout 0, tap 0, cin 1)" in msg          # element 1 holds (tap 1, cin 0)'s weight
    # the sign of a negative gamma reaches the weights: element 0 of that row is (tap 0, cin 0) in either layout
    assert float(case["out"][E.NEG_GAMMA_CHANNEL, 0]) * float(case["arrays"]["w"][E.NEG_GAMMA_CHANNEL].reshape(-1)[0]) < 0
    assert float(case["out"][0, 0]) * float(case["arrays"]["w"][0].reshape(-1)[0]) > 0


def test_add_rows_sum_converted_by_truncation_is_rejected():
    """the fp32 sum cut to fp16 toward zero instead of rounded to nearest (a conversion built from shifts): off by one unit in a
    quarter of the elements (many sums of two fp16 values are fp16 values themselves), far inside the tolerance of a model test,
    rejected by the bit comparison"""
    case = E.add_rows_case(2, 77, 768)
    x, pos = case["inputs"]["x"], case["inputs"]["pos"]
    trunc = ((x.float() + pos.float()).view(torch.int32) & ~0x1FFF).view(torch.float32).half()
    assert 0.1 < float((trunc != case["want"]).float().mean()) < 0.5 and rel_l2(trunc, case["want"].double()) < TOL_OP
    with pytest.raises(AssertionError, match="differ in their bits"):
        oc.assert_bits(trunc, case["want"], label="add_rows")
