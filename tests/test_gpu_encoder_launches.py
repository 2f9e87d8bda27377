"""-m gpu: the launches only the encoder and FVD objects reach, each through an operator entry that calls the function
the objects call: the pinned GEMM plan of the text encoder, the vision tower and the mapper per element and in its bit properties,
the BatchNorm-folding conv pack of lavie_r3d_finalize bit for bit against a one-rounding NumPy reference, the mapper's add_rows bit
for bit; refusals.  Cases: tests/enccases.py."""
import pytest
import torch

import enccases as E
import opcheck as oc

pytestmark = pytest.mark.gpu


def sync():
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ------------------------------------------------------------------ pinned_linear, per element
def run_pinned(case):
    from lavie_amd import ops
    got = oc.run_guarded(lambda i, o: case.run(ops, i, o), case.inputs, case.outputs, alias=case.alias, partial=case.partial, sync=sync)
    case.check(got)
    print(f"{case.name}: worst |err| / bound = {oc.WORST.get(case.name, float('nan')):.3f}")
    return got


RAGGED, EDGES, FORMS = E.ragged_cases(), E.edge_cases(), E.form_cases()


@pytest.mark.parametrize("case", RAGGED, ids=[c.name for c in RAGGED])
def test_pinned_linear_every_encoder_pair_at_ragged_row_counts(case):
    run_pinned(case)


@pytest.mark.parametrize("case", EDGES, ids=[c.name for c in EDGES])
def test_pinned_linear_row_counts_around_the_tile(case):
    run_pinned(case)


@pytest.mark.parametrize("case", FORMS, ids=[c.name for c in FORMS])
def test_pinned_linear_operand_forms(case):
    got = run_pinned(case)
    if case.form == "sigma8":
        assert float(case.take(got).abs().max()) > 8.0


# ------------------------------------------------------------------ pinned_linear, bit properties (no tolerance)
def device_operands(M, N, K):
    c = E.pinned_case(M, N, K)
    return {k: v.cuda() for k, v in c.inputs.items()}


@pytest.mark.parametrize("block,batches", [(77, (2, 3, 16)), (257, (2, 3))])
@pytest.mark.parametrize("N,K", [(384, 128), (768, 3072)])
def test_pinned_linear_block_of_a_batch_has_the_bits_of_its_own_launch(block, batches, N, K):
    """rows block i .. block i + block - 1 of an M = block B launch equal the M = block launch of those rows: for every B and i"""
    from lavie_amd import ops
    for B in batches:
        dev = device_operands(block * B, N, K)
        whole = ops.pinned_linear(dev["a"], dev["w"], dev["bias"], residual=dev["r"])
        again = ops.pinned_linear(dev["a"], dev["w"], dev["bias"], residual=dev["r"])
        assert torch.equal(bits(whole), bits(again)), (B, "two calls differ")
        for i in range(B):
            rows = slice(block * i, block * (i + 1))
            one = ops.pinned_linear(dev["a"][rows], dev["w"], dev["bias"], residual=dev["r"][rows])
            oc.assert_bits(one, whole[rows].cpu(), where=oc.loc_rows(N), label=f"pinned_linear[{N}x{K}] block {i} of {B} x {block} rows")


def test_pinned_linear_aliased_residual_gives_the_bits_of_a_separate_one():
    from lavie_amd import ops
    for N, K in E.FORM_PAIRS:
        dev = device_operands(129, N, K)
        want = ops.pinned_linear(dev["a"], dev["w"], dev["bias"], residual=dev["r"])
        buf = dev["r"].clone()
        ops.pinned_linear(dev["a"], dev["w"], dev["bias"], residual=buf, out=buf)
        assert torch.equal(bits(buf), bits(want)), (N, K)


CONTROL = (77, 1280, 768)          # N a multiple of 128 (the pinned plan) and of 320 (force_tile 3 moves the planner's kernel), 12 K-tiles


def planned(ops, dev):
    """the plan of the planner-routed linear of the same operands under the switches in force (planned, not launched)"""
    with ops.op_statistics(plan=(1, 0)):
        ops.linear(dev["a"], dev["w"], bias=dev["bias"], residual=dev["r"])
    return ops.op_statistics.last()


@pytest.mark.parametrize("switch,value", [("lavie_debug_force_tile", 3), ("lavie_debug_force_splits", 3)])
def test_force_switches_do_not_reach_the_pinned_plan(switch, value):
    """The output bits under the switch equal the unforced ones.  The control shows that the switch was live: the planner-routed
    ops.linear of the same operands plans another launch under it (lavie_debug_op_statistics_last) and still meets its bound."""
    from lavie_amd import _lib, ops
    lib = _lib.load()
    case = E.pinned_case(*CONTROL)
    dev = {k: v.cuda() for k, v in case.inputs.items()}
    free = ops.pinned_linear(dev["a"], dev["w"], dev["bias"], residual=dev["r"])
    plan_free = planned(ops, dev)
    try:
        _lib.check(getattr(lib, switch)(value), switch)
        forced = ops.pinned_linear(dev["a"], dev["w"], dev["bias"], residual=dev["r"])
        plan_forced = planned(ops, dev)
        control = ops.linear(dev["a"], dev["w"], bias=dev["bias"], residual=dev["r"])
        sync()
    finally:
        lib.lavie_debug_force_tile(0)
        lib.lavie_debug_force_splits(0)
    assert plan_forced != plan_free, (switch, plan_free)
    if switch.endswith("splits"):
        assert (plan_free["splits"], plan_forced["splits"]) == (1, value)
    else:
        assert (plan_free["colstat_rows"], plan_forced["colstat_rows"]) == (64, 80)       # the 128-row kernel, then the 160-row ping-pong one
    oc.assert_bits(forced, free.cpu(), where=case.where, label=f"pinned_linear under {switch}({value})")
    oc.assert_elementwise(control, *case.ref, oc.gemm_c(case.K + 3), where=case.where, label=f"linear under {switch}({value})")
    assert planned(ops, dev) == plan_free                                                   # and the switch is off again


# ------------------------------------------------------------------ conv3d_fold_pack, bit for bit
@pytest.mark.parametrize("label", [gm[0] for gm in E.FOLD_GEOMETRIES])
def test_conv3d_fold_pack_is_one_rounding_of_the_double_product(label):
    from lavie_amd import ops
    case = E.fold_case(label)
    n_double = case["double_rounding_differs"]
    print(f"fold {label}: {n_double} of {case['out'].numel()} elements round differently through fp32")
    assert n_double >= 1                   # a kernel that rounds through fp32 cannot pass the comparison below
    cout, cin = case["inputs"]["w"].shape[:2]

    def fn(i, o):
        ops.pack_conv3d_fold(i["w"], i["gamma"], i["beta"], i["mean"], i["var"], eps=E.FOLD_EPS, out=o["wp"], shift=o["shift"])
    got = oc.run_guarded(fn, case["inputs"], {"wp": (tuple(case["out"].shape), torch.float16), "shift": ((cout,), torch.float32)}, sync=sync)
    oc.assert_bits(got["wp"], case["out"], where=E.loc_packed(cin, case["kpad"]), label=f"fold {label}: packed weights")
    oc.assert_bits(got["shift"], case["shift"], label=f"fold {label}: shift")
    assert not got["wp"][:, case["k"]:].any()


@pytest.mark.parametrize("label", [gm[0] for gm in E.FOLD_GEOMETRIES])
def test_conv3d_pack_is_the_fold_with_an_identity_batchnorm(label):
    """gamma = 1, beta = 0, mean = 0 and var = 1, eps = 0: the scale is exactly 1 (an fp32 var exists for it because eps is an argument
    of the entry; at eps = 1e-5 none would: 1 - 1e-5 is not an fp32 value), so the fold of w16.float() is pack_conv3d of w16 and a
    zero shift."""
    from lavie_amd import ops
    case = E.fold_case(label)
    w16 = case["inputs"]["w"].half().cuda()
    cout = w16.shape[0]
    one, zero = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
    wp, shift = ops.pack_conv3d_fold(w16.float(), one, zero, zero, one, eps=0.0)
    oc.assert_bits(wp, ops.pack_conv3d(w16).cpu(), label=f"fold {label}: identity BatchNorm")
    assert not shift.any()


# ------------------------------------------------------------------ add_rows, exact
@pytest.mark.parametrize("shape", E.ADD_ROWS_SHAPES, ids=str)
def test_add_rows_is_one_rounding_of_the_fp32_sum(shape):
    """out separate from x: the one form the mapper uses (image_engine.cpp: the caller's text rows into the workspace)"""
    from lavie_amd import ops
    case = E.add_rows_case(*shape)
    got = oc.run_guarded(lambda i, o: ops.add_rows(i["x"], i["pos"], out=o["y"]), case["inputs"], {"y": (shape, torch.float16)}, sync=sync)["y"]
    c = shape[2]
    oc.assert_bits(got, case["want"], where=lambda i: "(batch %d, row %d, column %d)" % (i // c // shape[1], i // c % shape[1], i % c),
                   label=f"add_rows {shape}")


# ------------------------------------------------------------------ refusals
def refused(word, fn):
    with pytest.raises(RuntimeError, match=word):
        fn()


def test_operands_the_encoders_cannot_form_are_refused_by_name():
    from lavie_amd import _lib, ops
    lib = _lib.load()
    h = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
    f = lambda *s: torch.zeros(*s, device="cuda")
    a, w, b, y = h(77, 128), h(256, 128), f(256), h(77, 256)
    p = lambda t: None if t is None else t.data_ptr()

    def pin(A=a, lda=128, W=w, bias=b, R=None, ldr=256, C=y, ldc=256, M=77, N=256, K=128):
        return lambda: _lib.check(lib.lavie_pinned_linear_f16(p(A), lda, p(W), p(bias), p(R), ldr, p(C), ldc, M, N, K, None), "lavie_pinned_linear_f16")
    pin()()
    for kw, word in ((dict(A=None), "null tensor"), (dict(W=None), "null tensor"), (dict(bias=None), "null tensor"), (dict(C=None), "null tensor"),
                     (dict(M=0), "M=0"), (dict(N=192, ldc=192), "N=192 must be a multiple of 128"), (dict(N=64, ldc=64), "N=64"),
                     (dict(K=96, lda=96), "K=96 must be a multiple of 64"), (dict(lda=120), "lda=120"), (dict(ldc=252), "ldc=252"),
                     (dict(R=y, ldr=254), "ldr=254"), (dict(A=a[0, 4:]), "16-byte aligned")):
        refused(word, pin(**kw))
    with pytest.raises(ValueError, match="unit column stride"):
        ops.pinned_linear(a.t(), w, b)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.pinned_linear(a.float(), w, b)
    with pytest.raises(ValueError, match="must have shape"):
        ops.pinned_linear(a, w, b, residual=y[:76])
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.pinned_linear(a, w, b.half())
    sync()
    assert not y.any()                       # and no refused call launched anything that wrote

    x, pos = h(3, 7, 128), h(7, 128)
    add = lambda X=x, P=pos, O=x.clone(), B=3, L=7, C=128: (lambda: _lib.check(lib.lavie_add_rows_f16(p(X), p(P), p(O), B, L, C, None), "lavie_add_rows_f16"))
    add()()
    for kw, word in ((dict(X=None), "null tensor"), (dict(P=None), "null tensor"), (dict(O=None), "null tensor"), (dict(C=100), "C=100"),
                     (dict(C=4), "C=4"), (dict(B=0), "B=0"), (dict(L=0), "L=0")):
        refused(word, add(**kw))
    with pytest.raises(ValueError, match="x must be"):
        ops.add_rows(x, pos[:6])
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.add_rows(x.float(), pos)

    wf, bn = f(64, 64, 3, 3, 3), f(64)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.pack_conv3d_fold(wf.half(), bn, bn, bn, bn)
    with pytest.raises(ValueError, match=r"fp32 \[64\]"):
        ops.pack_conv3d_fold(wf, bn, bn, bn[:32], bn)
    with pytest.raises(ValueError, match="outside what"):
        ops.pack_conv3d_fold(f(64, 64, 3, 8, 3), bn, bn, bn, bn)
    out = h(64, 1728)
    refused("null BatchNorm tensor", lambda: _lib.check(lib.lavie_conv3d_fold_pack_f32(p(wf), None, p(bn), p(bn), p(bn), 1e-5, p(out), p(bn), 64, 64, 3, 3, 3,
                                                                                      None), "lavie_conv3d_fold_pack_f32"))
    refused("null tensor", lambda: _lib.check(lib.lavie_conv3d_fold_pack_f32(None, p(bn), p(bn), p(bn), p(bn), 1e-5, p(out), p(bn), 64, 64, 3, 3, 3, None),
                                              "lavie_conv3d_fold_pack_f32"))
