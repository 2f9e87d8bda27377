"""-m gpu: the producer-side norm statistics per element (tests/statcheck.py; DESIGN.md, "Producer statistics per element").
GEMM-family cases of tests/opcases.py run once more with the statistics sink armed (lavie_debug_op_statistics): C against the case's
float64 reference under its own bound, the column / row partials against float64 sums of the C that was written, in exactly sized,
NaN-poisoned buffers between NaN bands.  gn_fold_kernel and rowstat_finalize_kernel against float64 of the partials handed in, and
both chained behind a real producer."""
import pytest
import torch

import opcases as C
import opcheck as oc
import statcheck as S

pytestmark = pytest.mark.gpu
f16, f32t, f64 = torch.float16, torch.float32, torch.float64


def stats_runs():
    return [pytest.param(c, v, id=f"{c.name}-{v}") for c, v, _ in C.gemm_runs(C.stats_cases())]


def plan_of(ops, case, fs):
    """the plan of the case's launch with its kinds armed, from the library (nothing is launched)"""
    i = {k: v.cuda() for k, v in case.inputs.items()}
    o = {k: i[case.alias[k]] if k in case.alias else torch.empty(shape, dtype=dt, device="cuda") for k, (shape, dt) in case.outputs.items()}
    with ops.op_statistics(plan=("cs" in case.kind, "rs" in case.kind)):
        if case.base.setup is not None:
            with case.base.setup(tuple(fs)):
                case.base.run(ops, i, o)
        else:
            case.base.run(ops, i, o)
    torch.cuda.synchronize()
    return S.plan_of_info(ops.op_statistics.last())


def run_stats_case(ops, case, fs):
    plan = plan_of(ops, case, fs)
    (M, N), _ = case.outputs["y"]
    assert (plan["M"], plan["N"]) == (M, N) and plan["colstat"] == ("cs" in case.kind) and plan["rowstat"] == ("rs" in case.kind), plan
    outputs = dict(case.outputs)
    if "cs" in case.kind:
        outputs["cs"] = ((plan["cs_floats"],), f32t)
    if "rs" in case.kind:
        outputs["rs"] = ((M, plan["slots"], 2), f32t)

    def fn(i, o):
        if case.setup is not None:
            with case.setup(tuple(fs)):
                case.run(ops, i, o)
        else:
            case.run(ops, i, o)
    got = oc.run_guarded(fn, case.inputs, outputs, alias=case.alias, sync=torch.cuda.synchronize)
    assert S.plan_of_info(ops.op_statistics.last()) == plan
    case.check(got)                                     # C itself, statistics armed: the case's float64 reference and bound
    if "cs" in case.kind:
        S.check_colstat(got["y"], got["cs"], plan, parity=case.parity, label=f"colstat[{case.name}]")
    if "rs" in case.kind:
        S.check_rowstat(got["y"], got["rs"], plan, label=f"rowstat[{case.name}]")
    return got, plan


@pytest.mark.parametrize("case,variant", stats_runs())
def test_gemm_statistics(case, variant):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from lavie_amd import ops as o
    fs = case.force if variant == "forced" else C.VARIANTS[variant]
    with C.forced(*fs, (0, 0)):
        run_stats_case(o, case, fs)


def test_undersized_sink_is_refused_before_the_launch():
    from lavie_amd import ops as o
    case = C.with_stats(C.linear_case(161, 320, 320, "plain"), "cs+rs")
    plan = plan_of(o, case, (0, 0))
    i = {k: oc.guarded_like(v) for k, v in case.inputs.items()}
    y, cs, rs = oc.guarded((161, 320), f16), oc.guarded((plan["cs_floats"] - 1,), f32t), oc.guarded((161, plan["slots"], 2), f32t)
    with pytest.raises(RuntimeError, match=f"this launch writes {plan['cs_floats']}"):
        case.run(o, {k: g.t for k, g in i.items()}, {"y": y.t, "cs": cs.t, "rs": rs.t})
    torch.cuda.synchronize()
    for g in (y, cs, rs):
        g.check_bands("refused")
        assert g.unwritten().numel() == g.n


# ------------------------------------------------------------------ gn_fold_kernel: synthetic partials through lavie_group_norm_stats_f16
def run_fold(case):
    """one call on guarded operands: bands, inputs, y written, producer-count delta; returns (y, ws head) on the CPU"""
    from lavie_amd import _lib, ops
    nb, P, ctot = case.gn
    ws_n = _lib.load().lavie_group_norm_ws_floats(nb, case.groups)
    gi = {k: oc.guarded_like(v) for k, v in case.inputs.items()}
    y, ws = oc.guarded(case.outputs["y"][0], f16), oc.guarded((ws_n,), f32t)
    n0 = _lib.load().lavie_debug_gn_producer_count()
    case.run(ops, {k: g.t for k, g in gi.items()}, {"y": y.t, "ws": ws.t})
    torch.cuda.synchronize()
    folds = _lib.load().lavie_debug_gn_producer_count() - n0
    for k, g in {**gi, "y": y, "ws": ws}.items():
        g.check_bands(k)
    for k, g in gi.items():
        g.check_unchanged(k)
    assert y.unwritten().numel() == 0
    return y.t.cpu(), ws, folds


@pytest.mark.parametrize("shape", C.GN_FOLD, ids=[str(s) for s in C.GN_FOLD])
def test_gn_fold(shape):
    """(mean, rstd) of the fold against float64 of the partials handed in, under the derived bound; y against the float64 GroupNorm of
    the tensor under the group_norm bound; exactly one producer fold counted; the fold writes (mean, rstd) and nothing else"""
    case = C.gn_fold_case(*shape)
    nb, P, ctot = case.gn
    y, ws, folds = run_fold(case)
    assert folds == 1
    head = nb * case.groups * 2
    stray = ws.unwritten()
    assert stray.numel() == ws.n - head and int(stray.min()) == head, "the fold writes (mean, rstd) and nothing else"
    S1, A1, S2, n = S.fold_terms(case.descs, nb, P, case.groups)
    S.check_mean_rstd(ws.t[:head].reshape(nb, case.groups, 2), S1, A1, S2, n, float(P * (ctot // case.groups)), 1e-5, f"gn_fold[{case.name}]",
                      lambda i: "(batch %d, group %d)" % divmod(i, case.groups))
    case.check({"y": y})


@pytest.mark.parametrize("poisoned", [0, 1])
def test_gn_fold_reads_its_own_batch_only(poisoned):
    """NB = 2 with the other batch entry's blocks holding NaN: this entry's rows meet the bound, the other's come out NaN"""
    from lavie_amd import ops
    import copy
    nb, P, c = 2, 160, 320
    case = copy.copy(C.gn_fold_case(nb, P, c, 0, 80, 1, None, 0.0))
    case.inputs = dict(case.inputs, p1=case.inputs["p1"].clone())
    v = case.inputs["p1"].reshape(4, -1)               # four blocks of 80 rows, two per batch entry
    v[2 * poisoned:2 * poisoned + 2] = float("nan")
    y, ws, folds = run_fold(case)
    assert folds == 1
    keep = 1 - poisoned
    ref, scale = case.ref["y"]
    rows = slice(keep * P, (keep + 1) * P)
    oc.assert_elementwise(y[rows], ref[rows], scale[rows], case.c, where=oc.loc_rows(c), label=f"gn_fold batch {keep} beside NaN partials")
    assert bool(y[poisoned * P:(poisoned + 1) * P].float().isnan().all())


@pytest.mark.parametrize("why", list(C.GN_UNUSABLE))
def test_unusable_descriptor_takes_the_two_pass_path(why):
    """same output bound, no producer fold counted"""
    case = C.gn_fold_case(2, 160, 320, 0, 80, 1, None, 0.0, **C.GN_UNUSABLE[why])
    y, ws, folds = run_fold(case)
    assert folds == 0 and not case.usable, why
    case.check({"y": y})


# ------------------------------------------------------------------ rowstat_finalize_kernel
@pytest.mark.parametrize("M,slots,offset", C.ROWSTAT_FINALIZE)
def test_rowstat_finalize(M, slots, offset):
    from lavie_amd import ops
    case = C.rowstat_finalize_case(M, slots, offset)
    got = oc.run_guarded(lambda i, o: case.run(ops, i, o), case.inputs, case.outputs, sync=torch.cuda.synchronize)
    S.check_finalize(got["out"], case.inputs["p"], case.row_len, 1e-5, label=case.name)


# ------------------------------------------------------------------ chained behind a real producer
def test_chain_rowstat_finalize_lnfold():
    """linear (row statistics armed) -> rowstat_finalize -> linear_lnfold against float64 LayerNorm + Linear of the producer's written
    rows, under the lnfold bound (opcases.lnfold_case's reference, with the float64 statistics of those rows)"""
    from lavie_amd import ops
    M, N, K = 161, 320, 320
    prod = C.with_stats(C.linear_case(M, N, K, "bias_residual"), "rs")
    with C.forced(3, 0, (0, 0)):
        got, plan = run_stats_case(ops, prod, (3, 0))
    a = got["y"]                                        # fp16 rows as written: the consumer's input
    g = C.gen("chain_ln", M, N)
    gamma, beta = 1 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    w = torch.randn(256, N, generator=g) / N ** 0.5
    wf = (w * gamma).half()
    s, bf = wf.float().sum(1), (w @ beta + torch.randn(256, generator=g))
    stats = ops.rowstat_finalize(got["rs"].cuda(), N, 1e-5)
    S.check_finalize(stats, got["rs"], N, 1e-5, label="chain:rowstat_finalize")
    y = ops.linear_lnfold(a.cuda(), wf.cuda(), bf.cuda(), s.cuda(), stats)
    torch.cuda.synchronize()
    a64 = a.to(f64)
    mean, rstd = a64.mean(1, keepdim=True), (a64.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    # the folded form with float64 statistics of the rows = LayerNorm + Linear with the fp16 folded weight; scale as lnfold_case
    ref = rstd * (a64 @ wf.to(f64).t() - mean * s.to(f64)) + bf.to(f64)
    scale = rstd.abs() * (a64.abs() @ wf.to(f64).abs().t() + (mean * s.to(f64)).abs()) + bf.to(f64).abs()
    # the consumer's statistics are within (dm, dr) of the float64 statistics of the partials (check_finalize above), which are within
    # |mean_p - mean|, |rstd_p - rstd| of the rows' own (the partials met their bound in run_stats_case): triangle inequality, then
    # d(rstd) scales the bracket and d(mean) enters through rstd s_n
    p = got["rs"].to(f64)
    mean_p, rstd_p, dm, dr = S.stats_bound(p[..., 0].sum(1), p[..., 0].abs().sum(1), p[..., 1].sum(1), plan["slots"], float(N), 1e-5)
    dm, dr = dm + (mean_p - mean[:, 0]).abs(), dr + (rstd_p - rstd[:, 0]).abs()
    slack = dr[:, None] * (a64.abs() @ wf.to(f64).abs().t() + (mean * s.to(f64)).abs()) + rstd * dm[:, None] * s.to(f64).abs()
    got_y = y.cpu().to(f64)
    bound = oc.U16 * ref.abs() + oc.gemm_c(N + 2) * scale + slack
    bad = ~((got_y - ref).abs() <= bound)
    assert not bool(bad.any()), f"{int(bad.sum())} elements outside the lnfold bound, first at {oc.loc_rows(256)(int(bad.reshape(-1).nonzero()[0]))}"


def test_chain_gn_fold_apply():
    """conv3x3 on the halo-patch kernel (column statistics armed) -> group_norm_stats (one producer fold) against the float64 GroupNorm of
    the conv's written output under the group_norm bound"""
    from lavie_amd import _lib, ops
    prod = C.with_stats(C.conv_case(**C.HALO_CASES[1], force=5), "cs")          # 1 x 64 -> 160, 40 x 16: 640 rows, blocks of 80
    got, plan = run_stats_case(ops, prod, prod.force)
    x = got["y"]
    nb, P, c = 2, 320, 160
    g = C.gen("chain_gn")
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    cs = got["cs"].cuda()
    d = ops.producer_stats(cs, c, plan["rows"], plan["sets"], plan["set_blocks"], plan["span"])
    n0 = _lib.load().lavie_debug_gn_producer_count()
    y = ops.group_norm_stats(x.cuda(), gamma.cuda(), beta.cuda(), nb, 32, 1e-5, True, cs1=d)
    torch.cuda.synchronize()
    assert _lib.load().lavie_debug_gn_producer_count() - n0 == 1
    cpg = c // 32
    xg = x.to(f64).reshape(nb, P, 32, cpg)
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    a = (var + 1e-5).rsqrt().repeat_interleave(cpg, 1) * gamma.to(f64)
    bb = beta.to(f64) - mean.repeat_interleave(cpg, 1) * a
    xr = x.to(f64).reshape(nb, P, c)
    ref, sc = C.silu64(xr * a[:, None] + bb[:, None]), 1.1 * ((xr * a[:, None]).abs() + bb[:, None].abs())
    oc.assert_elementwise(y, ref.reshape(-1, c), sc.reshape(-1, c), oc.round_c(1), where=oc.loc_rows(c), label="chain:gn_fold -> apply")


def test_worst_fractions_are_reported(capsys):
    """runs last in this file: prints the worst observed fraction of each derived bound (recorded in DESIGN.md; nothing is asserted on it
    beyond what every check above already did)"""
    with capsys.disabled():
        for k, v in sorted(S.WORST.frac.items()):
            print(f"\nworst fraction of bound: {k}: {v:.3f}", end="")
    assert all(v <= 1.0 for v in S.WORST.frac.values())
