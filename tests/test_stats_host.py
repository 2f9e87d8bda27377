"""The statistics checks of tests/statcheck.py before a GPU is involved: a host model of the partials a launch leaves (fp32 sums of the
rounded C, in the layout of the plan `hostcheck optrace` prints for the case) meets every bound; each injected defect is caught at
exactly the entries it touches; the reach of the statistics cases from the library's own planner.  CPU only, needs hipcc."""
import shutil

import pytest
import torch

import opcases as C
import opcheck as oc
import statcheck as S

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
f32t, f64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def reach():
    return C.gemm_reach(list(C.stats_cases()) + list(C.stats_local_cases()))


def plan_of(reach, case, variant):
    (line,) = C.NOTES[(case.name, variant)]
    return S.parse_stats_line(line)


PARITY_SPLIT = {C.parity_case(n, c, h, w).name + "+cs" for n, c, h, w, _ in C.PARITY_SPLIT_CASES}


def small(case):
    (M, N), _ = case.outputs["y"]
    return M * N <= 3_000_000 or case.name in PARITY_SPLIT          # (the 2-split parity case has 5.7e6 outputs: modelled all the same)


def test_host_model_meets_every_bound(reach):
    """every statistics case whose output is small: the fp32 model of C, its fp32 block / slot sums, checked like the kernel's"""
    n, split_parity = 0, []
    for c, v, _ in C.gemm_runs(C.stats_cases()):
        plan = plan_of(reach, c, v)
        if c.name in PARITY_SPLIT:      # the reduce behind the parity launch: 32-row contiguous blocks of OUTPUT rows in one set, not four parity sets
            assert (plan["rows"], plan["span"], plan["sets"], plan["contiguous"], plan["set_blocks"]) == (32, 32, 1, 1, plan["M"] // 32), (c.name, plan)
            assert plan["splits"] == {C.parity_case(*s[:4]).name + "+cs": s[4] for s in C.PARITY_SPLIT_CASES}[c.name] and c.parity is not None
            split_parity.append(c.name)
        assert plan["colstat"] == ("cs" in c.kind) and plan["rowstat"] == ("rs" in c.kind) and plan["splits"] >= 1, (c.name, v, plan)
        if plan["colstat"]:
            assert plan["set_blocks"] == (-(-plan["M"] // plan["rows"]) if plan["sets"] == 1 else plan["M"] // 4 // plan["rows"]), plan
            assert plan["sets"] * plan["set_blocks"] <= plan["blocks_stored"] <= plan["sets"] * plan["set_blocks"] + 1 and plan["span"] % (plan["rows"] * plan["sets"]) == 0
        if not small(c):
            continue
        y = c.base.model()["y"]
        if plan["colstat"] and plan["contiguous"]:
            S.check_colstat(y, S.model_colstat(y, plan, parity=c.parity), plan, parity=c.parity, label=c.name)
            n += 1
        if plan["rowstat"]:
            S.check_rowstat(y, S.model_rowstat(y, plan), plan, label=c.name)
            n += 1
    assert n >= 32 and sorted(split_parity) == sorted(PARITY_SPLIT)


def test_armed_row_statistics_plan_an_unsplit_launch(reach):
    name = "linear[2689x512x192,bias_residual]"
    split = C.gemm_reach([C.linear_case(2689, 512, 192, "bias_residual")])[(name, "split-k-3")]
    assert "splitk_reduce_kernel" in [C.launch_name(l) for l in split]
    armed = reach[(name + "+rs", "split-k-3")]
    assert [C.launch_name(l) for l in armed] == ["igemm_kernel<2, 2, 4, 2, 2, false, 0>"] and C.launch_grid(armed[0])[1] == 1
    assert plan_of(reach, C.with_stats(C.linear_case(2689, 512, 192, "bias_residual"), "rs"), "split-k-3")["splits"] == 1


def caught(fn, *texts):
    with pytest.raises(AssertionError) as e:
        fn()
    for t in texts:
        assert t in str(e.value), (t, str(e.value))


@pytest.fixture(scope="module")
def pp(reach):
    """linear 161 x 320 x 320 on the ping-pong kernel, both kinds: three blocks of 80 rows announced (the last holds one row), four stored"""
    case = next(c for c in C.stats_cases() if c.name == "linear[161x320x320,bias_residual]+cs+rs")
    plan = plan_of(reach, case, "pingpong")
    assert (plan["rows"], plan["set_blocks"], plan["blocks_stored"], plan["cols"], plan["slots"]) == (80, 3, 4, 80, 4)
    y = case.base.model()["y"]
    return case, plan, y, S.model_colstat(y, plan), S.model_rowstat(y, plan)


def test_block_that_drops_its_last_row(pp):
    case, plan, y, cs, rs = pp
    s, q = S.cs_unpack(cs.clone(), 320)
    s, q = s.clone(), q.clone()
    s[1] -= y[159].float()
    q[1] -= y[159].float() ** 2
    caught(lambda: S.check_colstat(y, S.cs_pack(s, q), plan), "span sums", "blocks 1..1")
    caught(lambda: S.check_colstat(y, S.cs_pack(s, q), plan), "320 of 320 entries")            # every channel of that block, and no other block
    ok_s, ok_q = (t.clone() for t in S.cs_unpack(cs.clone(), 320))
    S.check_colstat(y, S.cs_pack(ok_s, ok_q), plan)


def test_ragged_block_that_counts_the_clamped_row(pp):
    """rows past M read the clamped row M - 1: counted, the last block holds 80 times its only row"""
    case, plan, y, cs, rs = pp
    s, q = (t.clone() for t in S.cs_unpack(cs.clone(), 320))
    s[2], q[2] = 80 * y[160].float(), 80 * y[160].float() ** 2
    caught(lambda: S.check_colstat(y, S.cs_pack(s, q), plan), "rows 160..160", "blocks 2..2")
    z = cs.clone()
    z[3 * 640 + 5] = 1.0                              # the padding block must hold zeros
    caught(lambda: S.check_colstat(y, z, plan), "padding block")


def test_sums_and_squares_exchanged(pp):
    case, plan, y, cs, rs = pp
    s, q = S.cs_unpack(cs.clone(), 320)
    caught(lambda: S.check_colstat(y, S.cs_pack(q, s), plan), "span sums", "span 0")


def test_row_slot_written_to_the_neighbouring_slot(pp):
    case, plan, y, cs, rs = pp
    bad = rs.clone()
    bad[:, 1], bad[:, 2] = rs[:, 2], rs[:, 1]
    caught(lambda: S.check_rowstat(y, bad, plan), "slot sums", "322 of 644 entries")           # slots 1 and 2 of each of the 161 rows
    nan = rs.clone()
    nan[160, 3] = float("nan")                        # a slot never written
    caught(lambda: S.check_rowstat(y, nan, plan), "never written")


def test_parity_set_indexed_with_the_blocks_of_the_output_rows(reach):
    """set j at j * cdiv(M, rows) instead of j * (M / 4 / rows): sets 1..3 land past their place"""
    n, c, h, w = C.PARITY_CASES[0]
    case = next(x for x in C.stats_cases() if x.parity and x.base.calls[0][1]["NI"] == n)
    plan = plan_of(reach, case, "auto")
    assert (plan["sets"], plan["set_blocks"], plan["rows"], plan["span"]) == (4, 4, 80, 640)
    y = case.base.model()["y"]
    good = S.model_colstat(y, plan, parity=case.parity)
    S.check_colstat(y, good, plan, parity=case.parity)
    s, q = S.cs_unpack(good, c)
    wrong = plan["M"] // plan["rows"]                  # 16 blocks per "set"
    bs, bq = torch.zeros(4 * wrong, c), torch.zeros(4 * wrong, c)
    for j in range(4):
        bs[j * wrong:j * wrong + 4], bq[j * wrong:j * wrong + 4] = s[j * 4:(j + 1) * 4], q[j * 4:(j + 1) * 4]
    bad = S.cs_pack(bs[:16], bq[:16])                  # what lands inside the exactly sized buffer (the rest hits the guard band)
    caught(lambda: S.check_colstat(y, bad, plan, parity=case.parity), "set 1")


def fold_setup(shape):
    case = C.gn_fold_case(*shape)
    nb, P, ctot = case.gn
    S1, A1, S2, n = S.fold_terms(case.descs, nb, P, case.groups)
    return case, nb, P, ctot, (S1, A1, S2, n)


def fp32_fold(S1, S2, count, eps=1e-5):
    mean = (S1.float() * (1.0 / count)).float()
    var = (S2.float() * (1.0 / count) - mean * mean).clamp_min(0)
    return torch.stack([mean, (var + eps).rsqrt()], -1)


@pytest.mark.parametrize("shape", C.GN_FOLD, ids=[str(s) for s in C.GN_FOLD])
def test_fold_model_meets_its_bound(shape):
    case, nb, P, ctot, (S1, A1, S2, n) = fold_setup(shape)
    count = float(P * (ctot // case.groups))
    S.check_mean_rstd(fp32_fold(S1, S2, count), S1, A1, S2, n, count, 1e-5, "fold model", lambda i: str(divmod(i, case.groups)))


def test_fold_reading_a_block_of_the_next_batch():
    case, nb, P, ctot, (S1, A1, S2, n) = fold_setup(C.GN_FOLD[1])          # 2 x 160 rows, blocks of 80: bpd = 2
    part, c, rows, nsets, sb = case.descs[0]
    s, q = (t.to(f64) for t in S.cs_unpack(part, c))
    cpg = ctot // case.groups
    extra_s, extra_q = s[2].reshape(case.groups, cpg).sum(1), q[2].reshape(case.groups, cpg).sum(1)      # batch 1's first block, read by batch 0
    bad1, bad2 = S1.clone(), S2.clone()
    bad1[0] += extra_s
    bad2[0] += extra_q
    count = float(P * cpg)
    caught(lambda: S.check_mean_rstd(fp32_fold(bad1, bad2, count), S1, A1, S2, n, count, 1e-5, "fold", lambda i: "(batch %d, group %d)" % divmod(i, case.groups)),
           "(batch 0, group")
    got = fp32_fold(bad1, bad2, count)
    got[0] = fp32_fold(S1, S2, count)[0]
    S.check_mean_rstd(got, S1, A1, S2, n, count, 1e-5, "fold", lambda i: str(i))       # batch 1 is untouched by the defect


def test_fold_including_channel_hi_of_a_straddling_quad():
    """60 channels per group over 1280 + 640: group g ends inside a quad whenever 60 (g + 1) % 4 != 0 — never; 10 per group over 320
    does (hi = 10, 30, ...): the quad's next channel belongs to the next group"""
    case, nb, P, ctot, (S1, A1, S2, n) = fold_setup(C.GN_FOLD[1])
    part, c, rows, nsets, sb = case.descs[0]
    s, q = (t.to(f64).reshape(nb, -1, c) for t in S.cs_unpack(part, c))
    cpg = ctot // case.groups
    assert cpg == 10
    bad1, bad2 = S1.clone(), S2.clone()
    hit = [g for g in range(case.groups - 1) if (g + 1) * cpg % 4 != 0]
    for g in hit:
        bad1[:, g] += s[:, :, (g + 1) * cpg].sum(1)
        bad2[:, g] += q[:, :, (g + 1) * cpg].sum(1)
    count = float(P * cpg)
    with pytest.raises(AssertionError) as e:
        S.check_mean_rstd(fp32_fold(bad1, bad2, count), S1, A1, S2, n, count, 1e-5, "fold", lambda i: "(batch %d, group %d)" % divmod(i, case.groups))
    assert f"{2 * len(hit)} of {2 * case.groups} entries" in str(e.value), str(e.value)


def test_second_tile_from_the_previous_tile_is_caught_by_c_alone(reach):
    """The persistent kernel's miscounted vmcnt releases the next tile's operands early: a tile's C rows come from the tile before.  The
    statistics of such a launch are sums of the C it wrote, so the statistics check, computed from the written C, passes; the check of
    C against its float64 reference is what catches it."""
    case = next(c for c in C.stats_cases() if c.name == "linear[320x256x320,bias_residual]+cs")
    plan = plan_of(reach, case, "ppx-persistent")
    y = case.base.model()["y"]
    bad = y.clone()
    bad[160:320] = y[0:160]
    S.check_colstat(bad, S.model_colstat(bad, plan), plan)                 # consistent with what was written: passes
    with pytest.raises(AssertionError) as e:
        case.check({"y": bad})
    assert "(row 1" in str(e.value) or "(row 2" in str(e.value) or "(row 3" in str(e.value), str(e.value)
    case.check({"y": y})


@pytest.mark.parametrize("M,slots,offset", [(257, 5, 0.0), (257, 5, 8.0), (1, 1, 8.0)])
def test_finalize_model_meets_its_bound(M, slots, offset):
    case = C.rowstat_finalize_case(M, slots, offset)
    p = case.inputs["p"]
    got = fp32_fold(p[..., 0].sum(1), p[..., 1].sum(1), float(case.row_len))
    S.check_finalize(got, p, case.row_len, 1e-5)
    if slots > 1:                                      # the last slot left out of one row's sums
        q = p.clone()
        q[M - 1, slots - 1] = 0
        bad = got.clone()
        bad[M - 1] = fp32_fold(q[..., 0].sum(1), q[..., 1].sum(1), float(case.row_len))[M - 1]
        caught(lambda: S.check_finalize(bad, p, case.row_len, 1e-5), f"(row {M - 1})", "1 of %d entries" % M)
