"""Per-element checks of the producer-side norm statistics ("Producer statistics per element"): the sums and sums of
squares the GEMM-family kernels leave in their epilogues for a consuming GroupNorm ("column statistics") or LayerNorm ("row
statistics"), and the two kernels that turn them into (mean, rstd).  A plain module like opcheck.py: the host tests run it on CPU
tensors and a host model of the statistics, the GPU tests on what the kernels wrote.

The statistics are DEFINED over the rounded fp16 values the kernel stored, so every check here reads the written C back and sums it
in float64: a statistics defect is not blurred by the GEMM's own tolerance (which the case's existing bound checks on C itself).

    sum of n terms o_i:            |got - sum o_i|   <= (n + 8) 2^-23 sum |o_i|
    sum of n squares:              |got - sum o_i^2| <= (n + 9) 2^-23 sum o_i^2        (one more rounding per term: the product)

n = rows per block (column statistics), 16 NT = columns per slot (row statistics).  `plan` everywhere is the dict of
lavie_op_statistics_info (ops.op_statistics.last(), or the "## stats" line of `hostcheck optrace`).  Nothing in here is measured."""
import math

import torch

import opcheck as oc

f32t, f64 = torch.float32, torch.float64
U32 = oc.U32
RSQRT_ULP = 2.0        # assumed: no accuracy table for the device library's rsqrtf ships with the ROCm headers or documents of this tree


class Worst:
    """worst observed fraction of each bound, by label (recorded in DESIGN.md; never read by an assertion)"""

    def __init__(self):
        self.frac = {}

    def note(self, label, err, bound):
        r = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        self.frac[label] = max(self.frac.get(label, 0.0), r)


WORST = Worst()


def cs_unpack(buf, C):
    """flat column-statistics buffer -> (sums [blocks, C], squares [blocks, C]) by the layout of igemm.h cs_index: per block and
    channel quad four sums, then four sums of squares"""
    v = buf.reshape(-1, C // 4, 2, 4)
    return v[:, :, 0, :].reshape(-1, C), v[:, :, 1, :].reshape(-1, C)


def cs_pack(sums, squares):
    blocks, C = sums.shape
    return torch.stack([sums.reshape(blocks, C // 4, 4), squares.reshape(blocks, C // 4, 4)], 2).reshape(-1).contiguous()


def parity_of_rows(M, Ho, Wo):
    """output parity py * 2 + px of each channels-last row of [(n Ho Wo), C]: the set that holds the row in the parity form"""
    r = torch.arange(M)
    y, x = (r // Wo) % Ho, r % Wo
    return (y % 2) * 2 + (x % 2)


def _assert(err, bound, label, where):
    bad = ~(err <= bound)
    if bool(bad.any()):
        ratio = torch.where(bad, torch.where(err.isnan(), torch.full_like(err, math.inf), err / bound.clamp_min(1e-300)), torch.zeros_like(err))
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{label}: {int(bad.sum())} of {err.numel()} entries outside the bound; worst at {where(i)}: |err| {err.reshape(-1)[i].item():.3e} > "
                             f"bound {bound.reshape(-1)[i].item():.3e}")


def _sets_of_rows(M, plan, parity):
    if plan["nsets"] == 1:
        return torch.zeros(M, dtype=torch.long)
    assert plan["nsets"] == 4 and parity is not None, "four sets: the parity form, which needs the output grid (Ho, Wo)"
    return parity_of_rows(M, *parity)


def check_colstat(y, buf, plan, parity=None, label="colstat"):
    """y [M, C]: the C the kernel wrote, read back; buf: the statistics buffer, exactly plan["cs_floats"] floats.
    Per span for every launch: the blocks of set j whose rows lie in the aligned run s of plan["span"] rows — blocks
    [s, s + 1) span / (rows nsets) of the set, the assignment GnColStat::span states and gn_fold_kernel relies on — add up to the
    column sums of the rows of that run that belong to set j.  Per block where the plan says blocks are contiguous rows.  Every block
    the launch stores past the announced ones (tile padding) holds exact zeros."""
    M, C = y.shape
    rows, span, nsets, sb = plan["rows"], plan["span"], plan["sets"], plan["set_blocks"]
    plan = dict(plan, nsets=nsets)
    assert buf.numel() == plan["cs_floats"] == plan["blocks_stored"] * 2 * C, (buf.numel(), plan)
    buf = buf.detach().cpu()
    assert not bool(buf.isnan().any()), f"{label}: {int(buf.isnan().sum())} statistics entries are NaN / never written"
    s_all, q_all = (t.to(f64) for t in cs_unpack(buf, C))
    announced = nsets * sb
    pad = torch.cat([s_all[announced:], q_all[announced:]])
    assert not bool((pad != 0).any()), f"{label}: a padding block past the {announced} announced ones holds a non-zero entry"
    o = y.detach().cpu().to(f64)
    set_of = _sets_of_rows(M, plan, parity)
    assert span % (rows * nsets) == 0, (span, rows, nsets)
    bps = span // (rows * nsets)                     # blocks of one span inside a set
    nspans = -(-M // span)
    assert sb <= nspans * bps, (sb, nspans, bps)

    def sums_over(mask_rows):
        sel = o[mask_rows]
        return sel.sum(0), sel.abs().sum(0), (sel * sel).sum(0)

    c1, c2 = (rows + 8) * U32, (rows + 9) * U32
    r = torch.arange(M)
    for j in range(nsets):
        for s in range(nspans):
            ref_s, abs_s, ref_q = sums_over((r // span == s) & (set_of == j))
            b0, b1 = j * sb + s * bps, j * sb + min((s + 1) * bps, sb)
            got_s, got_q = s_all[b0:b1].sum(0), q_all[b0:b1].sum(0)
            where = lambda i, j=j, s=s: f"(set {j}, span {s} = rows {s * span}..{min(M, (s + 1) * span) - 1}, blocks {b0}..{b1 - 1}, channel {i})"
            WORST.note(label.split("[")[0] + ":span sums", (got_s - ref_s).abs(), c1 * abs_s)
            WORST.note(label.split("[")[0] + ":span squares", (got_q - ref_q).abs(), c2 * ref_q)
            _assert((got_s - ref_s).abs(), c1 * abs_s, f"{label}: span sums", where)
            _assert((got_q - ref_q).abs(), c2 * ref_q, f"{label}: span sums of squares", where)
    if plan["contiguous"]:
        # block b of set j: rows [b rows, (b + 1) rows) of the set's own row order — output rows (one set), or for the parity form the
        # outputs of source rows [b rows, (b + 1) rows) at parity j, which are the rows of set j in ascending order
        for j in range(nsets):
            idx = (set_of == j).nonzero().flatten()
            nb = -(-idx.numel() // rows)
            assert nb == sb, (nb, sb)
            padded = torch.zeros(nb * rows, C, dtype=f64)
            padded[:idx.numel()] = o[idx]
            blk = padded.reshape(nb, rows, C)
            ref_s, abs_s, ref_q = blk.sum(1), blk.abs().sum(1), (blk * blk).sum(1)
            got_s, got_q = s_all[j * sb:(j + 1) * sb], q_all[j * sb:(j + 1) * sb]
            where = lambda i, j=j: "(set %d, block %d, channel %d)" % (j, i // C, i % C)
            WORST.note(label.split("[")[0] + ":block sums", (got_s - ref_s).abs(), c1 * abs_s)
            WORST.note(label.split("[")[0] + ":block squares", (got_q - ref_q).abs(), c2 * ref_q)
            _assert((got_s - ref_s).abs(), c1 * abs_s, f"{label}: block sums", where)
            _assert((got_q - ref_q).abs(), c2 * ref_q, f"{label}: block sums of squares", where)


def check_rowstat(y, rs, plan, label="rowstat"):
    """y [M, N] as written; rs [M, slots, 2]: slot k of row m = (sum, sum of squares) of columns [k cols, (k + 1) cols)"""
    M, N = y.shape
    cols, slots = plan["cols"], plan["slots"]
    assert cols * slots == N and tuple(rs.shape) == (M, slots, 2) and rs.numel() == plan["rs_floats"], (tuple(rs.shape), plan)
    rs = rs.detach().cpu().to(f64)
    assert not bool(rs.isnan().any()), f"{label}: {int(rs.isnan().sum())} row-statistics entries are NaN / never written"
    o = y.detach().cpu().to(f64).reshape(M, slots, cols)
    ref_s, abs_s, ref_q = o.sum(2), o.abs().sum(2), (o * o).sum(2)
    where = lambda i: "(row %d, slot %d)" % divmod(i, slots)
    c1, c2 = (cols + 8) * U32, (cols + 9) * U32
    WORST.note(label.split("[")[0] + ":slot sums", (rs[..., 0] - ref_s).abs(), c1 * abs_s)
    WORST.note(label.split("[")[0] + ":slot squares", (rs[..., 1] - ref_q).abs(), c2 * ref_q)
    _assert((rs[..., 0] - ref_s).abs(), c1 * abs_s, f"{label}: slot sums", where)
    _assert((rs[..., 1] - ref_q).abs(), c2 * ref_q, f"{label}: slot sums of squares", where)


# ------------------------------------------------------------------ host model of the statistics a launch leaves (fp32 sums of the rounded C)
def model_colstat(y, plan, parity=None):
    """The buffer a correct launch leaves, for kernels whose blocks are contiguous rows of their set (plan["contiguous"]): fp32 sums
    in ascending row order, zeros in the padding blocks"""
    assert plan["contiguous"]
    M, C = y.shape
    rows, nsets, sb = plan["rows"], plan["sets"], plan["set_blocks"]
    set_of = _sets_of_rows(M, dict(plan, nsets=nsets), parity)
    s = torch.zeros(plan["blocks_stored"], C, dtype=f32t)
    q = torch.zeros_like(s)
    o = y.float()
    for j in range(nsets):
        idx = (set_of == j).nonzero().flatten()
        for b in range(sb):
            sel = o[idx[b * rows:(b + 1) * rows]]
            s[j * sb + b], q[j * sb + b] = sel.sum(0), (sel * sel).sum(0)
    return cs_pack(s, q)


def model_rowstat(y, plan):
    M, N = y.shape
    o = y.float().reshape(M, plan["slots"], plan["cols"])
    return torch.stack([o.sum(2), (o * o).sum(2)], 2).contiguous()


# ------------------------------------------------------------------ (mean, rstd) from partials: gn_fold_kernel, rowstat_finalize_kernel
def stats_bound(S1, A1, S2, n, count, eps):
    """Reference and bound of (mean, rstd) computed in fp32 as  mean = (sum a_i) inv,  var = max((sum b_i) inv - mean^2, 0),
    rstd = rsqrtf(var + eps),  inv = 1.0f / count  from n fp32 partials a_i (sums, A1 = sum |a_i|) and b_i (sums of squares, >= 0).
    u = 2^-23 throughout (twice the unit roundoff of fp32: the factor covers the order of the sums, which is not modelled).
      mean:  the n-term sum (n + 8) u A1 / count, then inv (one division, and for GroupNorm one product of two exact integers: <= u),
             then the product with inv (u / 2):                                dm <= ((n + 8) A1 / count + 2 |mean|) u
      E[x^2] likewise with sum b_i = sum |b_i|:                                 dq <= ((n + 8) + 2) q u
      var = q - mean^2:  d(mean^2) <= 2 |mean| dm + dm^2 + u mean^2 (the product's rounding), the subtraction rounds once more:
                         dv <= dq + 2 |mean| dm + dm^2 + u mean^2 + u |var|     — the cancellation is in here: dq and u mean^2 are
                         relative to q and mean^2, not to var, so an offset mean of 8 sigma costs 65 (n + 11) u relative in var
      rstd = (var + eps)^-1/2:  |d rstd| <= rstd / 2 * dv' / (v - dv'), dv' = dv + u v (the addition of eps), v = var + eps, plus
                         RSQRT_ULP ulp of the device library's rsqrtf:          dr <= rstd (dv' / (2 (v - dv')) + RSQRT_ULP u)
    Returns mean, rstd, dm, dr (float64)."""
    u = U32
    mean, q = S1 / count, S2 / count
    dm = ((n + 8) * A1 / count + 2 * mean.abs()) * u
    dq = (n + 10) * q * u
    var = (q - mean * mean).clamp_min(0)
    dv = dq + 2 * mean.abs() * dm + dm * dm + u * mean * mean + u * var
    v = var + eps
    dv = dv + u * v
    rstd = v.rsqrt()
    assert bool((v > 2 * dv).all()), "the variance is lost in the cancellation at this shape: no meaningful bound"
    dr = rstd * (dv / (2 * (v - dv)) + RSQRT_ULP * u)
    return mean, rstd, dm, dr


def fold_terms(descs, NB, P, groups):
    """descs: [(partials fp32 CPU flat, C, rows, nsets, set_blocks)] of the concatenated tensors, in order.  Float64 sums over exactly
    the entries gn_fold_kernel's contract names: every set, the blocks [nb bpd, (nb + 1) bpd) of the domain, the channels of the group.
    Returns S1, A1, S2 [NB, groups] and the term count n of the largest group."""
    ctot = sum(d[1] for d in descs)
    cpg = ctot // groups
    S1, A1, S2 = (torch.zeros(NB, groups, dtype=f64) for _ in range(3))
    n = 0
    c0 = 0
    per_group_terms = torch.zeros(groups, dtype=torch.long)
    for part, C, rows, nsets, sb in descs:
        s, q = (t.to(f64).reshape(nsets, sb, C) for t in cs_unpack(part, C))
        bpd = P // (rows * nsets)
        for g in range(groups):
            lo, hi = max(g * cpg, c0) - c0, min((g + 1) * cpg, c0 + C) - c0
            if hi <= lo:
                continue
            per_group_terms[g] += nsets * bpd * (hi - lo)
            for nb in range(NB):
                blk_s, blk_q = s[:, nb * bpd:(nb + 1) * bpd, lo:hi], q[:, nb * bpd:(nb + 1) * bpd, lo:hi]
                S1[nb, g] += blk_s.sum()
                A1[nb, g] += blk_s.abs().sum()
                S2[nb, g] += blk_q.sum()
        c0 += C
    return S1, A1, S2, int(per_group_terms.max())


def check_mean_rstd(got, S1, A1, S2, n, count, eps, label, where):
    """got [..., 2] fp32 (mean, rstd)"""
    mean, rstd, dm, dr = stats_bound(S1, A1, S2, n, count, eps)
    got = got.detach().cpu().to(f64)
    name = label.split("[")[0]
    WORST.note(name + ":mean", (got[..., 0] - mean).abs(), dm)
    WORST.note(name + ":rstd", (got[..., 1] - rstd).abs(), dr)
    _assert((got[..., 0] - mean).abs(), dm, f"{label}: mean", where)
    _assert((got[..., 1] - rstd).abs(), dr, f"{label}: rstd", where)


def check_finalize(out, partials, row_len, eps, label="rowstat_finalize"):
    """out [M, 2] against float64 of the partials [M, slots, 2] handed in"""
    p = partials.detach().cpu().to(f64)
    M, slots, _ = p.shape
    check_mean_rstd(out, p[..., 0].sum(1), p[..., 0].abs().sum(1), p[..., 1].sum(1), slots, float(row_len), eps, label, lambda i: f"(row {i})")


def parse_stats_line(line):
    """the "## stats k=v ..." line `hostcheck optrace` prints behind a launch with the sink armed -> plan dict"""
    assert line.startswith("## stats "), line
    return {k: int(v) for k, v in (t.split("=") for t in line.split()[2:])}


def plan_of_info(info):
    """ops.op_statistics.last() -> the same dict"""
    return {"colstat": info["colstat_written"], "rows": info["colstat_rows"], "span": info["colstat_span"], "sets": info["nsets"],
            "set_blocks": info["set_blocks"], "contiguous": info["colstat_contiguous"], "blocks_stored": info["colstat_blocks_stored"],
            "cs_floats": info["colstat_floats"], "rowstat": info["rowstat_written"], "cols": info["rowstat_cols"], "slots": info["rowstat_slots"],
            "rs_floats": info["rowstat_floats"], "M": info["M"], "N": info["N"], "splits": info["splits"]}
