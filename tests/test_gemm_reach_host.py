"""Which implicit-GEMM kernels the per-element operator cases reach (tests/opcases.py), computed by the library's own planner: the
host-only build (lavie_amd/csrc/hostcheck) replays the C-ABI calls of every GEMM-family case under every variant it runs under and
records each launch.  Every igemm_* / split-K kernel a forward launches (the names of tests/golden/gemm_plan_trace.txt.gz) must be
among them; what is not reached is written down by name, with its reason.  CPU only, needs hipcc."""
import gzip
import os
import shutil

import pytest

import opcases as C
import statcheck as S

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_trace.txt.gz")
GEMM = ("igemm_", "splitk_reduce")


@pytest.fixture(scope="module")
def cases():
    return C.gemm_family_cases()


@pytest.fixture(scope="module")
def reach(cases):
    return C.gemm_reach(cases)


@pytest.fixture(scope="module")
def fixture_names():
    with gzip.open(FIXTURE, "rt") as f:
        return {C.launch_name(l) for l in f.read().splitlines() if not l.startswith(("== ", "workspace ", "!! ", "copy "))}


def names(reach, keep=lambda key: True):
    return {C.launch_name(l) for key, launches in reach.items() if launches and keep(key) for l in launches}


def test_every_gemm_kernel_of_a_forward_is_reached_by_a_case(reach, fixture_names):
    required = {n for n in fixture_names if n.startswith(GEMM)}
    assert len(required) >= 20
    allowed = set(C.TOO_LARGE) | {n for n in C.NO_OPERATOR_ENTRY if n.startswith(GEMM)}
    missing = required - names(reach) - allowed
    assert missing == set(), "no per-element case reaches: " + "; ".join(sorted(missing))
    assert allowed <= required and not (allowed & names(reach)), "an exception that is reached, or that no forward launches, is none"


def test_no_replayed_call_is_refused(reach):
    refused = sorted(key for key, launches in reach.items() if launches is None)
    assert refused == [], refused                       # (no GEMM-family case is a declared refusal)
    assert all(launches for launches in reach.values())


def test_registered_instantiations_are_reached_or_listed(reach):
    registered = {n for n in C.registered_kernels() if n.startswith("igemm_")}
    assert len(registered) >= 26
    reached = names(reach)
    listed = set(C.NOT_PLANNED) | set(C.TOO_LARGE)
    assert registered - reached - listed == set(), sorted(registered - reached - listed)
    assert listed & reached == set(), "listed as unreached, but reached: %s" % sorted(listed & reached)
    assert listed <= registered, "listed, but no longer registered: %s" % sorted(listed - registered)
    assert all(len(reason) > 20 for reason in list(C.NOT_PLANNED.values()) + list(C.TOO_LARGE.values()))


def test_fixture_names_are_all_accounted_for(reach, fixture_names):
    required = {n for n in fixture_names if n.startswith(GEMM)}
    elsewhere = {n for n in fixture_names if n.startswith(C.COVERED_ELSEWHERE + C.LOCAL_KERNELS)}
    ends = (set(C.ENDS_KERNELS) | set(C.PACK_STEP_KERNELS)) & fixture_names
    assert ends - names(reach) - set(C.PACK_STEP_KERNELS) == set(), "an end or glue kernel of a forward that no case launches"
    attention = {n for n in fixture_names if n.startswith(C.ATTENTION_KERNELS)}
    missing = attention - names(reach) - set(C.ATTENTION_NO_CASE)
    assert len(attention) >= 15 and missing == set(), "an attention kernel of a forward that no case launches: %s" % sorted(missing)
    assert set(C.ATTENTION_NO_CASE) <= attention and not (set(C.ATTENTION_NO_CASE) & names(reach)), "an exception that is reached, or that no forward launches, is none"
    accounted = required | elsewhere | attention | set(C.NO_OPERATOR_ENTRY) | ends
    assert accounted == fixture_names, sorted(fixture_names - accounted)
    assert set(C.NO_OPERATOR_ENTRY) <= fixture_names and not (set(C.NO_OPERATOR_ENTRY) & elsewhere)
    assert not (set(C.NO_OPERATOR_ENTRY) & names(reach)), "a kernel listed as having no operator entry point was launched by one"
    for name, test in C.NO_OPERATOR_ENTRY.items():
        path = test.split("::")[0].split(" ")[0]
        assert os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)), (name, path)


def test_local_kernels_of_a_forward_are_reached(reach, fixture_names):
    """Every GroupNorm, row-resident and temporal kernel a forward's trace names — each gn_stats_kernel<V> / gn_apply_kernel<V, SILU>
    and gn_finalize_kernel among them — is launched by a case; gn_finalize_kernel by every group_norm case, which is why it is no
    longer listed as having no operator entry point."""
    required = {n for n in fixture_names if n.startswith(C.LOCAL_KERNELS)}
    assert {"gn_finalize_kernel", "gn_stats_kernel<1>", "gn_stats_kernel<2>", "gn_apply_kernel<1, true>", "gn_apply_kernel<1, false>",
            "gn_apply_kernel<2, true>", "temporal_block_kernel<8>", "temporal_stream_kernel<1, 320, 2>", "temporal_stream_kernel<4, 160, 1>"} <= required
    assert required - names(reach) == set(), sorted(required - names(reach))
    assert "gn_finalize_kernel" not in C.NO_OPERATOR_ENTRY
    # the producer-side statistics kernels: a forward's trace names all three, the statistics cases launch all three
    stats = {"gn_fold_kernel", "rowstat_finalize_kernel", "splitk_reduce_cs_kernel"}
    assert stats <= fixture_names and stats <= names(reach) and not (stats & set(C.NO_OPERATOR_ENTRY))
    assert stats <= names(reach, lambda key: key[0].startswith(("gn_fold[", "rowstat_finalize[")) or "+cs" in key[0])
    gn = [c for c in C.all_cases() if c.name.startswith("group_norm[")]
    assert len(gn) == len(C.GN_CASES) + len(C.GN_PAST_SLAB) + len(C.GN_VAE)
    vae = [c for c in gn if c.gn[2] == 128]
    assert [reach[(c.name, "auto")][2].rsplit(" ", 3)[0] for c in vae] == ["gn_apply_kernel<1, true>", "gn_apply_kernel<1, false>"]
    assert all(C.launch_grid(reach[(c.name, "auto")][0]) == (3, 2, 1) for c in vae)          # the autoencoder's width: three slabs, two batch entries
    for c in gn:                                  # statistics, finalize, then apply or the (a, b) pairs; grids as the Python mirror of gn_slabs says
        lines = reach[(c.name, "auto")]
        nb, P, ctot = c.gn
        tx, vpt, ty = C.gn_geometry(ctot)
        slabs = C.gn_slabs(P, nb, ty)[0]
        assert [C.launch_name(l) for l in lines][:2] == [f"gn_stats_kernel<{vpt}>", "gn_finalize_kernel"], (c.name, lines)
        assert C.launch_grid(lines[0]) == (slabs, nb, 1) and C.launch_grid(lines[1]) == (-(-nb * 32 // 4), 1, 1), (c.name, lines)
        if c.calls[0][0] == "group_norm_affine":
            assert C.launch_name(lines[2]) == "gn_affine_kernel"
        else:
            silu = "true" if c.calls[0][1]["silu"] else "false"
            assert C.launch_name(lines[2]) == f"gn_apply_kernel<{vpt}, {silu}>" and C.launch_grid(lines[2]) == (slabs, nb, 1), (c.name, lines)


EDGE_OUT_KERNELS = {f"conv_edge_out_kernel<{ncb}, {t}>" for ncb in (0, 4, 8, 16) for t in ("float", "half")}
EDGE_IN_KERNELS = {"conv_edge_in_kernel<float>", "conv_edge_in_kernel<half>"}


def test_autoencoder_kernels_launch_what_the_walk_mirrors_say(reach):
    """Kernel name and grid of every edge-conv and wide-attention case from the replay, against opcases.edge_out_walk / edge_in_walk /
    wide_walk; every conv_edge_out and conv_edge_in instantiation is launched by some case; the grids of the issue's largest cases."""
    cases = C.all_cases()
    new = {c.name for c in C.vae_cases()}
    out = [c for c in cases if c.name.startswith("conv_edge_out[")]
    assert len(out) == 2 * len(C.EDGE_OUT) + len(C.EDGE_OUT_PAST) and {c.name for c in out if c.name in new} == {C.edge_out_case(*e).name for e in C.EDGE_OUT_PAST}
    for c in out:
        (line,) = reach[(c.name, "auto")]
        a = c.calls[0][1]
        ncb = {128: 4, 256: 8, 512: 16}.get(a["Cin"], 0)
        grid, per = C.edge_out_walk(c.edge[0])
        assert C.launch_name(line) == f"conv_edge_out_kernel<{ncb}, {'float' if a['y_dtype'] else 'half'}>", (c.name, line)
        assert C.launch_grid(line) == (grid, 1, 1) and line.rsplit(" ", 2)[1] == "256,1,1", (c.name, line)
        assert (per >= 2) == (c.edge[0] > 2048 * 64), c.name
    assert {C.launch_name(reach[(c.name, "auto")][0]) for c in out} == EDGE_OUT_KERNELS
    assert {C.launch_name(reach[(c.name, "auto")][0]) for c in out if c.name in new} >= {k for k in EDGE_OUT_KERNELS if "<0," in k}     # the rolled loop: new cases alone
    (line,) = reach[("conv_edge_out[1x128->3,257x513,float32]", "auto")]
    assert (C.launch_name(line), C.launch_grid(line)) == ("conv_edge_out_kernel<4, float>", (1031, 1, 1))
    (line,) = reach[("conv_edge_out[1x8->8,257x513,float16]", "auto")]
    assert (C.launch_name(line), C.launch_grid(line)) == ("conv_edge_out_kernel<0, half>", (1031, 1, 1))

    inn = [c for c in cases if c.name.startswith("conv_edge_in[")]
    assert len(inn) == 4 * len(C.EDGE_IN) + len(C.EDGE_IN_PAST)
    for c in inn:
        (line,) = reach[(c.name, "auto")]
        grid, steps = C.edge_in_walk(*c.edge)
        assert C.launch_name(line) == f"conv_edge_in_kernel<{'float' if c.calls[0][1]['x_dtype'] else 'half'}>" and C.launch_grid(line) == (grid, 1, 1), (c.name, line)
        assert (max(steps) >= 2) == (c.name in new), c.name                      # a second grid-stride step: the new cases, and only they
    assert {C.launch_name(reach[(c.name, "auto")][0]) for c in inn} == EDGE_IN_KERNELS
    assert {(C.launch_name(reach[(c.name, "auto")][0]), C.launch_grid(reach[(c.name, "auto")][0])) for c in inn if c.name in new} == {(k, (4096, 1, 1)) for k in EDGE_IN_KERNELS}

    wide = [c for c in cases if getattr(c, "route", None) == "wide"]
    assert len(wide) == len(C.WIDE_ATTN) + len(C.WIDE_HARD_CASES) + len(C.WIDE_PAST_CASES)
    for c in wide:
        (line,) = reach[(c.name, "auto")]
        walk, _ = C.wide_case_walk(c)
        assert C.launch_name(line) == f"attention_wide_kernel<{c.calls[0][1]['dh']}>" and C.launch_grid(line) == (len(walk), 1, 1), (c.name, line)
        assert (len(walk) > 1) == (c.name in new), c.name                        # what the suite had: one workgroup
    (line,) = reach[("attention[nb3,lq129,lkNone,c1024,h2,div1]", "auto")]
    assert (C.launch_name(line), C.launch_grid(line)) == ("attention_wide_kernel<512>", (12, 1, 1))
    assert {C.launch_name(reach[(c.name, "auto")][0]) for c in wide if c.name in new} == {"attention_wide_kernel<512>", "attention_wide_kernel<256>"}


def test_capped_block_cases_launch_with_their_cap(reach):
    """Each multi-pass case launches its kernel on exactly lavie_debug_rowfuse_grid workgroups, the natural-grid case on 256, and the
    older block cases on one workgroup per tile, as the share-rule mirror assumes."""
    kernels = {"geglu_mlp": "geglu_mlp_kernel<320, 8>", "temporal_block": "temporal_block_kernel<8>", "cross_block": "cross_block_kernel<8>",
               "cross_block_long": "cross_block_kernel<40>", "proj_qkv": "proj_qkv_kernel<8>"}
    multi = C.multi_pass_cases()                  # (the in-place twins make the same call)
    assert all(a.calls == b.calls and a.knobs == b.knobs for a, b in zip(multi, C.multi_pass_cases(in_place=True)))
    assert {c.calls[0][0] for c in multi} == set(kernels) and [c.name for c in multi if not c.cap] == [C.NATURAL_GRID + "[inplace0]"]
    for c in multi:
        (line,) = reach[(c.name, "auto")]
        fam, walk, _ = C.case_walk(c)
        assert C.launch_name(line) == kernels[fam] and C.launch_grid(line) == (c.cap or 256, 1, 1), (c.name, line)
        assert 1 + max(w for w, _, _ in walk) == C.launch_grid(line)[0]
        assert c.knobs == ({"rowfuse_grid": c.cap} if c.cap else {})
    older = [c for c in C.all_cases() if c.calls and c.calls[0][0] in kernels and c not in multi]
    assert len(older) >= 14
    for c in older:
        (line,) = reach[(c.name, "auto")]
        _, walk, _ = C.case_walk(c)
        assert C.launch_grid(line)[0] == len(walk) and max(p for _, p, _ in walk) == 0, (c.name, line)      # one tile per workgroup: what the suite had


def test_temporal_cases_launch_what_the_route_function_says(reach):
    """opcases.temporal_route against the launcher itself: kernel name and grid of every temporal attention case, and TATTN_ROUTES
    against the temporal kernels the library registers."""
    registered = {n for n in C.registered_kernels() if n.startswith(("temporal_stream_kernel<", "temporal_attention_kernel<"))}
    assert registered == set(C.TATTN_ROUTES), sorted(registered ^ set(C.TATTN_ROUTES))
    cases = C.temporal_attention_cases()
    for c in cases:
        (line,) = reach[(c.name, "auto")]
        assert (C.launch_name(line), C.launch_grid(line)) == (c.troute["kernel"], c.troute["grid"]), (c.name, line, c.troute)
        if "lds" in c.troute:
            assert int(line.rsplit(" ", 1)[1]) == c.troute["lds"], (c.name, line)
    assert {C.launch_name(reach[(c.name, "auto")][0]) for c in cases} == set(C.TATTN_ROUTES)


def test_end_and_glue_kernels_are_reached(reach, fixture_names):
    """Every kernel of opcases.ENDS_KERNELS is launched by a case of ends_cases(), each conv_out case by the kernel its shape table
    names (<5> / <6> / general), and every one but the general conv_out kernel (no model has Cout != 4 or Cin > 336) runs in a forward."""
    by_family = C.ends_cases()
    got = {k: {C.launch_name(l) for c in cs for l in reach[(c.name, "auto")]} for k, cs in by_family.items()}
    assert set().union(*got.values()) == set(C.ENDS_KERNELS), sorted(set().union(*got.values()) ^ set(C.ENDS_KERNELS))
    assert set(C.ENDS_KERNELS) - fixture_names == {"conv_out_kernel"}
    assert got["conv_out"] == {"pack_conv3x3_kernel", "conv_out4_kernel<5>", "conv_out4_kernel<6>", "conv_out_kernel"}
    assert got["gemv"] == {"gemv_kernel"} and got["ln_fold"] == {"ln_fold_kernel"} and got["conv_in"] == {"pack_conv_in_kernel", "conv_in_kernel"}
    for c in by_family["conv_out"]:
        assert [C.launch_name(l) for l in reach[(c.name, "auto")]] == ["pack_conv3x3_kernel", c.kernel], c.name
    routes = {(ci, co): C.conv_out_route(ci, co) for ci, co in C.CONV_OUT_SHAPES}
    assert routes == {(256, 4): "conv_out4_kernel<5>", (64, 4): "conv_out4_kernel<5>", (320, 4): "conv_out4_kernel<6>", (336, 4): "conv_out4_kernel<6>",
                      (344, 4): "conv_out_kernel", (64, 8): "conv_out_kernel", (64, 3): "conv_out_kernel"}
    # without a family, its kernels are missed
    for fam, kernel in (("gemv", "gemv_kernel"), ("timestep_sinusoid", "timestep_sinusoid_kernel"), ("ln_fold", "ln_fold_kernel"),
                        ("add_class_emb_silu", "add_class_emb_silu_kernel"), ("fill_relpos_bias", "fill_relpos_bias_kernel"), ("conv_in", "conv_in_kernel")):
        assert kernel not in set().union(*(v for k, v in got.items() if k != fam)), (fam, kernel)
    for ci, co in C.CONV_OUT_SHAPES:          # ... and without a conv_out shape pair, where it is the only one of its kernel and slot count
        rest = {C.conv_out_route(a, b) for a, b in C.CONV_OUT_SHAPES if (a, b) != (ci, co)}
        assert rest == {"conv_out4_kernel<5>", "conv_out4_kernel<6>", "conv_out_kernel"}      # two shapes per kernel: one at each end of its range


def test_refusals_of_the_end_and_glue_entries():
    """every refusal the GPU tests expect, from the library itself on the host-only build"""
    lines = [f"conv_out B=1 Cin={ci} F=1 H=1 W=2 Cout={co}" for ci, co in C.CONV_OUT_REFUSED]
    lines += [f"conv_in B=1 Cin={ci} F=1 H=1 W=2 Cout={co}" for ci, co in C.CONV_IN_REFUSED]
    lines += [f"gemv B={b} N={n} K={k} act_in=0 act_out=0 bias=1" for b, n, k in C.GEMV_REFUSED]
    lines += [f"copy_rows ld_src={ls} ld_dst={ld} rows={r} cols={c} col0={c0}" for r, c, ls, ld, c0 in C.COPY_ROWS_REFUSED]
    lines += ["pack_geglu_vec N=48", "add_class_emb_silu B=2 N=8 num_classes=5 label=5", "add_class_emb_silu B=2 N=8 num_classes=5 label=-1",
              "add_class_emb_silu B=9 N=8 num_classes=5"]
    for line, launches in C.optrace(lines):
        assert launches == ["!! refused"], (line, launches)


def test_gather_kernels_belong_to_the_block_cases_pack_steps():
    """rf_gather8 / rf_gather_f16_f32 / xb_gather2 / xb_gather8 are launched by lavie_pack_geglu_mlp_f16 and lavie_bind_cross_block[_long]_f16
    (behind their pack), which geglu_mlp_case and cross_block_case call: they have an operator entry point."""
    blocks = dict(C.optrace(["pack_geglu_mlp C=320", "bind_cross_block B=2 ctx_len=77 C=320", "bind_cross_block_long B=1 ctx_len=154 C=320"]))
    got = {k: {C.launch_name(l) for l in v} for k, v in blocks.items()}
    assert got["pack_geglu_mlp C=320"] == {"rf_gather8_kernel", "rf_gather_f16_f32_kernel"}
    assert got["bind_cross_block B=2 ctx_len=77 C=320"] == got["bind_cross_block_long B=1 ctx_len=154 C=320"] == {"rf_gather8_kernel", "xb_gather2_kernel", "xb_gather8_kernel"}
    assert set().union(*got.values()) == set(C.PACK_STEP_KERNELS) and not (set(C.PACK_STEP_KERNELS) & set(C.NO_OPERATOR_ENTRY))


# what each table entry of opcases.py claims, from the trace: (case name, variant) -> kernel
TABLE = [
    ("lnfold[160x320x320]", "ppx-persistent", "igemm_ppx_kernel<0, 5, 2>"), ("lnfold[320x320x320]", "ppx-persistent", "igemm_ppx_kernel<0, 5, 2>"),
    ("lnfold[160x256x320]", "ppx-persistent", "igemm_ppx_kernel<0, 4, 2>"), ("lnfold[320x256x320]", "ppx-persistent", "igemm_ppx_kernel<0, 4, 2>"),
    ("geglu[160x320]", "ppx-persistent", "igemm_ppx_kernel<1, 4, 0>"), ("lnfold_geglu[160x320]", "ppx-persistent", "igemm_ppx_kernel<1, 4, 2>"),
    ("lnfold_geglu[129x64]", "auto", "igemm_kernel<2, 2, 4, 4, 2, false, 1>"), ("lnfold_geglu[154x320]", "auto", "igemm_kernel<2, 2, 4, 4, 2, false, 1>"),
    ("lnfold_geglu[154x320]", "pingpong", "igemm_pp_kernel<false, 1, 4>"), ("geglu[2233x512]", "auto", "igemm_pp_kernel<false, 1, 4>"),
    ("lnfold_geglu[2233x512]", "auto", "igemm_pp_kernel<false, 1, 4>"), ("linear[34721x256x640,plain]", "auto", "igemm_pp_kernel<false, 0, 4>"),
    ("linear[2689x512x192,bias_residual]", "split-k-3", "igemm_kernel<2, 2, 4, 4, 2, false, 0>"),
    ("linear[2689x512x192,bias_residual]", "split-k-3", "splitk_reduce_kernel"),
    ("temporal_conv[1x128->256,f8,d4341,t5]", "auto", "igemm_pp_kernel<true, 0, 4>"),
]
CONV_TABLE = [
    (dict(n=1, c1=64, cout=512, h=52, w=52), "split-k-3", "igemm_kernel<2, 2, 4, 4, 2, true, 0>"),
    (dict(n=1, c1=64, cout=320, h=5, w=7), "pingpong", "igemm_pp_kernel<true, 0, 5>"),
    (dict(n=1, c1=64, cout=128, h=40, w=8, extras=True, force=5), "forced", "igemm_patch_kernel<0, 4, 0>"),
    (dict(n=1, c1=64, cout=160, h=10, w=96, extras=True, force=5), "forced", "igemm_patch_kernel<0, 5, 1>"),
    (dict(n=1, c1=128, cout=256, h=20, w=128, extras=True, force=5), "forced", "igemm_patch_kernel<0, 4, 1>"),
]


def test_reach_table_entries(reach):
    for case, variant, kernel in TABLE:
        assert kernel in {C.launch_name(l) for l in reach[(case, variant)]}, (case, variant, reach[(case, variant)])
    for kw, variant, kernel in CONV_TABLE:
        name = C.conv_case(**kw).name
        assert kernel in {C.launch_name(l) for l in reach[(name, variant)]}, (name, variant, reach[(name, variant)])
    for taps in (3, 5):
        name = C.temporal_conv_case(*C.TCONV_FORCED[0], taps, force=5).name
        assert [C.launch_name(l) for l in reach[(name, "forced")]] == ["igemm_patch_kernel<0, 4, 2>"]
    for n, c, h, w in C.PARITY_CASES:
        name = C.conv_case(n=n, c1=c, cout=c, h=h, w=w, ups=1, parity=True).name
        assert all(C.launch_name(reach[(name, v)][0]) == "igemm_patch_kernel<0, 5, 3>" for v in C.VARIANTS)
        assert all(len(reach[(name, v)]) == 1 and C.launch_grid(reach[(name, v)][0]) == (n * h * w // 320 * (c // 160), 1, 4) for v in C.VARIANTS)    # unsplit
    assert [s for *_, s in C.PARITY_SPLIT_CASES] == [4, 2]
    for n, c, h, w, splits in C.PARITY_SPLIT_CASES:        # the planner's own factor (force_splits does not apply), then the reduce
        case = C.parity_case(n, c, h, w)
        assert case.variants == ("auto",)
        lines = reach[(case.name, "auto")]
        assert [C.launch_name(l) for l in lines] == ["igemm_patch_kernel<0, 5, 3>", "splitk_reduce_kernel"], (case.name, lines)
        assert C.launch_grid(lines[0]) == (n * h * w // 320 * (c // 160), splits, 4), (case.name, lines)
        assert c // 64 >= 5 * splits                        # nchunks: whole slabs per split, as many as the unsplit cases have in all
        armed = reach[(case.name + "+cs", "auto")]           # with the sink armed: the same launch, the reduce with statistics behind it
        assert [C.launch_name(l) for l in armed] == ["igemm_patch_kernel<0, 5, 3>", "splitk_reduce_cs_kernel"] and C.launch_grid(armed[0]) == C.launch_grid(lines[0])
        (note,) = C.NOTES[(case.name + "+cs", "auto")]
        plan = S.parse_stats_line(note)
        assert (plan["splits"], plan["rows"], plan["span"], plan["sets"], plan["set_blocks"], plan["contiguous"]) == (splits, 32, 32, 1, 4 * n * h * w // 32, 1), plan


def test_deep_k_linear_cases_split_by_the_cost_rule(reach):
    """80 K-tiles: `auto` launches the 128-row kernel with the factor the planner's cost rule yields — more than the 3 any forced variant
    reaches — over ranges of unequal length where nk % s != 0, the reduce behind it; the three forced cases run one unsplit 80-tile K
    loop on the 128-row, the ping-pong and the persistent kernel; the GEGLU case runs 20 K-tiles on each GEGLU kernel."""
    factors = {}
    for name in C.DEEP_AUTO:
        lines = reach[(name, "auto")]
        assert [C.launch_name(l).split("<")[0] for l in lines] == ["igemm_kernel", "splitk_reduce_kernel"], (name, lines)
        factors[name] = C.launch_grid(lines[0])[1]
        assert factors[name] > 3, (name, lines)
    assert 80 % factors[C.DEEP_AUTO[0]] != 0               # t_begin / t_end over ranges of unequal length
    assert len(set(factors.values())) == 2, factors        # two different numbers of slabs under the fixed-order sum
    assert factors == {C.DEEP_AUTO[0]: 6, C.DEEP_AUTO[1]: 5}, factors           # (what the trace shows today: 13 / 14 K-tiles and 16 a range)
    wide = "linear[160x320x5120,bias_residual]"
    pp = reach[(wide, "pingpong")]                          # the ping-pong kernel under the same automatic factor
    assert C.launch_name(pp[0]) == "igemm_pp_kernel<false, 0, 5>" and C.launch_grid(pp[0])[1] > 3 and C.launch_name(pp[1]) == "splitk_reduce_kernel"
    unsplit = {f: reach[(C.linear_case(160, 320, 5120, "bias_residual", force=f).name, "forced")] for f in C.DEEP_UNSPLIT}
    assert all(len(l) == 1 and C.launch_grid(l[0])[1] == 1 for l in unsplit.values()), unsplit
    assert [C.launch_name(l[0]) for l in unsplit.values()] == ["igemm_kernel<2, 2, 4, 5, 2, false, 0>", "igemm_pp_kernel<false, 0, 5>", "igemm_ppx_kernel<0, 5, 1>"]
    geglu = {v: [C.launch_name(l) for l in reach[("geglu[160x1280]", v)]] for v in C.VARIANTS}
    assert {k[0] for k in geglu.values()} == {"igemm_kernel<2, 2, 4, 4, 2, false, 1>", "igemm_pp_kernel<false, 1, 4>", "igemm_ppx_kernel<1, 4, 0>"} and all(len(k) == 1 for k in geglu.values())


def test_forced_splits_begin_inside_segments(reach):
    """Where each split-K range of the 192 + 128 cases begins, from nk, the segment table of the call and the factor (the kernels'
    cursor arithmetic, opcases.kloop_position), and the factor itself from the grid of the trace."""
    sc = C.conv_case(**C.SEG_SC)
    segs = C.kloop_segments(sc.calls[0][1])
    assert segs == [(3, 9), (2, 9), (3, 1), (2, 1)]
    nk = sum(a * b for a, b in segs)
    assert nk == 50 and C.kloop_segments(C.conv_case(**C.SEG).calls[0][1]) == [(3, 9), (2, 9)]
    begins = set()
    for tile, s in C.SEG_FORCED:
        case = C.conv_case(**C.SEG_SC, force=tile, splits=s)
        lines = reach[(case.name, "forced")]
        kernel = {1: "igemm_kernel<2, 2, 4, 5, 2, true, 0>", 3: "igemm_pp_kernel<true, 0, 5>"}[tile]
        assert C.launch_name(lines[0]) == kernel and C.launch_grid(lines[0])[1] == s, (case.name, lines)
        assert [C.launch_name(l) for l in lines[1:]] == (["splitk_reduce_kernel"] if s > 1 else []), (case.name, lines)
        assert case.calls == sc.calls
        begins |= {(tile, C.kloop_position(segs, t)) for t in C.split_begins(nk, s)[1:]}
    for tile in (1, 3):
        at = [p for t, p in begins if t == tile]
        assert any(seg == 0 and slab >= 1 and tap > 0 for seg, slab, tap in at), at          # inside segment 0, past its first slab, not at a slab's first tap
        assert any(seg == 1 and (slab, tap) != (0, 0) for seg, slab, tap in at), at           # inside segment 1
        assert any(seg == 1 and slab >= 1 and tap > 0 for seg, slab, tap in at), at           # ... and inside its second slab
        assert (2, 0, 0) in at and any(seg == 2 and slab > 0 for seg, slab, tap in at) and any(seg == 3 for seg, slab, tap in at), at    # at and inside the shortcuts
    assert [C.kloop_position(segs, t) for t in C.split_begins(nk, 3)] == [(0, 0, 0), (0, 1, 7), (1, 0, 6)]
    assert [C.kloop_position(segs, t) for t in C.split_begins(nk, 10)][6:] == [(1, 0, 3), (1, 0, 8), (1, 1, 4), (2, 0, 0)]
    # the same operands under the six variants: whatever factor the variant yields, the launch is the gather kernel it names
    for v, (tile, s) in C.VARIANTS.items():
        lines = reach[(sc.name, v)]
        assert C.launch_name(lines[0]) in ("igemm_kernel<2, 2, 4, 5, 2, true, 0>", "igemm_kernel<2, 2, 4, 2, 2, true, 0>", "igemm_pp_kernel<true, 0, 5>"), (v, lines)
        assert not s or C.launch_grid(lines[0])[1] == s
    # the halo-patch kernel splits over whole slabs (igemm_patch.hip:90-91): 5 slabs of 9 taps
    assert [[5 * i // s for i in range(s + 1)] for s in C.HALO_SEG_SPLITS] == [[0, 5], [0, 2, 5], [0, 1, 3, 5], [0, 1, 2, 3, 4, 5]]
    for kw, kernel in zip(C.HALO_SEG_CASES, ("igemm_patch_kernel<0, 5, 0>", "igemm_patch_kernel<0, 5, 1>")):
        for s in C.HALO_SEG_SPLITS:
            case = C.conv_case(**kw, force=5, splits=s)
            hsegs = C.kloop_segments(case.calls[0][1])
            assert hsegs == [(3, 9), (2, 9)]
            lines = reach[(case.name, "forced")]
            assert C.launch_name(lines[0]) == kernel and C.launch_grid(lines[0])[1] == s and len(lines) == (2 if s > 1 else 1), (case.name, lines)
            starts = [C.kloop_position(hsegs, 9 * (5 * i // s)) for i in range(s)]
            assert all(tap == 0 for _, _, tap in starts)
            if s == 2:
                assert starts == [(0, 0, 0), (0, 2, 0)]      # the second range begins inside segment 0 and crosses into segment 1
            if s == 3:
                assert starts == [(0, 0, 0), (0, 1, 0), (1, 0, 0)] and 5 * 2 // 3 == 3     # [1, 3) crosses the boundary; [3, 5) is segment 1
            if s == 5:
                assert starts[4] == (1, 1, 0)                # a range that begins inside segment 1 (no factor below 5 has one)


def epi_linear(name):
    """whether an igemm_* instantiation has the EPI_LINEAR epilogue: the template argument that holds EPI (0 = linear)"""
    args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]
    return args[{"igemm_kernel": 6, "igemm_pp_kernel": 1, "igemm_ppx_kernel": 0, "igemm_patch_kernel": 0}[name[:name.index("<")]]] == "0"


def test_every_linear_instantiation_is_reached_with_column_statistics(reach):
    """Every EPI_LINEAR igemm_* instantiation some case reaches is also launched UNSPLIT with the statistics sink armed and the plan
    writing column statistics (split-K leaves them to the reduce kernel: the instantiation's own epilogue branch does not run), or is
    excused by name in opcases.NO_COLSTAT; the reduce kernel with statistics is reached behind a plain GEMM, a gathered one and the
    halo-patch kernel."""
    linear = {n for n in names(reach) if n.startswith("igemm_") and epi_linear(n)}
    assert len(linear) >= 19, sorted(linear)
    with_cs, reduce_behind = set(), set()
    for key, launches in reach.items():
        notes = [S.parse_stats_line(l) for l in C.NOTES.get(key, []) if l.startswith("## stats ")]
        if not notes or not notes[0]["colstat"]:
            continue
        ks = [C.launch_name(l) for l in launches if C.launch_name(l).startswith(("igemm_", "splitk_reduce"))]
        if notes[0]["splits"] == 1:
            assert len(ks) == 1, (key, ks)
            with_cs.add(ks[0])
        else:
            assert ks[1:] == ["splitk_reduce_cs_kernel"] and notes[0]["rows"] == 32 and notes[0]["contiguous"] == 1, (key, ks, notes)
            reduce_behind.add(ks[0])
    assert linear - with_cs - set(C.NO_COLSTAT) == set(), sorted(linear - with_cs - set(C.NO_COLSTAT))
    assert not (set(C.NO_COLSTAT) & with_cs) and set(C.NO_COLSTAT) <= linear and all(len(r) > 20 for r in C.NO_COLSTAT.values())
    assert {"igemm_kernel<2, 2, 4, 4, 2, false, 0>", "igemm_kernel<2, 2, 4, 4, 2, true, 0>", "igemm_patch_kernel<0, 4, 1>",
            "igemm_patch_kernel<0, 5, 3>"} <= reduce_behind
    # row statistics: each kernel family, each slot width the planner yields
    rs = {}
    for key, launches in reach.items():
        notes = [S.parse_stats_line(l) for l in C.NOTES.get(key, []) if l.startswith("## stats ")]
        if notes and notes[0]["rowstat"]:
            assert notes[0]["splits"] == 1 and len(launches) == 1, (key, launches)
            rs.setdefault(C.launch_name(launches[0]).split("<")[0], set()).add(notes[0]["cols"])
    assert rs == {"igemm_kernel": {32, 64, 80}, "igemm_pp_kernel": {64, 80}, "igemm_ppx_kernel": {64, 80}}, rs
    # the fold runs for every usable descriptor and for no other
    for c in C.stats_local_cases():
        if c.name.startswith("gn_fold["):
            assert C.NOTES[(c.name, "auto")] == ["## fold=%d" % c.usable], (c.name, C.NOTES[(c.name, "auto")])
            assert ("gn_fold_kernel" in {C.launch_name(l) for l in reach[(c.name, "auto")]}) == c.usable


def test_removing_a_new_case_is_noticed(cases):
    """the reach of the suite without the grid-rule linear case, and without the forced temporal convs, misses exactly their kernels"""
    for drop, kernel in (("linear[34721x256x640,plain]", "igemm_pp_kernel<false, 0, 4>"), ("temporal_conv[1x64->128,f8,d40", "igemm_patch_kernel<0, 4, 2>")):
        rest = [c for c in cases if not c.name.startswith(drop)]
        assert len(rest) < len(cases)
        assert kernel not in names(C.gemm_reach(rest)), (drop, kernel)


def test_persistent_kernel_runs_past_its_workgroup_cap(reach, cases):
    """Each past-the-cap case launches igemm_ppx_kernel with the full grid of 256 workgroups under `auto` and `ppx-persistent`, and
    its shape has the tile count its table entry states: >= 257 for a second tile in some workgroup, >= 513 for a workgroup with a
    first, a steady-state and a last tile."""
    by_name = {c.name: c for c in cases}
    assert set(C.PAST_CAP) <= set(by_name)
    for name, (bn, least) in C.PAST_CAP.items():
        ints = by_name[name].calls[0][1]
        tiles = (ints["M"] // 160) * (ints["N"] // bn)
        assert ints["M"] % 160 == 0 and ints["N"] % bn == 0 and tiles >= least, (name, tiles)
        assert by_name[name].variants == C.BIG
        for v in C.BIG:
            (launch,) = reach[(name, v)]
            assert C.launch_name(launch).startswith("igemm_ppx_kernel<") and C.launch_grid(launch) == (256, 1, 1), (name, v, launch)
    modes = {C.launch_name(reach[(name, "auto")][0]) for name in C.PAST_CAP}
    assert modes == {f"igemm_ppx_kernel<{e}>" for e in ("0, 5, 0", "0, 5, 1", "0, 5, 2", "0, 4, 0", "0, 4, 1", "0, 4, 2", "1, 4, 0", "1, 4, 2")}, sorted(modes)
