"""The implicit-GEMM planner pinned by its launch trace (tests/golden/make_golden_trace.py): the host-only sanitizer build runs
the engine and the operator entry points at production shapes under every force_tile mode and every route of a forward (fused
mask bits, context cache, shared prefix, LayerNorm fold, context length) and records every kernel launch (kernel, grid, block,
dynamic LDS) and the workspace each prepare planned.  A refactor of the planner or of the forward's sequencing must leave the
trace as it is; a change of a kernel choice regenerates the fixture.  CPU only."""
import itertools
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import make_golden_trace  # noqa: E402


def first_difference(want, got):
    """(case, launch index inside the case, wanted line, produced line) of the first differing line, or None.  A "workspace N"
    line (the planned workspace after a prepare) is compared like any other line and is not counted as a launch."""
    case, idx = "(before the first case)", 0
    for w, g in itertools.zip_longest(want, got):
        if w != g:
            return case, idx, w, g
        if w.startswith("== "):
            case, idx = w[3:], 0
        elif not w.startswith("workspace "):
            idx += 1
    return None


def test_launch_trace_matches_fixture():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    want = make_golden_trace.fixture_lines()
    got = make_golden_trace.trace_lines()
    diff = first_difference(want, got)
    assert diff is None, ("launch trace differs in case '%s' at launch %d:\n  fixture: %s\n  now:     %s\n"
                          "(a deliberate change of the kernel choice regenerates tests/golden/gemm_plan_trace.txt.gz)" % diff)
    assert any(line.startswith("igemm_patch_kernel") for line in got) and any(line.startswith("igemm_ppx_kernel") for line in got)


def test_first_difference_names_the_launch():
    want = ["== a", "k1 1,1,1 64,1,1 0", "== b", "k1 1,1,1 64,1,1 0", "k2 2,1,1 64,1,1 0"]
    assert first_difference(want, list(want)) is None
    got = want[:4] + ["k2 2,2,1 64,1,1 0"]
    assert first_difference(want, got) == ("b", 1, want[4], got[4])
    assert first_difference(want, want[:3]) == ("b", 0, want[3], None)
    want.insert(3, "workspace 4096")
    assert first_difference(want, want[:5] + ["k2 2,2,1 64,1,1 0"]) == ("b", 1, want[5], "k2 2,2,1 64,1,1 0")
    assert first_difference(want, want[:3] + ["workspace 8192"] + want[4:]) == ("b", 0, want[3], "workspace 8192")
