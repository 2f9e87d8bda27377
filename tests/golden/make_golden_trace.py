"""Generates tests/golden/gemm_plan_trace.txt.gz: the launch trace of the host-only sanitizer build (lavie_amd/csrc/hostcheck,
`hostcheck trace FILE`), one line per kernel launch (kernel, grid, block, dynamic LDS bytes) under a "== case" line per case of
driver.cpp's run_traces(), one "workspace BYTES" line after every lavie_unet_prepare and one "copy BYTES" line per asynchronous
device-to-device copy (the shared prefix's duplications, finalize's packing copies).  The cases:
* the base model at the production shape (B = 2, F = 16, 40 x 64, cached 77-token context, shared prefix) under every force_tile
  mode, forced split-K 2 and 3 and fused mask 0x30;
* the routes of a forward, on a second base model at that shape: F = 8 (no fused temporal block); fused masks 0, 0x136, 0x135,
  0x133, 0x127, 0x117 and 0x037 (nothing fused; the default with each of bits 0, 1, 2, 4, 5, 8 off in turn), each with
  {uncached, cached context} x {shared prefix off, on}; lavie_unet_set_ln_fold(0); a cached 154-token context (the long fused
  text cross-attention);
* the interpolation model (F = 61; feed-forward before temporal) under the default mask, 0x136 and 0x133, and the VSR UNet (F = 8 at
  320 x 512);
* the reduced variants of `make asan`; on the reduced base model also perturbed-attention guidance (B = 3, one perturbed entry, a
  level-0 and the mid-block transformer) and FreeU, each followed by the plain forward again, and the two block entry points
  (lavie_unet_resnet_forward on a resnet with a skip input and a shortcut, lavie_unet_transformer_forward);
* lavie_linear_f16 / lavie_conv3x3_f16 / lavie_upsample_conv3x3_f16 at level shapes under every force_tile mode.

It pins every kernel choice, grid (split-K factor = grid.y of the GEMM launches) and tile of the implicit-GEMM planner, which
launches a forward sequences under each of its switches, and the workspace prepare() plans for them: tests/test_gemm_plan_trace.py
regenerates the trace and compares.  A change that means to pick another kernel regenerates this file, so that the change shows in
its diff.  CPU only, needs hipcc.  Run from the repo root:  python tests/golden/make_golden_trace.py"""
import gzip
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "lavie_amd", "csrc")
FIXTURE = os.path.join(HERE, "gemm_plan_trace.txt.gz")


def trace_lines():
    """Builds the host-only driver and returns the lines of a fresh trace."""
    r = subprocess.run(["make", "-C", CSRC, "-j", "8", "build_asan/hostcheck"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("building the host-only driver failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "trace.txt")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([os.path.join(CSRC, "build_asan", "hostcheck"), "trace", out], cwd=CSRC, capture_output=True, text=True,
                           env=env, timeout=900)
        if r.returncode != 0 or "trace written" not in r.stdout:
            raise RuntimeError("hostcheck trace failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])
        with open(out) as f:
            return f.read().splitlines()


def fixture_lines():
    with gzip.open(FIXTURE, "rt") as f:
        return f.read().splitlines()


def main():
    lines = trace_lines()
    with open(FIXTURE, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
        g.write(("\n".join(lines) + "\n").encode())
    print(f"{FIXTURE}: {len(lines)} lines, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
