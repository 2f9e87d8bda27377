"""The operator cases of the per-element checks, shared by tests/test_opcheck_host.py (CPU: the fp32 model of each kernel must
meet its own bound) and tests/test_gpu_ops_local.py (the kernels).  A case holds its inputs (CPU tensors in the dtypes the
kernel takes), how to run the operator, a float64 reference with the per-element scale, the constant c of its family, and a
torch fp32 model of the kernel with fp16 roundings at the counted points.

Shapes are the smallest that cross each kernel's edges; none is a workload shape."""
import functools
import math
import os
import subprocess
import tempfile
import zlib

import torch
import torch.nn.functional as F

import opcheck as oc

f16, f32t, f64 = torch.float16, torch.float32, torch.float64


class Case:
    def __init__(self, name, inputs, outputs, run, ref, c, model, where, alias=None, regions=None, setup=None, u=oc.U16, partial=None,
                 exact=None, post=None):
        self.name, self.inputs, self.outputs, self.run, self.c, self.model, self.where = name, inputs, outputs, run, c, model, where
        self.alias = alias or {}
        self.u = u                            # the relative term's unit roundoff: U16, U32 for an fp32 output (or name -> u)
        self.partial = partial or {}          # name -> bool mask of the elements the call must write (opcheck.run_guarded)
        self.exact = exact or {}              # name -> the expected tensor of a pure move / exact conversion, compared bit for bit
        self.post = post                      # optional further assertion on the outputs (a property the bound does not express)
        self._ref = ref
        self.regions = regions or {}          # name -> bool mask over output "y": regions asserted on their own as well
        self.setup = setup                    # optional context manager factory (forced kernels)
        self.calls = None                     # GEMM family: the C-ABI calls `run` makes (call()), replayed on the host-only build
        self.force = None                     # (tile, splits) the case forces around its launch, whatever the variant
        self.variants = None                  # the VARIANTS the case runs under where not all six (restricted(): the reach tables)
        self.knobs = {}                       # further switches around the launch, as `hostcheck optrace` names them: rowfuse_grid, temporal_budget

    @functools.cached_property
    def ref(self):
        """name -> (ref64, scale64)"""
        return self._ref()

    def check(self, got, label=""):
        for k, (ref, scale) in self.ref.items():
            w = self.where[k] if isinstance(self.where, dict) else self.where
            c = self.c[k] if isinstance(self.c, dict) else self.c
            u = self.u[k] if isinstance(self.u, dict) else self.u
            oc.assert_elementwise(got[k], ref, scale, c, where=w, label=f"{label}{self.name}:{k}", u=u)
            if k == "y":
                for rname, mask in self.regions.items():
                    oc.assert_elementwise(got[k], ref, scale, c, where=w, label=f"{label}{self.name}:{k}:{rname}", mask=mask, u=u)
        for k, want in self.exact.items():
            oc.assert_bits(got[k], want, where=self.where[k] if isinstance(self.where, dict) else self.where, label=f"{label}{self.name}:{k}")
        if self.post is not None and not label.startswith("model"):      # a property of the kernel's arithmetic, not of torch's
            self.post(got)


# the six kernel choices the GPU operator tests run every case under: name -> (force_tile, force_splits)
VARIANTS = {"auto": (0, 0), "row128-tiles": (1, 0), "split-k-3": (0, 3), "pingpong": (3, 0), "pingpong-split-k-2": (3, 2),
            "ppx-persistent": (7, 0)}


def call(entry, **ints):
    """One C-ABI call of a GEMM-family case as lavie_amd/ops.py makes it: the entry point without lavie_ / _f16, its integer
    arguments under the names of include/lavie_hip.h, 1 for each optional operand that is passed (bias, bias2, R, x2, sc1, sc2).
    What `hostcheck optrace` replays (gemm_reach)."""
    return entry, {k: int(v) for k, v in ints.items()}


def with_calls(case, calls, force=None):
    case.calls, case.force = calls, force
    return case


def local_calls(case, calls, **knobs):
    """with_calls for a kernel that does not depend on the GEMM choice: replayed once, under the switches it runs under itself"""
    case.calls, case.variants, case.knobs = calls, ("auto",), {k: int(v) for k, v in knobs.items() if v}
    return case


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def rnd(g, *shape, s=1.0, dtype=f16):
    return (torch.randn(*shape, generator=g) * s).to(dtype)


def d(t):
    return None if t is None else t.to(f64)


def rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# ------------------------------------------------------------------ linear family
LINEAR_SHAPES = [(1, 64, 64), (127, 64, 192), (130, 192, 64), (154, 320, 320), (160, 320, 320), (161, 320, 320),
                 (320, 256, 320), (480, 640, 320)]
LINEAR_OPTIONS = ["plain", "bias_residual", "bias2", "residual_in_place"]
# "bias2_residual" (bias + per-batch bias + residual: every operand of the epilogue at once) is run by the statistics cases alone


@functools.lru_cache(maxsize=None)
def linear_case(M, N, K, opt, force=None):
    """force: (tile mode, splits) forced around the launch, whatever the variant (splits = 1: unsplit where the cost rule would split)"""
    g = gen("linear", M, N, K, opt)
    a, w = rnd(g, M, K), rnd(g, N, K, s=1 / math.sqrt(K))
    ins = {"a": a, "w": w}
    rpb = (M + 1) // 2
    if opt in ("bias_residual", "bias2", "bias2_residual"):
        ins["bias"] = rnd(g, N, dtype=f32t)
    if opt in ("bias2", "bias2_residual"):
        ins["bias2"] = rnd(g, -(-M // rpb), N, dtype=f32t)
    if opt in ("bias_residual", "residual_in_place", "bias2_residual"):
        ins["r"] = rnd(g, M, N)
    b2rows = torch.arange(M) // rpb

    def run(ops, i, o):
        ops.linear(i["a"], i["w"], bias=i.get("bias"), residual=i.get("r"), bias2=i.get("bias2"),
                   rows_per_batch=rpb if "bias2" in i else 0, out=o["y"])

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        y = p(cv(a)) @ p(cv(w)).t()
        if "bias" in ins:
            y = y + p(cv(ins["bias"]))
        if "bias2" in ins:
            y = y + p(cv(ins["bias2"]))[b2rows]
        if "r" in ins:
            y = y + p(cv(ins["r"]))
        return y

    name = f"linear[{M}x{N}x{K},{opt}]" if force is None else f"linear[{M}x{N}x{K},{opt},f{force[0]},k{force[1]}]"
    case = Case(name, ins, {"y": ((M, N), f16)}, run, lambda: {"y": (terms(d, False), terms(d, True))},
                oc.gemm_c(K + 3), lambda: {"y": terms(lambda t: t.float(), False).half()}, oc.loc_rows(N),
                alias={"y": "r"} if opt == "residual_in_place" else None,
                setup=(lambda restore: forced(*force, restore)) if force is not None else None)
    return with_calls(case, [call("linear", lda=K, ldb2=N, rows_per_batch=rpb if "bias2" in ins else 0, ldr=N, ldc=N, M=M, N=N, K=K, geglu=0,
                                  bias="bias" in ins, bias2="bias2" in ins, R="r" in ins)], force)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


@functools.lru_cache(maxsize=None)
def geglu_case(M, C):
    """linear(..., geglu=True): [M, C] -> [M, 4C] = h * gelu(gate).  The output needs h and gate to (K + 8) 2^-23 of their own
    scales and is stored once in fp16: n = 1 (igemm_epilogue.h:170, the only fp16 conversion of the GEGLU branch)."""
    g = gen("geglu", M, C)
    a, w, b = rnd(g, M, C), rnd(g, 8 * C, C, s=1 / math.sqrt(C)), rnd(g, 8 * C, s=0.1)
    ins = {"a": a, "w": w, "b": b}

    def run(ops, i, o):
        wp, bp = ops.pack_geglu(i["w"], i["b"])
        ops.linear(i["a"], wp, bias=bp, geglu=True, out=o["y"])

    def ref():
        pre = d(a) @ d(w).t() + d(b)
        sc = d(a).abs() @ d(w).abs().t() + d(b).abs()
        h, gate = pre.chunk(2, -1)
        sh, sg = sc.chunk(2, -1)
        # |d(h gelu(g))| <= |gelu(g)| dh + |h| max|gelu'| dg, max|gelu'| < 1.13
        return {"y": (h * gelu64(gate), sh * gelu64(gate).abs() + h.abs() * 1.13 * sg)}

    def model():
        pre = a.float() @ w.float().t() + b.float()
        h, gate = pre.chunk(2, -1)
        return {"y": (h * F.gelu(gate)).half()}

    case = Case(f"geglu[{M}x{C}]", ins, {"y": ((M, 4 * C), f16)}, run, ref, oc.round_c(1), model, oc.loc_rows(4 * C))
    return with_calls(case, [call("linear", lda=C, ldb2=8 * C, rows_per_batch=0, ldr=4 * C, ldc=4 * C, M=M, N=8 * C, K=C, geglu=1, bias=1)])


@functools.lru_cache(maxsize=None)
def lnfold_case(M, N, K):
    g = gen("lnfold", M, N, K)
    a = (torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).half()
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    wf = (w * gamma).half()
    s = wf.float().sum(1)
    bf = (w @ beta + torch.randn(N, generator=g))
    af = a.float()
    stats = torch.stack([af.mean(1), (af.var(1, unbiased=False) + 1e-5).rsqrt()], 1).contiguous()
    ins = {"a": a, "wf": wf, "bias": bf, "s": s, "stats": stats}

    def run(ops, i, o):
        ops.linear_lnfold(i["a"], i["wf"], i["bias"], i["s"], i["stats"], out=o["y"])

    def ref():
        mean, rstd = d(stats[:, :1]), d(stats[:, 1:])
        acc = d(a) @ d(wf).t()
        y = rstd * (acc - mean * d(s)) + d(bf)
        sc = rstd.abs() * (d(a).abs() @ d(wf).abs().t() + (mean * d(s)).abs()) + d(bf).abs()
        return {"y": (y, sc)}

    def model():
        acc = af @ wf.float().t()
        return {"y": (stats[:, 1:] * (acc - stats[:, :1] * s) + bf).half()}

    case = Case(f"lnfold[{M}x{N}x{K}]", ins, {"y": ((M, N), f16)}, run, ref, oc.gemm_c(K + 2), model, oc.loc_rows(N))
    return with_calls(case, [call("linear_lnfold", M=M, N=N, K=K, bias=1)])


def geglu_perm(N):
    """lavie_pack_geglu_f16's row order: packed row n holds source row perm[n] — 16-row blocks alternating value / gate
    (elementwise.hip geglu_src_row)."""
    n = torch.arange(N)
    j, i = n >> 5, n & 31
    return torch.where(i < 16, 16 * j + i, N // 2 + 16 * j + (i - 16))


@functools.lru_cache(maxsize=None)
def lnfold_geglu_case(M, C):
    """linear_lnfold(..., geglu=True): [M, C] -> [M, 4C], the feed-forward's first projection behind a folded LayerNorm.  lnfold_case's
    fold (reference and scale of the pre-activations), then geglu_case's h gelu(gate) with its 1.13 slope term and its single fp16
    rounding (igemm_epilogue.h:170); the folded weight, bias and row sums are formed in natural order and permuted into
    pack_geglu's row order on the host, as the engine packs all three with one permutation (engine.cpp:446-448)."""
    g = gen("lnfold_geglu", M, C)
    N = 8 * C
    a = (torch.randn(M, C, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).half()
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w = torch.randn(N, C, generator=g) / math.sqrt(C)
    wf = (w * gamma).half()
    s = wf.float().sum(1)
    bf = (w @ beta + 0.1 * torch.randn(N, generator=g))
    af = a.float()
    stats = torch.stack([af.mean(1), (af.var(1, unbiased=False) + 1e-5).rsqrt()], 1).contiguous()
    perm = geglu_perm(N)
    ins = {"a": a, "wf": wf[perm].contiguous(), "bias": bf[perm].contiguous(), "s": s[perm].contiguous(), "stats": stats}

    def run(ops, i, o):
        ops.linear_lnfold(i["a"], i["wf"], i["bias"], i["s"], i["stats"], geglu=True, out=o["y"])

    def ref():
        mean, rstd = d(stats[:, :1]), d(stats[:, 1:])
        pre = rstd * (d(a) @ d(wf).t() - mean * d(s)) + d(bf)
        sc = rstd.abs() * (d(a).abs() @ d(wf).abs().t() + (mean * d(s)).abs()) + d(bf).abs()
        h, gate = pre.chunk(2, -1)
        sh, sg = sc.chunk(2, -1)
        return {"y": (h * gelu64(gate), sh * gelu64(gate).abs() + h.abs() * 1.13 * sg)}

    def model():
        pre = stats[:, 1:] * (af @ wf.float().t() - stats[:, :1] * s) + bf
        h, gate = pre.chunk(2, -1)
        return {"y": (h * F.gelu(gate)).half()}

    case = Case(f"lnfold_geglu[{M}x{C}]", ins, {"y": ((M, 4 * C), f16)}, run, ref, oc.round_c(1), model, oc.loc_rows(4 * C))
    return with_calls(case, [call("linear_lnfold_geglu", M=M, N=N, K=C, bias=1)])


# The smallest shape the planner (igemm.hip igemm_plan) sends to each GEMM-family instantiation that LINEAR_SHAPES, the two GEGLU and
# the two lnfold shapes of the first tables do not reach, found with `hostcheck optrace` (gemm_reach) and asserted from it by
# tests/test_gemm_reach_host.py.  Variants: the ones a case runs under — all six where the shape is small, else those whose trace
# names the target.  "past the cap": more tiles than the persistent kernel's 256 workgroups, so that its deferred-epilogue path runs
# (a second tile from 257 tiles on; first, steady-state and last tile in one workgroup from 513 on).
#  instantiation                        case (M x N x K | M x C)            variants              rule that makes it the smallest
#  igemm_ppx_kernel<0, 5, 2>            lnfold 160x320x320, 320x320x320     all (ppx-persistent)  M % 160 == 0, nk >= 5, N % 320 == 0 (igemm_ppx_eligible)
#  igemm_ppx_kernel<0, 4, 2>            lnfold 160x256x320, 320x256x320     all (ppx-persistent)  ... N % 256 == 0 and N % 320 != 0
#  igemm_ppx_kernel<1, 4, 0>            geglu 160x320 (N = 2560, K = 320)   all (ppx-persistent)  GEGLU: N = 8C % 256 == 0, nk = C / 64 >= 5 -> C = 320
#  igemm_ppx_kernel<1, 4, 2>            lnfold_geglu 160x320                all (ppx-persistent)  the same behind a fold
#  igemm_kernel<2, 2, 4, 4, 2, false, 1> with ln_stats    lnfold_geglu 129x64, 154x320   all       ragged M: the 128-row kernel everywhere but `pingpong`
#  igemm_pp_kernel<false, 1, 4> with ln_stats             lnfold_geglu 154x320           pingpong  forced: N % 256 == 0
#  igemm_pp_kernel<false, 1, 4> by its grid rule          geglu / lnfold_geglu 2233x512  auto      nk >= 8 (GEGLU_PP_MIN_NK) with N = 8C % 256 == 0 -> C = 512,
#                                                                                                  16 column tiles; >= 85 % of 256 -> 14 row tiles; ragged last
#  igemm_pp_kernel<false, 0, 4>         linear 34721x256x640                auto                  N % 256 == 0 and % 320 != 0, nk >= 10, 218 tiles of 160x256 (85 % of a
#                                                                                                  round), not the persistent kernel's (M % 160 != 0): 217 * 160 + 1 rows
#  igemm_pp_kernel<true, 0, 4>          temporal_conv 1x128->256, f8, d4341, t5   auto          the same rule on a gathered A operand, where K is shortest: nk = taps cin / 64
#                                                      >= 10 -> 5 taps x 128 channels (a 3x3 conv needs 9 x 128), 8 x 4341 = 34728 rows = 218 tiles (d4340: 217, the
#                                                      128-row kernel); cout = 256 < 1024 keeps it off the halo-patch kernel (patch_fits).  The temporal gather is what
#                                                      is covered; the 3x3 gather of this instantiation would need 186x187 pixels and 2.05e10 multiply-adds
#  igemm_kernel<2, 2, 4, 4, 2, false, 0>   linear 2689x512x192              all (split-k-3)       the 128-wide tile of the 128-row kernel wins only where the 64-wide one
#                                                      needs a second round of 512 workgroups (igemm_pick_bn): 22 row tiles x 4 x 3 splits = 264 > 256, M = 21 * 128 + 1
#  igemm_kernel<2, 2, 4, 4, 2, true, 0>    conv 1x64->512, 52x52            all (split-k-3)       the same for a gathered A operand: 2704 pixels = 22 row tiles
#  igemm_pp_kernel<true, 0, 5>          conv 1x64->320, 5x7                 all (pingpong)        mode 3 forces it wherever cout % 320 == 0
#  igemm_patch_kernel<0, 4, 0>          conv 1x64->128, 40x8, force 5       forced                cout % 128 == 0 and % 160 != 0, one 320-pixel tile of whole image rows
#  igemm_patch_kernel<0, 5, 1>          conv 1x64->160, 10x96, force 5      forced                320 % W != 0: 10 x 32 tiles, W % 32 == 0, H % 10 == 0 -> 10 x 96
#  igemm_patch_kernel<0, 4, 2>          temporal_conv 1x64->128, f8, d40, force 5   forced        F | 320, D % (320 / F) == 0, cout % 128 == 0: one tile
#  past the cap (igemm_ppx.hip:162-182: 8 XCD chunks, workgroup j of a chunk takes its tiles j, j + 32, j + 64):
#  igemm_ppx_kernel<0, 5, 1>            linear 20640x1280x320 bias_residual, residual_in_place   auto, ppx-persistent   129 x 4 = 516 tiles >= 513: four
#                                                                                                  workgroups run three tiles; nk = 5 is the kernel's minimum
#  igemm_ppx_kernel<0, 4, 1>            linear 20640x1024x320 bias_residual  auto, ppx-persistent  the same on the 256-wide tile: 516 tiles (not in the issue's list)
#  igemm_ppx_kernel<0, 5, 0> / <0, 4, 0>   linear 20640x640x320 / 20640x512x320 plain            auto, ppx-persistent   129 x 2 = 258 tiles >= 257
#  igemm_ppx_kernel<0, 5, 2> / <0, 4, 2>   lnfold 13760x960x320 / 20640x512x320                  auto, ppx-persistent   258 tiles; 86 x 3 for <0, 5, 2>, so that a
#                                                      workgroup's second tile (its first + 32) lies in another column tile and every aux piece differs between the two
#  igemm_ppx_kernel<1, 4, 0> / <1, 4, 2>   geglu / lnfold_geglu 5120x320                         auto, ppx-persistent   32 x 10 = 320 tiles of 160x256; the automatic
#                                                      rule counts 320-wide tiles for GEGLU too (ppx_shape: 32 x 8 = 256 >= 256), so M = 4160 (260 tiles) stays on the 128-row kernel
#  at model depth (deep_cases(), PARITY_SPLIT_CASES; grids and split factors asserted from the trace by test_gemm_reach_host.py):
#  case                                             variant                     kernel                                  splits
#  parity 2x1280, 10x16                             auto                        igemm_patch_kernel<0, 5, 3> + reduce_cs  4 (planned; grid 8, 4, 4)
#  parity 14x640, 10x16                             auto                        igemm_patch_kernel<0, 5, 3> + reduce_cs  2 (planned; grid 28, 2, 4)
#  conv 1x192+128->320, 5x7 (nk 45), sc(192, 128) (nk 50)   the six variants    128-row gather <2, 2, 4, 5, 2, true, 0> / ping-pong gather <true, 0, 5>   1, 2, 3, automatic
#  conv 1x192+128->320, 5x7, sc(192, 128)           forced 1 / 3                the same two kernels                    1, 3 (t_begin 16, 33), 10 (t_begin 45: the first shortcut tile), 25 (46, 48)
#  conv 5x192+128->320, 8x8 and 1x..., 10x96        forced 5                   igemm_patch_kernel<0, 5, 0> / <0, 5, 1>  1, 2 ([0,2) [2,5)), 3 ([0,1) [1,3) [3,5)), 5
#  linear 130x192x5120 bias_residual (80 K-tiles)   auto                        128-row kernel + reduce                 6 (the cost rule; ranges of 13 / 14 K-tiles)
#  linear 640x1280x5120 bias_residual               auto                        128-row kernel + reduce                 5 (the cost rule, at the product's level-3 width)
#  linear 160x320x5120 bias_residual                forced (1, 1) (3, 1) (7, 1) 128-row / ping-pong / persistent        1: one 80-tile K loop per kernel
#  geglu 160x1280 (20 K-tiles, the family's longest in the model: C = 1280)   the six variants     GEGLU kernels        1
#  TOO_LARGE: none
BIG = ("auto", "ppx-persistent")
# 80 K-tiles (K = 5120, the level-3 feed-forward output GEMM): (M, N, K, option, variants or None = all six)
DEEP_LINEAR = [(130, 192, 5120, "bias_residual", None), (160, 320, 5120, "bias_residual", None), (640, 1280, 5120, "bias_residual", ("auto",))]
DEEP_AUTO = ["linear[130x192x5120,bias_residual]", "linear[640x1280x5120,bias_residual]"]      # `auto` must plan more than 3 splits
DEEP_UNSPLIT = [(1, 1), (3, 1), (7, 1)]                   # (tile mode, force_splits = 1) around linear 160x320x5120: one unsplit pass per kernel
# (M, N, K, option, variants or None = all six)
REACH_LINEAR = [(20640, 1280, 320, "bias_residual", BIG), (20640, 1280, 320, "residual_in_place", BIG), (20640, 1024, 320, "bias_residual", BIG), (20640, 640, 320, "plain", BIG),
                (20640, 512, 320, "plain", BIG), (34721, 256, 640, "plain", ("auto",)), (2689, 512, 192, "bias_residual", None)]
REACH_LNFOLD = [(160, 320, 320, None), (160, 256, 320, None), (320, 320, 320, None), (320, 256, 320, None), (13760, 960, 320, BIG), (20640, 512, 320, BIG)]
# (160, 1280): C = 1280 is the widest feed-forward of the model, K = 20 K-tiles: the longest K loop the GEGLU epilogue sees
REACH_GEGLU = [(160, 320, None), (2233, 512, ("auto",)), (5120, 320, BIG), (160, 1280, None)]
REACH_LNFOLD_GEGLU = [(129, 64, None), (154, 320, None), (160, 320, None), (2233, 512, ("auto",)), (5120, 320, BIG)]
# tiles of the persistent kernel each past-the-cap case must have (name prefix -> (tile width, least tile count))
PAST_CAP = {"linear[20640x1280x320,bias_residual]": (320, 513), "linear[20640x1280x320,residual_in_place]": (320, 513),
            "linear[20640x1024x320,bias_residual]": (256, 513),
            "linear[20640x640x320,plain]": (320, 257), "linear[20640x512x320,plain]": (256, 257), "lnfold[13760x960x320]": (320, 257),
            "lnfold[20640x512x320]": (256, 257), "geglu[5120x320]": (256, 257), "lnfold_geglu[5120x320]": (256, 257)}
TCONV_FORCED = [(1, 64, 128, 8, 40)]                      # force 5, taps 3 and 5
REACH_TCONV = [(1, 128, 256, 8, 4341, 5, ("auto",))]      # (b, cin, cout, frames, d, taps, variants)

# instantiations whose smallest reaching shape is above 2^34 multiply-adds for the float64 reference and its scale: name -> shape and count
TOO_LARGE = {}
# registered implicit-GEMM instantiations no route of the planner selects (test_gemm_reach_host.py: each is registered and unreached)
NOT_PLANNED = {}
# kernels of the launch-trace fixture that no operator entry point launches: name -> the existing test that exercises it
WHOLE_FORWARD = "tests/test_gpu_engine.py (whole-output rel-L2 of the engine's blocks and forwards against the fp32 oracle)"
NO_OPERATOR_ENTRY = {
    # (the producer-side statistics kernels gn_fold_kernel, rowstat_finalize_kernel and splitk_reduce_cs_kernel were listed here until
    # lavie_debug_op_statistics, lavie_group_norm_stats_f16 and lavie_rowstat_finalize_f32 reached them: stats_cases(), stats_local_cases())
    # the chunked form of the pack (the unchunked one: pack_conv_out_case) and the packs of the GEGLU / parity operands: bit-moves
    # whose output every conv / GEGLU / parity case consumes
    "pack_conv3x3_parity_kernel": "tests/test_gpu_ops_local.py::test_upsample_conv3x3_parity (ops.pack_conv3x3_parity)",
    "pack_geglu_bias_kernel": "tests/test_gpu_ops_local.py::test_geglu (ops.pack_geglu)",
    "pack_geglu_rows_kernel": "tests/test_gpu_ops_local.py::test_geglu (ops.pack_geglu)",
}
# EPI_LINEAR igemm_* instantiations that a case reaches, but none with column statistics in an unsplit launch: name -> reason
NO_COLSTAT = {}
# gather kernels of the row-resident blocks' pack / bind steps: launched by lavie_pack_geglu_mlp_f16 and lavie_bind_cross_block[_long]_f16
# (`hostcheck optrace`, asserted by test_gemm_reach_host.py), which the block cases call before the kernel whose output they check
PACK_STEP_KERNELS = {
    "rf_gather8_kernel": "tests/test_gpu_ops_local.py::test_geglu_mlp, ::test_cross_block (ops.pack_geglu_mlp, ops.pack_cross_block[_long])",
    "rf_gather_f16_f32_kernel": "tests/test_gpu_ops_local.py::test_geglu_mlp (ops.pack_geglu_mlp)",
    "xb_gather2_kernel": "tests/test_gpu_ops_local.py::test_cross_block (ops.bind_cross_block[_long])",
    "xb_gather8_kernel": "tests/test_gpu_ops_local.py::test_cross_block (ops.bind_cross_block[_long])",
}
# the end and glue kernels of tests/test_gpu_ends_local.py: each must be launched by a case of ends_cases() (test_gemm_reach_host.py)
ENDS_KERNELS = ("timestep_sinusoid_kernel", "gemv_kernel", "add_class_emb_silu_kernel", "conv_in_kernel", "conv_out4_kernel<5>", "conv_out4_kernel<6>",
                "conv_out_kernel", "ln_fold_kernel", "pack_conv_in_kernel", "pack_conv3x3_kernel", "pack_geglu_vec_kernel", "copy_rows_kernel",
                "f16_to_f32_kernel", "fill_relpos_bias_kernel")
# the fixture's attention kernels: each must be in the replayed launches of an attention case (test_gemm_reach_host.py), whose
# kernel is the one attention_route names (test_opcheck_host.py)
ATTENTION_KERNELS = ("attention_dma_kernel<", "attention_kernel<", "attention_wide_kernel")
# ... except these, which a forward launches and no per-element case does (ATT_ROUTES has the sparse-causal twins off head dim 40
# at one query-tile count only): name -> the existing test that exercises it
ATTENTION_NO_CASE = {
    "attention_dma_kernel<10, 2, 3, false, true, true, 4>": "tests/test_gemm_plan_trace.py (sparse-causal head dim 80 at more than 192 tokens: in the interpolation forward's launch trace; its QT 1 twin has the per-element cases)",
}
# the fixture's other names, by the prefix of the kernel the LayerNorm cases launch (not replayed) ...
# ... and the FreeU kernels of the trace's FreeU case, whose launches tests/freeucases.py mirrors (test_freeu_host.py) and whose output
# tests/test_gpu_freeu_local.py checks per element
COVERED_ELSEWHERE = ("layernorm_kernel", "freeu_apply_kernel", "freeu_sums_kernel")
# ... and of the GroupNorm, row-resident and temporal cases, which describe their calls: every such name of a forward's trace must be in
# the replayed launches of a case (test_gemm_reach_host.py::test_local_kernels_of_a_forward_are_reached)
LOCAL_KERNELS = ("gn_affine_kernel", "gn_apply_kernel<", "gn_stats_kernel<", "gn_finalize_kernel", "gn_fold_kernel", "rowstat_finalize_kernel", "geglu_mlp_kernel<", "cross_block_kernel<",
                 "temporal_block_kernel<", "proj_qkv_kernel<", "temporal_stream_kernel<", "temporal_attention_kernel<")


# ------------------------------------------------------------------ 3x3 convolution family
class forced:
    """lavie_debug_force_tile / force_splits for the duration of a case, then back to what the fixture set."""

    def __init__(self, tile, splits, restore):
        self.tile, self.splits, self.restore = tile, splits, restore

    def __enter__(self):
        from lavie_amd import _lib
        lib = _lib.load()
        _lib.check(lib.lavie_debug_force_tile(self.tile), "lavie_debug_force_tile")
        lib.lavie_debug_force_splits(self.splits)

    def __exit__(self, *exc):
        from lavie_amd import _lib
        lib = _lib.load()
        lib.lavie_debug_force_tile(self.restore[0])
        lib.lavie_debug_force_splits(self.restore[1])


class grid_cap:
    """lavie_debug_rowfuse_grid for the duration of a case: at most `cap` workgroups for the row-resident launchers, then back to 0
    (automatic).  Takes the fixture's (tile, splits) like `forced` and leaves them alone."""

    def __init__(self, cap, restore=None):
        self.cap = cap

    def __enter__(self):
        from lavie_amd import _lib
        _lib.check(_lib.load().lavie_debug_rowfuse_grid(self.cap), "lavie_debug_rowfuse_grid")

    def __exit__(self, *exc):
        from lavie_amd import _lib
        _lib.load().lavie_debug_rowfuse_grid(0)


def conv2d_any(x, w, b, stride, ups, pad):
    if ups:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    if pad == (0, 1):
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=stride)
    return F.conv2d(x, w, b, stride=stride, padding=1)


def border_mask(n, h, w, c):
    m = torch.ones(n, h, w, c, dtype=torch.bool)
    if h > 2 and w > 2:
        m[:, 1:-1, 1:-1] = False
    return m.reshape(-1)


def lines_mask(n, h, w, c, ys, xs):
    m = torch.zeros(n, h, w, c, dtype=torch.bool)
    for y in ys:
        if 0 <= y < h:
            m[:, y] = True
    for x in xs:
        if 0 <= x < w:
            m[:, :, x] = True
    return m.reshape(-1)


@functools.lru_cache(maxsize=None)
def conv_case(n, c1, cout, h, w, stride=1, ups=0, pad=None, c2=0, csc=0, extras=False, force=None, splits=0, parity=False):
    """extras: per-frame bias2 + residual (the halo-patch test's form); csc: fused 1x1 shortcut over two raw sources of csc
    channels each (or a pair (sc1, sc2) of unequal widths) + bias2 (the ResnetBlock3D form); force: (tile mode, splits) forced around the launch."""
    g = gen("conv", n, c1, cout, h, w, stride, ups, pad, c2, csc, extras, parity)
    cin = c1 + c2
    csc1, csc2 = csc if isinstance(csc, tuple) else (csc, csc)      # (sc1, sc2): shortcut sources of unequal width
    x1 = rnd(g, n, c1, h, w)
    x2 = rnd(g, n, c2, h, w) if c2 else None
    wt = rnd(g, cout, cin, 3, 3, s=1 / math.sqrt(9 * cin))
    b = rnd(g, cout, dtype=f32t)
    ins = {"x1": rows(x1), "wt": wt, "b": b}
    if c2:
        ins["x2"] = rows(x2)
    s1 = s2 = ws = None
    if csc:
        s1, s2 = rnd(g, n, csc1, h, w), rnd(g, n, csc2, h, w)
        ws = rnd(g, cout, csc1 + csc2, 1, 1, s=1 / math.sqrt(csc1 + csc2))
        ins.update(s1=rows(s1), s2=rows(s2), ws=ws)
    probe = conv2d_any(torch.zeros(1, 1, h, w), torch.zeros(1, 1, 3, 3), None, stride, ups, pad)
    ho, wo = probe.shape[2:]
    rpb = ho * wo                                            # one bias2 row per frame
    if csc or extras:
        ins["b2"] = rnd(g, n, cout, dtype=f32t)
    res = None
    if extras:
        res = rnd(g, n, cout, ho, wo)
        ins["r"] = rows(res)

    def run(ops, i, o):
        if parity:
            ops.upsample_conv3x3(i["x1"], ops.pack_conv3x3_parity(i["wt"]), i["b"], n, h, w, out=o["y"])
            return
        wp = ops.pack_conv3x3(i["wt"], i.get("ws"))
        if pad is not None:
            ops.conv3x3(i["x1"], wp, i["b"], n, h, w, stride=stride, pad=pad, out=o["y"])
        else:
            ops.conv3x3(i["x1"], wp, i["b"], n, h, w, x2=i.get("x2"), sc1=i.get("s1"), sc2=i.get("s2"), bias2=i.get("b2"),
                        rows_per_batch=rpb if "b2" in i else 0, residual=i.get("r"), stride=stride, ups=ups, out=o["y"])

    def parity_terms(cv, p):
        """The four 2x2 convs on x with the tap sums the pack step forms: summed in fp32, rounded to fp16 (elementwise.hip:592-593) —
        a property of the packed operand, so reference and scale are taken from the same rounded sums."""
        wf = wt.float()
        sets = {0: ([0], [1, 2]), 1: ([0, 1], [2])}            # output parity -> kernel rows summed for source offset (-1 | 0), (0 | +1)
        xp = F.pad(p(cv(x1)), (1, 1, 1, 1))
        y = torch.zeros(n, cout, 2 * h, 2 * w, dtype=xp.dtype)
        for py in (0, 1):
            for px in (0, 1):
                w2 = torch.stack([torch.stack([wf[:, :, ry][:, :, :, rx].sum((2, 3)) for rx in sets[px]], -1) for ry in sets[py]], -2)
                w2 = p(cv(w2.half()))                                                  # [cout, cin, 2, 2]
                y[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], w2, p(cv(b)))
        return rows(y)

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        if parity:
            return parity_terms(cv, p)
        xin = torch.cat([x1, x2], 1) if c2 else x1
        y = conv2d_any(p(cv(xin)), p(cv(wt)), p(cv(b)), stride, ups, pad)
        if csc:
            y = y + F.conv2d(p(cv(torch.cat([s1, s2], 1))), p(cv(ws)))
        if "b2" in ins:
            y = y + p(cv(ins["b2"]))[:, :, None, None]
        if res is not None:
            y = y + p(cv(res))
        return rows(y)

    c = oc.gemm_c((4 if parity else 9) * cin + csc1 + csc2 + 3)
    regions = {"border": border_mask(n, ho, wo, cout)}
    if parity:
        for py in (0, 1):
            for px in (0, 1):
                m = torch.zeros(n, ho, wo, cout, dtype=torch.bool)
                m[:, py::2, px::2] = True
                regions[f"parity{py}{px}"] = m.reshape(-1)
    if force is not None or parity:
        # tile seams of the halo-patch geometries: 320 pixels per tile as whole image rows (or 10 x 32 blocks when a row is wider
        # than a tile): the rows / columns on either side of every tile boundary
        if w <= 320 and 320 % w == 0:
            tr, tc = max(320 // w, 1), w
        else:
            tr, tc = 10, 32
        sh, sw = (2, 2) if parity else (1, 1)
        ys = [y * sh + k for y in range(tr, h, tr) for k in (-1, 0)] if tr < h else []
        xs = [x * sw + k for x in range(tc, w, tc) for k in (-1, 0)] if tc < w else []
        regions["seams"] = lines_mask(n, ho, wo, cout, ys, xs) | regions["border"]
    name = f"conv[{n}x{c1}+{c2}->{cout},{h}x{w},s{stride},u{ups},pad{pad},sc{csc},ex{int(extras)},f{force},k{splits},par{int(parity)}]"
    setup = (lambda restore: forced(force, splits, restore)) if force is not None else None
    case = Case(name, ins, {"y": ((n * ho * wo, cout), f16)}, run, lambda: {"y": (terms(d, False), terms(d, True))}, c,
                lambda: {"y": terms(lambda t: t.float(), False).half()}, oc.loc_image(n, ho, wo, cout), regions=regions, setup=setup)
    if parity:
        calls = [call("upsample_conv3x3", NI=n, Hi=h, Wi=w, C=c1, bias=1)]
    elif pad is not None:
        calls = [call("conv3x3_down", C=c1, NI=n, Hi=h, Wi=w, Cout=cout, stride=stride, pad_lo=pad[0], bias=1)]
    else:
        calls = [call("conv3x3", C1=c1, C2=c2, SC1=csc1, SC2=csc2, ldb2=cout, rows_per_batch=rpb if "b2" in ins else 0, NI=n, Hi=h, Wi=w,
                      Cout=cout, stride=stride, ups=ups, bias=1, bias2="b2" in ins, R="r" in ins, x2=bool(c2), sc1=bool(csc), sc2=bool(csc))]
    return with_calls(case, calls, (force, splits) if force is not None else None)


CONV_CASES = [dict(n=1, c1=64, cout=64, h=1, w=1), dict(n=1, c1=64, cout=64, h=3, w=3),
              dict(n=2, c1=64, cout=64, h=5, w=7, stride=2), dict(n=3, c1=64, cout=128, h=4, w=6, ups=1),
              dict(n=2, c1=64, c2=64, cout=64, h=3, w=5, csc=64),
              dict(n=1, c1=128, cout=128, h=13, w=18, stride=2, pad=(0, 1)), dict(n=1, c1=128, cout=128, h=2, w=2, stride=2, pad=(0, 1)),
              # the gathered ping-pong kernel (`pingpong`) and the 128-wide tile of the 128-row kernel (`split-k-3`): the reach table above
              dict(n=1, c1=64, cout=320, h=5, w=7), dict(n=1, c1=64, cout=512, h=52, w=52)]
# Two sources of unequal width, 192 + 128 channels = 3 + 2 slabs of 64 (the product's convs concatenate 1280 + 640, 640 + 320): with more
# than one slab in a segment the (segment, slab, tap) cursor's slab-major, tap-minor order differs from its transpose, and a split-K
# range can begin inside a segment that is not the first.  K-tiles: 27 + 18 (nk = 45), with the fused shortcut over 192 + 128 raw
# channels 27 + 18 + 3 + 2 (nk = 50).  cout = 320: the 160-wide tile of the 128-row gather kernel, and the ping-pong gather kernel under
# mode 3.  Where each split begins is computed by kloop_position and asserted by tests/test_gemm_reach_host.py.
SEG = dict(n=1, c1=192, c2=128, cout=320, h=5, w=7)
SEG_SC = dict(SEG, csc=(192, 128))
CONV_CASES += [SEG, SEG_SC]                               # under the six variants; then forced (tile mode, splits): unsplit, 3 and 10 splits
SEG_FORCED = [(t, s) for t in (1, 3) for s in (1, 3, 10, 25)]      # 25: ranges of 2 K-tiles, t_begin 46 and 48 inside the shortcut segments
# the halo-patch kernel (9-tap segments only) over the same 3 + 2 slabs, split over whole slabs: whole-row tiles and 2-D tiles; unsplit
# (force_splits = 1), [0,2) [2,5), [0,1) [1,3) [3,5), and one slab a range: [4,5) begins inside segment 1
# (cout = 320, two 160-wide column tiles: the planner leaves N % 64 != 0 unsplit, so cout = 160 as in HALO_CASES would never split)
HALO_SEG_CASES = [dict(n=5, c1=192, c2=128, cout=320, h=8, w=8, extras=True), dict(n=1, c1=192, c2=128, cout=320, h=10, w=96, extras=True)]
HALO_SEG_SPLITS = (1, 2, 3, 5)


def kloop_segments(ints):
    """[(nchunks, ntaps)] of a conv3x3 call: its 9-tap sources, then its 1-tap shortcut sources, sources of 0 channels skipped
    (igemm_setup_conv3x3)"""
    return [(ints[k] // 64, taps) for k, taps in (("C1", 9), ("C2", 9), ("SC1", 1), ("SC2", 1)) if ints.get(k)]


def kloop_position(segs, t):
    """(segment, slab, tap) of K-tile t of the flattened K loop: segment-major, then slab-major, tap-minor (igemm.hip:138-148)"""
    for i, (nchunks, ntaps) in enumerate(segs):
        if t < nchunks * ntaps:
            return i, t // ntaps, t % ntaps
        t -= nchunks * ntaps
    raise IndexError(t)


def split_begins(nk, s):
    """t_begin of each split-K range of nk K-tiles under s splits (igemm.hip:112)"""
    return [nk * i // s for i in range(s)]


HALO_CASES =[dict(n=5, c1=64, cout=160, h=8, w=8, extras=True), dict(n=1, c1=64, cout=160, h=40, w=16, extras=True),
              dict(n=1, c1=128, cout=256, h=20, w=128, extras=True), dict(n=2, c1=64, c2=64, cout=256, h=10, w=96, extras=True, splits=2),
              # the 128-wide tile on whole image rows and the 160-wide one on 10 x 32 tiles (the reach table above)
              dict(n=1, c1=64, cout=128, h=40, w=8, extras=True), dict(n=1, c1=64, cout=160, h=10, w=96, extras=True)]
# (2, 320, 10, 16) is the smallest geometry lavie_upsample_conv3x3_supported takes: 160 channels, (1, 320, 10, 16), (2, 320, 5, 16),
# (2, 320, 10, 8) and (1, 320, 5, 8) are all refused (test_upsample_conv3x3_parity asserts it)
PARITY_CASES = [(2, 320, 10, 16), (32, 320, 5, 8)]
PARITY_REFUSED = [(2, 160, 10, 16), (1, 320, 10, 16), (2, 320, 5, 16), (2, 320, 10, 8), (1, 320, 5, 8)]
# The parity form under split-K (igemm.hip plan_splits, the par_ups branch: wgs = source tiles x (C / 160) x 4 parities; 1 split from 218
# workgroups, 2 where 2 wgs >= 218 and nchunks >= 10, else 4 where nchunks >= 20; force_splits does not apply), the smallest geometry of
# each factor.  Both cases above have nchunks = 5 and run unsplit.  (n, c, h, w, splits the planner must choose):
#  (2, 1280, 10, 16)   one 320-row source tile per parity, 1 x 8 x 4 = 32 workgroups, nchunks = 20 -> 4 splits (the base UNet's first
#                      upsampler at 16 frames plans 4).  Reference in its 4-tap form: 1280 rows x 1280 x 5120 = 8.4e9 multiply-adds
#  (14, 640, 10, 16)   7 source tiles, 7 x 4 x 4 = 112 workgroups (2 x 112 >= 218), nchunks = 10 -> 2 splits.  8960 rows x 640 x 2560 =
#                      1.47e10 multiply-adds, under the 2^34 = 1.72e10 of TOO_LARGE
# The reduce behind the launch writes the column statistics: 32-row contiguous blocks of output rows in ONE set, not four parity sets.
PARITY_SPLIT_CASES = [(2, 1280, 10, 16, 4), (14, 640, 10, 16, 2)]


def parity_case(n, c, h, w):
    return conv_case(n=n, c1=c, cout=c, h=h, w=w, ups=1, parity=True)


@functools.lru_cache(maxsize=None)
def temporal_conv_case(b, cin, cout, f, dd, taps, force=None):
    """force: the tile mode forced around the launch (5: the halo-patch kernel's temporal mode wherever its geometry holds)"""
    g = gen("tconv", b, cin, cout, f, dd, taps)
    x = rnd(g, b, cin, f, dd)                               # [b, c, f, d]
    wt = rnd(g, cout, cin, taps, 1, 1, s=1 / math.sqrt(taps * cin))
    bias, b2 = rnd(g, cout, dtype=f32t), rnd(g, b, cout, dtype=f32t)
    r = rnd(g, b, cout, f, dd)
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(b * f * dd, -1).contiguous()
    ins = {"x": to_rows(x), "wt": wt, "bias": bias, "b2": b2, "r": to_rows(r)}

    def run(ops, i, o):
        ops.temporal_conv(i["x"], ops.pack_temporal_conv(i["wt"]), i["bias"], b, f, dd, taps, bias2=i["b2"], residual=i["r"], out=o["y"])

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        y = F.conv3d(p(cv(x))[..., None], p(cv(wt)), p(cv(bias)), padding=(taps // 2, 0, 0))[..., 0]
        return to_rows(y + p(cv(b2))[:, :, None, None] + p(cv(r)))

    ends = torch.zeros(b, f, dd, cout, dtype=torch.bool)
    first, last = ends.clone(), ends.clone()
    first[:, 0] = True
    last[:, -1] = True
    name = f"temporal_conv[{b}x{cin}->{cout},f{f},d{dd},t{taps}" + ("]" if force is None else f",f{force}]")
    case = Case(name, ins, {"y": ((b * f * dd, cout), f16)}, run,
                lambda: {"y": (terms(d, False), terms(d, True))}, oc.gemm_c(taps * cin + 3),
                lambda: {"y": terms(lambda t: t.float(), False).half()}, oc.loc_image(b * f, dd, 1, cout),
                regions={"first_frame": first.reshape(-1), "last_frame": last.reshape(-1)},
                setup=(lambda restore: forced(force, 0, restore)) if force is not None else None)
    return with_calls(case, [call("temporal_conv", C=cin, ldb2=cout, rows_per_batch=f * dd, B=b, F=f, D=dd, Cout=cout, taps=taps,
                                  bias=1, bias2=1, R=1)], (force, 0) if force is not None else None)


TCONV_SHAPES = [(1, 64, 64, 1, 7), (1, 64, 64, 2, 7), (3, 128, 64, 2, 7), (2, 64, 128, 8, 80)]


# ------------------------------------------------------------------ the VAE's edge convs
EDGE_IN = [(1, 3, 128, 1, 1), (1, 4, 512, 3, 5), (2, 8, 128, 7, 9)]
EDGE_OUT = [(1, 128, 3, 1, 1), (1, 256, 4, 3, 5), (2, 512, 8, 7, 9)]

# Past the first quad of a workgroup and the first grid-stride step.  The cases above have at most 126 pixels: conv_edge_out then runs
# 8 tiles = 2 workgroups of one quad (4 waves x 16 pixels) each, conv_edge_in 126 x Cout / 8 items on at most 32 workgroups of one step.
# edge_out_walk / edge_in_walk mirror the two launchers; each shape is the smallest that takes its path on the production grid.
#  case                                       walk                                               path it provides
#  conv_edge_out 1x128->3, 257x513, fp32      131841 pixels, 8241 tiles, 2061 quads, 2 a         <4, float>: every workgroup but the last walks two quads; the last (1030) has one
#                                             workgroup, grid 1031                               tile of one pixel in wave 0, three waves that break at q = 0, all four breaking at q = 1
#  conv_edge_out 1x8->8, 257x513, fp16        the same walk                                      <0, half_t>: the rolled loop with a single, partly guarded channel block (kq >= 1: no channel)
#  conv_edge_out 2x40->{3,8}, 7x9, both       126 pixels, 2 workgroups                           <0, *> with two channel blocks, the last of 8 channels
#  conv_edge_out 1x{128,256,512}->{3,4,8}, 20x16   320 pixels = 5 quads, 5 workgroups            the unrolled widths with four waves on interior pixels, all nine taps present
#  conv_edge_in 1x4->512, 129x128, fp16, tap  16512 x 64 = 1056768 items on 4096 workgroups      workgroups 0..31 take a second grid-stride step: items >= 1048576 = pixels >= 16384 = the
#  conv_edge_in 1x3->512, 129x128, fp32       the same                                           bottom image row, whose three lower taps and their tap biases fall outside the image
# (n, cin, cout, h, w, dtype, tap)
EDGE_IN_PAST = [(1, 4, 512, 129, 128, f16, True), (1, 3, 512, 129, 128, f32t, False)]
# (n, cin, cout, h, w, dtype)
EDGE_OUT_PAST = ([(1, 128, 3, 257, 513, f32t), (1, 8, 8, 257, 513, f16)] + [(2, 40, co, 7, 9, dt) for co, dt in ((3, f16), (8, f32t))]
                 + [(1, 128, 3, 20, 16, f16), (1, 256, 4, 20, 16, f32t), (1, 512, 8, 20, 16, f16)])
EDGE_OUT_TILE, EDGE_OUT_MAX_WG, EDGE_IN_MAX_WG = 16, 2048, 4096


def edge_out_walk(M):
    """conv_edge.hip launch_edge_out: (grid, quads_per_wg) for M pixels.  Workgroup b walks quads b * per .. b * per + per - 1, wave w of
    quad q the tile 4 q + w, and leaves the loop at the first tile >= ntiles."""
    ntiles = -(-M // EDGE_OUT_TILE)
    quads = -(-ntiles // 4)
    per = -(-quads // EDGE_OUT_MAX_WG)
    return -(-quads // per), per


def edge_out_tiles(M):
    """tile -> (workgroup, step q, wave), and per workgroup the step at which each wave breaks (None: it runs all quads_per_wg steps)"""
    grid, per = edge_out_walk(M)
    ntiles = -(-M // EDGE_OUT_TILE)
    where = {(b * per + q) * 4 + w: (b, q, w) for b in range(grid) for q in range(per) for w in range(4) if (b * per + q) * 4 + w < ntiles}
    assert sorted(where) == list(range(ntiles))
    breaks = {b: [next((q for q in range(per) if (b * per + q) * 4 + w >= ntiles), None) for w in range(4)] for b in range(grid)}
    return where, breaks


def edge_in_walk(M, cout):
    """conv_edge.hip launch_conv_edge_in: (grid, [steps of each workgroup's fullest thread]) for M pixels: items = M * cout / 8, 256 a
    workgroup and step, at most EDGE_IN_MAX_WG workgroups, item idx = (step * grid + workgroup) * 256 + thread = pixel * (cout / 8) + group"""
    total = M * (cout // 8)
    grid = min(-(-total // 256), EDGE_IN_MAX_WG)
    return grid, [len(range(b * 256, total, grid * 256)) for b in range(grid)]


@functools.lru_cache(maxsize=None)
def edge_in_case(n, cin, cout, h, w, dtype, tap):
    """NCHW image (fp16 or fp32) -> channels-last fp16 rows.  fp16 input: GEMM family, K_terms = 9 cin + 10 (bias + nine tap biases).
    fp32 input: the kernel converts x to fp16 on load (conv_edge.hip:72-73), one deterministic conversion of the operand: reference
    and scale are taken from x.half(), and the GEMM-family bound holds for both input types."""
    g = gen("edge_in", n, cin, cout, h, w, dtype, tap)
    x = rnd(g, n, cin, h, w, dtype=dtype)
    wt, b = rnd(g, cout, cin, 3, 3, s=1 / math.sqrt(9 * cin)), rnd(g, cout, dtype=f32t, s=0.5)
    ins = {"x": x, "wt": wt, "b": b}
    if tap:
        ins["tb"] = rnd(g, 9, cout, dtype=f32t, s=0.3)

    def run(ops, i, o):
        ops.conv_edge_in(i["x"], ops.pack_conv_edge_in(i["wt"]), i["b"], cout, tap_bias=i.get("tb"), out=o["y"])

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        xx = cv(x.half())
        y = F.conv2d(p(xx), p(cv(wt)), p(cv(b)), padding=1)
        if tap:     # the taps of a pixel that fall inside the image add their bias: a conv of an all-ones image
            y = y + F.conv2d(torch.ones(n, 1, h, w, dtype=y.dtype), p(cv(ins["tb"])).t().reshape(cout, 1, 3, 3).contiguous(), padding=1)
        return rows(y)

    c = oc.gemm_c(9 * cin + 10)
    case = Case(f"conv_edge_in[{n}x{cin}->{cout},{h}x{w},{str(dtype)[6:]},tap{int(tap)}]", ins, {"y": ((n * h * w, cout), f16)}, run,
                lambda: {"y": (terms(d, False), terms(d, True))}, c,
                lambda: {"y": terms(lambda t: t.float(), False).half()}, oc.loc_image(n, h, w, cout),
                regions={"border": border_mask(n, h, w, cout)})
    case.edge = (n * h * w, cout)
    return local_calls(case, [call("conv_edge_in", x_dtype=dtype == f32t, N=n, Cin=cin, H=h, W=w, Cout=cout, bias=1, tap_bias=bool(tap))])


@functools.lru_cache(maxsize=None)
def edge_out_case(n, cin, cout, h, w, dtype):
    """channels-last fp16 rows -> NCHW image in fp16 or fp32 from fp32 accumulators: GEMM family, K_terms = 9 cin + 1."""
    g = gen("edge_out", n, cin, cout, h, w, dtype)
    x = rnd(g, n, cin, h, w)
    wt, b = rnd(g, cout, cin, 3, 3, s=1 / math.sqrt(9 * cin)), rnd(g, cout, dtype=f32t, s=0.5)
    ins = {"x": rows(x), "wt": wt, "b": b}

    def run(ops, i, o):
        ops.conv_edge_out(i["x"], ops.pack_conv_edge_out(i["wt"]), i["b"], n, h, w, cout, dtype, out=o["y"])

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        return F.conv2d(p(cv(x)), p(cv(wt)), p(cv(b)), padding=1)

    border = torch.ones(n, cout, h, w, dtype=torch.bool)
    if h > 2 and w > 2:
        border[:, :, 1:-1, 1:-1] = False
    case = Case(f"conv_edge_out[{n}x{cin}->{cout},{h}x{w},{str(dtype)[6:]}]", ins, {"y": ((n, cout, h, w), dtype)}, run,
                lambda: {"y": (terms(d, False), terms(d, True))}, oc.gemm_c(9 * cin + 1),
                lambda: {"y": terms(lambda t: t.float(), False).to(dtype)}, oc.loc_nchw(cout, h, w), regions={"border": border.reshape(-1)},
                u=oc.U32 if dtype == f32t else oc.U16)       # the relative term is the output format's unit roundoff (opcheck.py)
    case.edge = (n * h * w, cin)
    return local_calls(case, [call("conv_edge_out", y_dtype=dtype == f32t, N=n, Cin=cin, H=h, W=w, Cout=cout, bias=1)])


# ------------------------------------------------------------------ norms
def silu64(x):
    return x * torch.sigmoid(x)


@functools.lru_cache(maxsize=None)
def group_norm_case(nb, P, c1, c2=0, silu=True, eps=1e-5, offset=0.0, affine=False, tag=""):
    """[nb * P, c1 (+ c2)] rows, 32 groups, statistics over the P rows of a batch.  Rounding points, n = 1: the output store
    (norm.hip:261); everything before it is fp32, the variance formed as E[x^2] - mean^2 (norm.hip:150) — the model does the same.
    offset: group means at `offset` standard deviations."""
    g = gen("gn", nb, P, c1, c2, silu, offset, affine)
    ctot, groups = c1 + c2, 32
    x = torch.randn(nb * P, ctot, generator=g)
    x = x + offset if offset else x * (0.5 + torch.rand(1, ctot, generator=g)) + 0.3
    x = x.half()
    gamma, beta = (1 + 0.1 * torch.randn(ctot, generator=g)), 0.1 * torch.randn(ctot, generator=g)
    ins = {"x1": x[:, :c1].contiguous(), "gamma": gamma, "beta": beta}
    if c2:
        ins["x2"] = x[:, c1:].contiguous()
    cpg = ctot // groups

    def ab(cv, kernel_variance):
        xg = cv(x).reshape(nb, P, groups, cpg)
        mean = xg.mean((1, 3))
        if kernel_variance:            # fp32 sums, var = max(E[x^2] - mean^2, 0)
            cnt = float(P * cpg)
            mean = xg.sum((1, 3)) * (1.0 / cnt)
            var = ((xg * xg).sum((1, 3)) * (1.0 / cnt) - mean * mean).clamp_min(0.0)
        else:
            var = xg.var((1, 3), unbiased=False)
        rstd = (var + eps).rsqrt()                                        # [nb, groups]
        a = rstd.repeat_interleave(cpg, 1) * cv(gamma)                    # [nb, ctot]
        bb = cv(beta) - mean.repeat_interleave(cpg, 1) * a
        return a, bb

    def run(ops, i, o):
        if affine:
            ops.group_norm_affine(i["x1"], i["gamma"], i["beta"], nb, groups, eps, out=o["y"])
        else:
            ops.group_norm(i["x1"], i["gamma"], i["beta"], nb, groups, eps, silu, x2=i.get("x2"), out=o["y"])

    def ref():
        a, bb = ab(d, False)
        if affine:
            mean_a = (d(beta) - bb).abs()
            return {"y": (torch.stack([a, bb], -1), torch.stack([a.abs(), mean_a + d(beta).abs()], -1))}
        xr = d(x).reshape(nb, P, ctot)
        y = xr * a[:, None] + bb[:, None]
        sc = (xr * a[:, None]).abs() + bb[:, None].abs()
        if silu:
            y, sc = silu64(y), 1.1 * sc                                   # max |silu'| < 1.1
        return {"y": (y.reshape(nb * P, ctot), sc.reshape(nb * P, ctot))}

    def model():
        a, bb = ab(lambda t: t.float(), True)
        if affine:
            return {"y": torch.stack([a, bb], -1)}
        y = x.float().reshape(nb, P, ctot) * a[:, None] + bb[:, None]
        return {"y": (F.silu(y) if silu else y).reshape(nb * P, ctot).half()}

    out = ((nb, ctot, 2), f32t) if affine else ((nb * P, ctot), f16)
    where = (lambda i: "(batch %d, channel %d, %s)" % (i // (2 * ctot), i // 2 % ctot, "ab"[i % 2])) if affine else oc.loc_rows(ctot)
    case = Case(f"group_norm[{tag}nb{nb},P{P},{c1}+{c2},silu{int(silu)},off{offset},aff{int(affine)}]", ins, {"y": out}, run, ref,
                oc.round_c(1), model, where)
    case.gn = (nb, P, ctot)
    if affine:
        return local_calls(case, [call("group_norm_affine", C=c1, NB=nb, P=P, groups=groups)])
    return local_calls(case, [call("group_norm", C1=c1, C2=c2, NB=nb, P=P, groups=groups, silu=silu, x2=bool(c2))])


GN_THREADS, GN_UNROLL, GN_MAX_SLABS = 256, 4, 2048


def gn_geometry(ctot):
    """norm.hip gn_geometry: (tx channel-vector lanes, vpt vectors per thread = the V of gn_stats_kernel<V> / gn_apply_kernel<V, SILU>,
    ty row lanes)"""
    assert ctot % 8 == 0 and ctot <= 4096
    nvec, vpt = ctot // 8, 1
    while nvec // vpt > GN_THREADS or nvec % vpt:
        vpt += 1
        assert vpt <= 4, ctot
    return nvec // vpt, vpt, GN_THREADS // (nvec // vpt)


def gn_slabs(P, NB, ty, cap_total=GN_MAX_SLABS):
    """norm.hip gn_slabs -> (slabs = grid.x of the statistics and of the apply pass, rows per slab, whether the cap_total / NB clamp bound)"""
    want = max(-(-P // (ty * 4)), 1)
    cap = 1 if NB >= cap_total else cap_total // NB
    slabs = min(want, cap)
    quantum = ty * GN_UNROLL
    rps = -(-(-(-P // slabs)) // quantum) * quantum
    return -(-P // rps), rps, want > cap


# Past one slab per pass.  The existing cases have P <= 10: one slab (two for 1280+640, ty = 1), one partial unrolled iteration.
# Without the clamp a slab is exactly one quantum = ty * GN_UNROLL rows (gn_slabs rounds cdiv(P, slabs) <= quantum up to it), so a
# row lane runs at most one whole unrolled iteration; more than one needs the cap_total / NB clamp to bind.
#  case (nb, P, channels)          geometry (tx, V, ty)   slabs x rows   what it provides
#  2 x 61 x 320                    (40, 1, 6)             3 x 24         three statistics slabs, the last ragged (13 rows): finalize folds 3 partials
#  2 x 61 x 320 affine             (40, 1, 6)             3 x 24         the statistics-only form past one slab (gn_affine_kernel behind 3 partials)
#  2 x 61 x 320 silu0, eps 1e-6    (40, 1, 6)             3 x 24         gn_apply_kernel<1, false> past one slab (the per-frame norm)
#  1 x 11 x 1280+640               (240, 1, 1)            3 x 4          two sources past one slab, the group straddling them; ragged (3 rows)
#  1 x 11 x 1280+1280              (160, 2, 1)            3 x 4          gn_stats_kernel<2> / gn_apply_kernel<2, true> (the 2560-wide skip concatenations), two sources
#  700 x 23 x 1280                 (160, 1, 1)            2 x 12         NB = 700: 2048 / 700 = 2 < the 6 slabs wanted, the clamp binds: 12-row slabs = three whole
#                                                                        unrolled iterations in slab 0, two and a remainder of 3 rows in the ragged slab 1 (11 rows)
#  2 x (2 q + ty + 1) x every other width of GN_WIDTHS   each (tx, V, ty) gn_geometry tells apart at the models' widths, three slabs, the last ragged
# V = 3 needs an odd number of 16-byte vectors above 256 (e.g. 2424 channels), V = 4 none at all below GN_MAX_C: no model width, no forward names them.
GN_WIDTHS = (256, 320, 512, 640, 768, 960, 1024, 1280, 1536, 1920, 2048, 2560)       # block widths and skip concatenations of the base, interpolation and VSR UNets
GN_PAST_SLAB = [dict(nb=2, P=61, c1=320, tag="slabs:"), dict(nb=2, P=61, c1=320, affine=True, tag="slabs:"),
                dict(nb=2, P=61, c1=320, silu=False, eps=1e-6, tag="slabs:"), dict(nb=1, P=11, c1=1280, c2=640, tag="slabs:"),
                dict(nb=1, P=11, c1=1280, c2=1280, tag="slabs:"), dict(nb=700, P=23, c1=1280, tag="clamp:")]
GN_PAST_SLAB += [dict(nb=2, P=2 * 4 * gn_geometry(w)[2] + gn_geometry(w)[2] + 1, c1=w, tag="width:") for w in GN_WIDTHS if w not in (320,)]
# The autoencoder's width: 128 channels = 4 a group, half a 16-byte vector (gn_geometry(128) = (16, 1, 16): 16 row lanes), eps = 1e-6; in no
# list above.  The same P rule: 2 x 145 rows = slabs of 64 / 64 / 17.  silu1: the resnet norms of the decoder's last level; silu0: the
# form of the mid block's attention norm
GN_VAE = [dict(nb=2, P=2 * 4 * gn_geometry(128)[2] + gn_geometry(128)[2] + 1, c1=128, silu=s_, eps=1e-6, tag="vae:") for s_ in (True, False)]
GN_CASES = [dict(nb=1, P=3, c1=64, tag="video:"), dict(nb=2, P=10, c1=320, tag="video:"),
            dict(nb=3, P=5, c1=320, silu=False, eps=1e-6, tag="frame:"), dict(nb=1, P=6, c1=1280, c2=640, tag="straddle:"),
            dict(nb=2, P=10, c1=320, affine=True), dict(nb=2, P=10, c1=320, offset=8.0, tag="offset:")]


@functools.lru_cache(maxsize=None)
def layer_norm_case(M, C, offset=0.0):
    """n = 1: the output store (norm.hip:448); mean and the two-pass variance are fp32 (norm.hip:426-435)."""
    g = gen("ln", M, C, offset)
    x = torch.randn(M, C, generator=g)
    x = (x / x.std(1, keepdim=True) + offset if offset else x * 2 + 0.7).half()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ins = {"x": x, "gamma": gamma, "beta": beta}

    def ab(cv):
        xx = cv(x)
        mean = xx.mean(1, keepdim=True)
        a = ((xx - mean).pow(2).mean(1, keepdim=True) + 1e-5).rsqrt() * cv(gamma)
        return a, mean

    def run(ops, i, o):
        ops.layer_norm(i["x"], i["gamma"], i["beta"], out=o["y"])

    def ref():
        a, mean = ab(d)
        b = d(beta) - mean * a
        return {"y": (d(x) * a + b, (d(x) * a).abs() + b.abs())}

    def model():
        a, mean = ab(lambda t: t.float())
        return {"y": ((x.float() - mean) * a + beta).half()}

    return Case(f"layer_norm[{M}x{C},off{offset}]", ins, {"y": ((M, C), f16)}, run, ref, oc.round_c(1), model, oc.loc_rows(C))


LN_CASES = [(1, 320, 0.0), (5, 256, 0.0), (65, 1280, 0.0), (5, 320, 8.0)]


# ------------------------------------------------------------------ attention
LOG2E = 1.4426950408889634


def attn_model(q, k, v, scale, n_q_round):
    """[..., lq, dh] x [..., lk, dh]: the kernels' arithmetic in torch fp32 — Q scaled by scale log2(e) and rounded to fp16 where the
    kernel does that, exp2 of the shifted scores, P rounded to fp16 before the PV product, the row sum taken over the rounded P
    (the matrix pipe sums it as an extra V column), one rounding at the store."""
    qs = (q.float() * (scale * LOG2E))
    if n_q_round:
        qs = qs.half().float()
    s = qs @ k.float().transpose(-1, -2)
    p = torch.exp2(s - s.max(-1, keepdim=True).values).half().float()
    return ((p @ v.float()) / p.sum(-1, keepdim=True)).half()


def attn_ref(q, k, v, scale):
    p = torch.softmax(d(q) @ d(k).transpose(-1, -2) * scale, -1)
    return p @ d(v), p @ d(v).abs()


def split_heads(t, nb, heads):
    return t.reshape(nb, -1, heads, t.shape[-1] // heads).permute(0, 2, 1, 3)


def merge_heads(t):
    nb, heads, l, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(nb * l, heads * dh)


def attention_route(dh, lq, lk, sc=False):
    """The instantiation launch_attention picks (attention.hip: att_route, the one function that decides, and ATT_TABLE), as
    a name: what the comment tables below and test_opcheck_host.py::test_attention_cases_reach_every_instantiation go by, and what
    decides whether the model rounds Q' (only the V2 softmax does: the Q' scaling in attention_dma_kernel).  lk = the keys a query sees."""
    if dh in (256, 512):
        return "wide"                                                   # att_route: ATT_WIDE -> attention_wide.hip
    qt = 2 if lq > 64 * 3 else 1                                        # att_route: qt
    tag = ",sc" if sc else ""
    nch = {40: 5, 80: 10, 160: 20}.get(dh) or (None if sc else {32: 4, 64: 8, 128: 16}.get(dh))      # att_route: the LDS-DMA head dims
    if nch:
        short_keys = nch == 5 and lk <= 2 * 64                          # att_route: short_keys
        if nch == 5 and qt == 2 and not short_keys and lq % 256 == 0:   # att_route: nw
            return f"dma<{nch},QT2,V2,8 waves{tag}>"
        v2 = nch <= 10 and not short_keys                               # att_route: v2
        return f"dma<{nch},QT{qt},{'V2' if v2 else 'round-3'},4 waves{tag}>"
    lsum = dh % 16 != 0                                                 # att_route: the register-staged kernels' LSUM
    dhp = 64 if dh <= 64 else 96 if dh <= 96 else 160                   # att_route: dhp
    ndt = ",NDT4" if dh == 64 else ""                                   # att_route: NDT (sparse-causal only: plain dh 64 is on the DMA kernel)
    return f"reg<{dhp},QT{qt},{'lsum' if lsum else 'sum'}{ndt}{tag}>"


def route_kernel(route, dh):
    """The kernel name the launch stub records for a route name: the row of attention.hip's ATT_TABLE that att_route's result selects."""
    if route == "wide":
        return f"attention_wide_kernel<{dh}>"
    kind, args = route[:-1].split("<")
    args = args.split(",")
    sc = "true" if args[-1] == "sc" else "false"
    if kind == "dma":
        nch, qt, v2, nw = int(args[0]), args[1][2:], "true" if args[2] == "V2" else "false", args[3].split()[0]
        return f"attention_dma_kernel<{nch}, {qt}, {2 if nch >= 16 else 3}, {'true' if nch == 5 else 'false'}, {sc}, {v2}, {nw}>"
    return f"attention_kernel<{args[0]}, {args[1][2:]}, {'true' if args[2] == 'lsum' else 'false'}, {sc}, {4 if 'NDT4' in args else 0}>"


def rounds_q(dh, lq, lk, sc=False):
    return "V2" in attention_route(dh, lq, lk, sc)


# Every instantiation ops.attention / ops.sparse_causal_attention can reach, at QT 1 and QT 2 where the plain kernels have both and
# at one of them for the sparse-causal twins off the interpolation model's head dims (40).  Not reachable, so not listed:
# attention_kernel<64, *, false, false, 4> (att_route's NDT without SC: plain head dim 64 is among the LDS-DMA head dims) and
# dma<5,QT2,round-3,sc> (QT 2 needs lq > 192, sparse-causal has lk = 2 lq, short_keys needs lk <= 128).
ATT_ROUTES = ([f"dma<{n},QT{qt},V2,4 waves>" for n in (4, 5, 8, 10) for qt in (1, 2)] + ["dma<5,QT2,V2,8 waves>"]
              + [f"dma<{n},QT{qt},round-3,4 waves>" for n in (5, 16, 20) for qt in (1, 2)]
              + [f"reg<{dp},QT{qt},{sm}>" for dp, sm in ((64, "lsum"), (64, "sum"), (96, "lsum"), (96, "sum"), (160, "sum")) for qt in (1, 2)]
              + [f"dma<5,QT{qt},V2,4 waves,sc>" for qt in (1, 2)] + ["dma<5,QT2,V2,8 waves,sc>", "dma<5,QT1,round-3,4 waves,sc>",
                                                                     "dma<10,QT1,V2,4 waves,sc>", "dma<20,QT1,round-3,4 waves,sc>"]
              + [f"reg<64,QT{qt},sum,NDT4,sc>" for qt in (1, 2)]
              + [f"reg<{dp},QT1,{sm},sc>" for dp, sm in ((64, "lsum"), (64, "sum"), (96, "lsum"), (96, "sum"), (160, "sum"))] + ["wide"])

PROFILES = ["far_below", "dominant_last", "creep", "mixed_wave"]


def key_tile(dh):
    """keys per tile of the kernel that serves head dim dh: attention_wide.hip AW_KEYS = 32 at 256 / 512, attention.hip's 64 below"""
    return 32 if dh in (256, 512) else 64


def profile_applies(profile, lq, lk, tile=64):
    """lk: the keys of one key sequence that can be placed freely (sparse-causal: the d tokens of a frame); tile: keys per key tile."""
    if profile == "far_below":
        return lk > tile                     # a whole first key tile below, the matching key behind it
    if profile == "creep":
        return lk > 2 * tile                 # three key tiles
    if profile == "mixed_wave":
        return lk > tile + 1 and lq >= 32    # its matching key is lk - 2 (lk - 1 is the dominant one) and must lie behind the first tile
    return lk >= 2


def hard_rows(lq):
    """Row 0, row lq - 1 and up to two rows between them, each in a 16-row group of its own (= other waves / query tiles)."""
    groups = -(-lq // 16)
    rows = {0, lq - 1}
    for grp in (1, groups // 2):
        if 0 < grp < (lq - 1) // 16:
            rows.add(16 * grp + 5)
    return sorted(rows)


MIXED_ROWS = (18, 27)        # mixed_wave: (the dominant_last row, the far_below row), both in the 16-row group 1


def apply_profile(profile, g, q, k, dh, qsrc, first64, tile=64):
    """Rewrites rows of q [nbq, lq, c] and k [nbk, lk, c] in place (heads packed along c).  qsrc[b]: the query batch entry whose
    rows the dominant keys of key batch entry b are copied from; first64: the key batch entries whose keys 0..tile-1 are the first
    tile of a query; tile: keys per key tile of the kernel (64, the default, leaves every older case its inputs bit for bit; 32 for
    attention_wide.hip).  Every constant is exact in fp16.  Returns what the case asserts on: far / creep rows (in every batch entry),
    (key batch, row, key) triples of the dominant keys, and the index from the end of the key that matches a far_below row."""
    lq, lk, c = q.shape[1], k.shape[1], q.shape[2]
    u = (torch.randint(0, 2, (c,), generator=g) * 2 - 1).to(f16)           # one sign vector per head, side by side
    hard = {"far": [], "dom": [], "creep": [], "match": 1}
    rows = hard_rows(lq)

    def far_below(rs, match):
        for b in first64:
            k[b, :tile] = (-1.25 * u.float() + 0.1 * torch.randn(tile, c, generator=g)).half()
        k[:, lk - match] = u
        # first-tile logits -20 sqrt(dh) nats (-25 sqrt(dh) below head dim 32, where -20 sqrt(dh) is above -100) as 16 x -1.25, not
        # 4 x -5: a key of magnitude 5 multiplies the rounding of Q' in the logits of the UNIT rows that see it, and the fp32 model
        # of sparse_causal[f2,d65,c320,far_below] then missed the bound at one element of a unit row (3.482e-03 > 3.457e-03)
        q[:, rs] = (16 if dh >= 32 else 20) * u
        hard["far"], hard["match"] = list(rs), match

    def dominant(pairs):
        for r, key in pairs:
            for b in range(k.shape[0]):
                k[b, key] = 3 * q[qsrc[b], r]
            hard["dom"].append((r, key))

    if profile == "far_below":
        far_below(rows, 1)
    elif profile == "dominant_last":
        dominant([(rows[-1], lk - 1), (rows[0], lk - 2)])
    elif profile == "creep":
        s = torch.tensor(5 / (math.sqrt(dh) * LOG2E)).half()
        q[:, rows] = u
        for t in range(-(-lk // tile)):
            k[:, min(tile * t + 3, lk - 1)] = ((t + 1) * s.float() * u.float()).half()
        hard["creep"] = rows
    elif profile == "mixed_wave":
        far_below([MIXED_ROWS[1]], 2)
        # the dominant row loses its component along u (per head) first: its key 3 q[r] then scores ~0 for the far_below row, whose
        # logits are 16 x those of a unit row — against a random 3 q[r] they reach the matching key's, and the rounding of Q'
        # (2^-12 of a logit of ~130 log2 units) then decides between two keys: the fp32 model missed the bound there at head dim 32
        qd = q[:, MIXED_ROWS[0]].float().view(-1, c // dh, dh)
        uu = u.float().view(c // dh, dh)
        q[:, MIXED_ROWS[0]] = (qd - (qd * uu).sum(-1, keepdim=True) / dh * uu).view(-1, c).half()
        dominant([(MIXED_ROWS[0], lk - 1)])
    else:
        raise ValueError(profile)
    return hard


def assert_profile(hard, qh, kh, scale, dom_batches, creep_tiles, key0=0, tile=64):
    """float64, on the values the kernel gets: qh [nb, heads, lq, dh], kh [nb, heads, keys, dh] as a query sees them; dom_batches:
    the query batch entries whose rows the dominant keys were copied from; key0: where the key sequence apply_profile wrote to
    starts among the keys a query sees (sparse-causal: the previous-frame half); tile: keys per key tile, as apply_profile got it."""
    s = d(qh) @ d(kh).transpose(-1, -2) * scale                             # nats
    if hard["far"]:
        first, match = s[:, :, hard["far"], :tile], s[:, :, hard["far"], s.shape[-1] - hard["match"]]
        assert first.max() < -100 and match.min() > 0, (first.max().item(), match.min().item())
    for r, key in hard["dom"]:
        row = s[dom_batches, :, r]
        rest = row.clone()
        rest[..., [kk + o for _, kk in hard["dom"] for o in (0, key0)]] = -math.inf
        assert (row[..., key0 + key] - rest.max(-1).values).min() > 0, (r, key)      # it is the row's maximum
    if hard["creep"]:
        tiles = F.pad(s[:, :, hard["creep"], :tile * creep_tiles], (0, max(tile * creep_tiles - s.shape[-1], 0)), value=-math.inf)
        tiles = tiles.reshape(*s.shape[:2], len(hard["creep"]), creep_tiles, tile).max(-1).values * LOG2E     # best score per key tile
        step = tiles[..., 1:] - tiles[..., :-1]
        assert step.min() > 3.0 and step.max() < 8.0 and (tiles[..., -1] - tiles[..., 0]).min() > 8.0, (step.min().item(), step.max().item())


@functools.lru_cache(maxsize=None)
def attention_case(nb, lq, c, lk=None, kv_div=1, heads=8, profile="unit", tile=64):
    """ops.attention on column slices of wider tensors whose other columns are NaN.  Self-attention (lk None): q | k | v are the
    thirds of one [nb*lq, 3c + 16] tensor; cross-attention: k | v are halves of a [(nb / kv_div) lk, 2c + 16] tensor.
    Rounding points: n = 3 at head dims up to 160 — Q' = fp16(Q scale log2 e) (attention_dma_kernel's `if constexpr (V2)` after
    the Q load), P before the PV product (att_pack4 in attention_frag.h, for every kernel; the register-staged kernel has no Q'
    rounding), the output store (the normalise-and-store epilogue of both kernels); n = 2 at head dims 256 / 512 (att_pack4 and
    attention_wide_kernel's epilogue).  The round-3 softmax of the DMA kernel (the else arm of its `if constexpr (V2)`, P through
    att_pack4 as well) has no Q' rounding either: the model rounds Q' where attention_route says V2; the bound
    is round_c(3) for all of them.
    profile: "unit" = N(0, 1) operands; the others (PROFILES, apply_profile) rewrite a few query rows and keys of those, laid out for
    key tiles of `tile` keys (key_tile(dh) for the cases past one workgroup; the older wide cases keep 64 = two of that kernel's tiles)."""
    g = gen("attn", nb, lq, c, lk, kv_div, heads)
    dh = c // heads
    wide = dh > 160
    cross = lk is not None
    lk_ = lk if cross else lq
    nkv = nb // kv_div
    q, k, v = rnd(g, nb * lq, c), rnd(g, nkv * lk_, c), rnd(g, nkv * lk_, c)
    hard = None
    if profile != "unit":
        assert profile_applies(profile, lq, lk_, tile), (profile, lq, lk_, tile)
        hard = apply_profile(profile, gen("attn-profile", nb, lq, c, lk, kv_div, heads, profile), q.view(nb, lq, c), k.view(nkv, lk_, c),
                             dh, [b * kv_div for b in range(nkv)], range(nkv), tile)
    nan = lambda r, w: torch.full((r, w), math.nan, dtype=f16)
    if cross:
        ins = {"qw": torch.cat([nan(nb * lq, 8), q, nan(nb * lq, 8)], 1), "kvw": torch.cat([k, nan(nkv * lk_, 16), v], 1)}
    else:
        ins = {"qkvw": torch.cat([q, nan(nb * lq, 8), k, nan(nb * lq, 8), v], 1)}

    def run(ops, i, o):
        if cross:
            qd, kd, vd = i["qw"][:, 8:8 + c], i["kvw"][:, :c], i["kvw"][:, c + 16:]
        else:
            qd, kd, vd = i["qkvw"][:, :c], i["qkvw"][:, c + 8:2 * c + 8], i["qkvw"][:, 2 * c + 16:]
        ops.attention(qd, kd, vd, nb=nb, lq=lq, lk=lk_, heads=heads, kv_batch_div=kv_div, out=o["y"])

    def heads_of():
        rep = lambda t: split_heads(t.reshape(nkv, lk_, c), nkv, heads).repeat_interleave(kv_div, 0)
        return split_heads(q.reshape(nb, lq, c), nb, heads), rep(k), rep(v)

    if hard:
        qh, kh, _ = heads_of()
        assert_profile(hard, qh, kh, dh ** -0.5, [b * kv_div for b in range(nkv)], -(-lk_ // tile), tile=tile)

    def ref():
        y, sc = attn_ref(*heads_of(), dh ** -0.5)
        return {"y": (merge_heads(y), merge_heads(sc))}

    name = f"attention[nb{nb},lq{lq},lk{lk},c{c},h{heads},div{kv_div}" + ("]" if profile == "unit" else f",{profile}]")
    case = Case(name, ins, {"y": ((nb * lq, c), f16)}, run, ref, oc.round_c(2 if wide else 3),
                lambda: {"y": merge_heads(attn_model(*heads_of(), dh ** -0.5, rounds_q(dh, lq, lk_)))}, oc.loc_heads(heads, dh))
    case.route = attention_route(dh, lq, lk_)
    case.hard = hard
    # the launch is replayed (`hostcheck optrace`): the kernel must be the one the route names (test_opcheck_host.py), the wide
    # kernel's grid what wide_walk mirrors
    wq, wkv = (c + 16, 2 * c + 16) if cross else (3 * c + 16, 3 * c + 16)
    return local_calls(case, [call("attention", ldq=wq, ldk=wkv, ldv=wkv, ldo=c, NB=nb, Lq=lq, Lk=lk_, heads=heads, dh=dh, kv_batch_div=kv_div)])


SELF_ATTN = [(1, 1, 256), (2, 33, 320), (1, 65, 320), (1, 129, 1280)]
CROSS_ATTN = [(lk, div) for lk in (1, 10, 77) for div in (1, 3)]
WIDE_ATTN = [(1, 512), (33, 512), (65, 512), (33, 256)]

# The smallest shape that reaches each instantiation, 8 heads; run under every profile that applies (profile_applies).
# All decided in attention.hip's att_route: QT 2 from lq = 193 (qt), the 8-wave kernel at lq % 256 == 0 (nw), V2 at head dim 40
# from lk = 129 (short_keys).
# (nb, lq, c)              head dim   instantiation (attention_route)
SELF_HARD = [
    (1, 129, 320),       # 40         dma<5,QT1,V2,4 waves>   three key tiles, the last holding one key
    (1, 193, 320),       # 40         dma<5,QT2,V2,4 waves>
    (2, 256, 320),       # 40         dma<5,QT2,V2,8 waves>
    (1, 65, 640),        # 80         dma<10,QT1,V2,4 waves>  (every key count: short_keys is head dim 40's)
    (1, 193, 640),       # 80         dma<10,QT2,V2,4 waves>
    (1, 129, 256),       # 32         dma<4,QT1,V2,4 waves>
    (1, 193, 256),       # 32         dma<4,QT2,V2,4 waves>
    (1, 129, 512),       # 64         dma<8,QT1,V2,4 waves>
    (1, 193, 512),       # 64         dma<8,QT2,V2,4 waves>
    (1, 129, 1024),      # 128        dma<16,QT1,round-3,4 waves>
    (1, 193, 1024),      # 128        dma<16,QT2,round-3,4 waves>
    (1, 129, 1280),      # 160        dma<20,QT1,round-3,4 waves>   (its unit case is SELF_ATTN's)
    (1, 193, 1280),      # 160        dma<20,QT2,round-3,4 waves>
    (1, 65, 192),        # 24         reg<64,QT1,lsum>
    (1, 193, 192),       # 24         reg<64,QT2,lsum>
    (1, 65, 384),        # 48         reg<64,QT1,sum>
    (1, 193, 384),       # 48         reg<64,QT2,sum>
    (1, 65, 576),        # 72         reg<96,QT1,lsum>
    (1, 193, 576),       # 72         reg<96,QT2,lsum>   (not in the issue's list: the QT 2 form of the one above)
    (1, 65, 768),        # 96         reg<96,QT1,sum>
    (1, 193, 768),       # 96         reg<96,QT2,sum>
    (1, 65, 1152),       # 144        reg<160,QT1,sum>
    (1, 193, 1152),      # 144        reg<160,QT2,sum>   (not in the issue's list: the QT 2 form of the one above)
]
# (nb, lq, lk, c, kv_div)
CROSS_HARD = [
    (3, 40, 128, 320, 1), (3, 40, 128, 320, 3),     # 40   dma<5,QT1,round-3,4 waves>: lk = 2 * 64 is still short_keys
    (3, 40, 129, 320, 1), (3, 40, 129, 320, 3),     # 40   dma<5,QT1,V2,4 waves>: one key past it
    (3, 193, 77, 320, 3),                           # 40   dma<5,QT2,round-3,4 waves>: short_keys wins over QT 2 and 8 waves
    (3, 40, 77, 640, 3),                            # 80   dma<10,QT1,V2,4 waves>: V2 at 77 keys
    (1, 129, 321, 320, 1), (1, 129, 321, 640, 1),   # 40 / 80  V2, six key tiles: `creep` passes the rescale threshold twice
]
# (lq = lk, c), one head: attention_wide.hip (32-key tiles, AW_KEYS; a running maximum that is always finite).  These two keep the
# profiles laid out for 64 keys = two of its tiles; WIDE_PAST below lays them out for its own tile
WIDE_HARD = [(65, 512), (33, 256)]

# attention_wide.hip past one workgroup and past three key tiles.  A workgroup holds AW_QBLK = 128 queries as 4 waves x 2 query tiles
# of 16; the grid is nqblk x heads x nb workgroups, renumbered so that blockIdx % 8 (one XCD) takes a contiguous run (wide_walk); K and
# V each have a ring of two 32-key tiles, refilled with tile t + 2 / t + 1 while tile t is computed.  Profiles at key_tile = 32.
# (nb, lq, lk or None = lq, c, heads, kv_div)   what it provides
WIDE_PAST = [
    (1, 161, None, 512, 1, 1),     # two query blocks: block 0 with all four waves full, block 1 with one query (wave 0, query tile 0, every other
                                   # lane clamped); six key tiles: each K slot and each V slot refilled at least twice, the last tile holding one key
    (1, 161, None, 256, 1, 1),     # the same at head dim 256 (KPP = 2, PIECES = 4 against 1 and 8)
    (3, 129, None, 1024, 2, 1),    # nwg = 2 x 2 x 3 = 12: xq = 1, xr = 4 in the renumbering (workgroups with blockIdx % 8 >= xr); two heads, three batch entries
    (4, 40, 97, 512, 1, 2),        # cross form, lk != lq, kv_batch_div = 2; four key tiles, the last holding one key
]
WIDE_QBLK = 128


def wide_walk(nwg, nqblk, heads):
    """attention_wide_kernel's "workgroup order" block: (batch entry, head, query block) of each blockIdx.  blockIdx % 8 labels the workgroups of one XCD;
    label x takes a contiguous run of the list ordered (batch, head, query block), query block fastest — xq + 1 entries for the
    first xr = nwg % 8 labels, xq = nwg / 8 for the others."""
    xq, xr = nwg >> 3, nwg & 7
    out = []
    for bid in range(nwg):
        x = bid & 7
        w = (x * (xq + 1) if x < xr else xr * (xq + 1) + (x - xr) * xq) + (bid >> 3)
        bh = w // nqblk
        out.append((bh // heads, bh % heads, w % nqblk))
    return out


def wide_case_walk(case):
    """(walk, key tiles) of a wide attention case from the integers of its call"""
    a = case.calls[0][1]
    nqblk = -(-a["Lq"] // WIDE_QBLK)
    return wide_walk(nqblk * a["heads"] * a["NB"], nqblk, a["heads"]), -(-a["Lk"] // 32)


def with_profiles(shapes, lq_of, lk_of, have_unit=()):
    """shapes x the profiles that apply; "unit" too, unless the shape already has its unit case in the lists above"""
    return [(s, p) for s in shapes for p in ["unit"] + PROFILES
            if (s not in have_unit if p == "unit" else profile_applies(p, lq_of(s), lk_of(s)))]


SELF_HARD_CASES = with_profiles(SELF_HARD, lambda s: s[1], lambda s: s[1], SELF_ATTN)
CROSS_HARD_CASES = with_profiles(CROSS_HARD, lambda s: s[1], lambda s: s[2])
WIDE_HARD_CASES = with_profiles(WIDE_HARD, lambda s: s[0], lambda s: s[0], WIDE_ATTN)
WIDE_PAST_CASES = [(s, p) for s in WIDE_PAST for p in ["unit"] + PROFILES if p == "unit" or profile_applies(p, s[1], s[2] or s[1], 32)]


def wide_past_cases():
    return [attention_case(nb, lq, c, lk=lk, kv_div=div, heads=heads, profile=p, tile=key_tile(c // heads))
            for (nb, lq, lk, c, heads, div), p in WIDE_PAST_CASES]


@functools.lru_cache(maxsize=None)
def sparse_causal_case(frames, dd, c=320, heads=8, videos=2, profile="unit"):
    """Frame f attends to [frame 0 || frame max(f - 1, 0)] of its video; same kernels and rounding points as attention_case (n = 3).
    Profiles are laid out in token space: the far-below keys are the first 64 tokens of frame 0, the matching / dominant keys the
    last tokens of every frame (= the end of the previous-frame half), the dominant ones copied from the rows of the frame that
    sees them there.  With two frames both halves of the key sequence are frame 0, so `creep` climbs over the tiles of the first
    half only (it needs three: d > 128) and the second half repeats it from below."""
    g = gen("sc", frames, dd, c)
    nb, dh = videos * frames, c // heads
    qkv = rnd(g, nb * dd, 3 * c)
    prev = torch.tensor([vi * frames + (0, max(fi - 1, 0))[j] for vi in range(videos) for fi in range(frames) for j in (0, 1)])
    hard = None
    if profile != "unit":
        assert profile_applies(profile, dd, dd), (profile, dd)
        q, k = (qkv.view(nb, dd, 3 * c)[:, :, i * c:(i + 1) * c] for i in (0, 1))
        nxt = [vi * frames + min(fi + 1, frames - 1) for vi in range(videos) for fi in range(frames)]
        hard = apply_profile(profile, gen("sc-profile", frames, dd, c, heads, videos, profile), q, k, dh, nxt,
                             [vi * frames for vi in range(videos)])
    ins = {"qkv": qkv}

    def run(ops, i, o):
        t = i["qkv"]
        ops.sparse_causal_attention(t[:, :c], t[:, c:2 * c], t[:, 2 * c:], nb, frames, dd, heads, out=o["y"])

    def heads_of():
        q, k, v = (t.reshape(nb, dd, c) for t in qkv.split(c, 1))
        kk, vv = (t[prev].reshape(nb, 2 * dd, c) for t in (k, v))
        return split_heads(q, nb, heads), split_heads(kk, nb, heads), split_heads(vv, nb, heads)

    if hard:
        qh, kh, _ = heads_of()
        # a dominant key is copied from the frame after its own: the rows of that frame see it at the end of their second half
        seen_by = [b for b in range(nb) if nxt[int(prev[2 * b + 1])] == b]
        assert_profile(hard, qh, kh, dh ** -0.5, seen_by, -(-dd // 64), key0=dd)

    def ref():
        y, sc = attn_ref(*heads_of(), dh ** -0.5)
        return {"y": (merge_heads(y), merge_heads(sc))}

    name = f"sparse_causal[f{frames},d{dd}]" if (c, profile) == (320, "unit") else f"sparse_causal[f{frames},d{dd},c{c},{profile}]"
    case = Case(name, ins, {"y": ((nb * dd, c), f16)}, run, ref, oc.round_c(3),
                lambda: {"y": merge_heads(attn_model(*heads_of(), dh ** -0.5, rounds_q(dh, dd, 2 * dd, True)))}, oc.loc_heads(heads, dh))
    case.route = attention_route(dh, dd, 2 * dd, True)
    case.hard = hard
    return local_calls(case, [call("sparse_causal_attention", ldq=3 * c, ldk=3 * c, ldv=3 * c, ldo=c, NB=nb, frames=frames, D=dd, heads=heads, dh=dh)])


SPARSE_CAUSAL = [(1, 5), (3, 5), (2, 65)]
# (frames, d, c)           head dim   instantiation                                   decided at
SC_HARD = [
    (2, 65, 320),        # 40         dma<5,QT1,V2,4 waves,sc>  (130 keys; (1, 5) and (3, 5) above: round-3, 10 keys)
    (2, 193, 320),       # 40         dma<5,QT2,V2,4 waves,sc>
    (2, 256, 320),       # 40         dma<5,QT2,V2,8 waves,sc>
    (2, 65, 640),        # 80         dma<10,QT1,V2,4 waves,sc>
    (2, 65, 1280),       # 160        dma<20,QT1,round-3,4 waves,sc>
    (2, 65, 512),        # 64         reg<64,QT1,sum,NDT4,sc>   (ATT_TABLE has no sparse-causal DMA row at head dim 64)
    (2, 193, 512),       # 64         reg<64,QT2,sum,NDT4,sc>
    # not in the issue's list: the sparse-causal twins of the register-staged instantiations, which dispatch_att<true> selects
    # for head dims the interpolation model does not have (24, 48, 72, 96, 128)
    (2, 65, 192),        # 24         reg<64,QT1,lsum,sc>
    (2, 65, 384),        # 48         reg<64,QT1,sum,sc>
    (2, 65, 576),        # 72         reg<96,QT1,lsum,sc>
    (2, 65, 768),        # 96         reg<96,QT1,sum,sc>
    (2, 65, 1024),       # 128        reg<160,QT1,sum,sc>
]
SC_HARD_CASES = with_profiles(SC_HARD, lambda s: s[1], lambda s: s[1], [(f, dd, 320) for f, dd in SPARSE_CAUSAL])


def attention_hard_cases():
    cs = [attention_case(*s, profile=p) for s, p in SELF_HARD_CASES]
    cs += [attention_case(nb, lq, c, lk=lk, kv_div=div, profile=p) for (nb, lq, lk, c, div), p in CROSS_HARD_CASES]
    cs += [attention_case(1, l, c, heads=1, profile=p) for (l, c), p in WIDE_HARD_CASES]
    cs += [sparse_causal_case(f, dd, c=c, profile=p) for (f, dd, c), p in SC_HARD_CASES]
    return cs


# ------------------------------------------------------------------ temporal attention and the row-resident fused blocks
def h_(t):
    """one fp16 rounding point of a model"""
    return t.half().float()


def ident(t):
    return t


def rotary_tables(frames, rot_dim=32):
    inv = 10000.0 ** (-torch.arange(0, rot_dim, 2, dtype=f32t) / rot_dim)
    ang = torch.arange(frames, dtype=f32t).reshape(-1, 1) * inv.reshape(1, -1)
    return ang.cos().contiguous(), ang.sin().contiguous()


def rot(t, cos, sin):
    """rotary embedding on channel pairs (2k, 2k + 1) of the first 2 * cos.shape[1] head dims; t [..., f, dh]"""
    r = 2 * cos.shape[1]
    e, o = t[..., 0:r:2], t[..., 1:r:2]
    out = t.clone()
    out[..., 0:r:2] = e * cos - o * sin
    out[..., 1:r:2] = o * cos + e * sin
    return out


def temporal_core(q, k, v, bias, cos, sin, scale, cv, rq, p_before_norm):
    """[N, heads, f, dh] sequences: softmax(rot(q scale) rot(k)^T + bias) v.  rq = rounding applied where the kernels round
    (identity for the float64 reference); p_before_norm: the fused block rounds exp() and normalises the product,
    the standalone kernels round the normalised P.  Returns (out, sum_j p_j |v_j|)."""
    q, k, v = cv(q) * scale, cv(k), cv(v)
    if cos is not None:
        q, k = rot(q, cv(cos), cv(sin)), rot(k, cv(cos), cv(sin))
    s = rq(q) @ rq(k).transpose(-1, -2) + cv(bias)[None]
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    if p_before_norm:
        return (rq(e) @ v) / l, (e / l) @ v.abs()
    return rq(e / l) @ v, (e / l) @ v.abs()


def temporal_route(b, f, d, heads, dh, budget=0):
    """What launch_temporal_attention launches (temporal_attention.hip, the launcher at the end of the file), as the stub names it,
    with its grid and how the work is dealt: for the streaming kernel `ngroups` head groups, `per_group` workgroups per group walking
    `tiles` (video, pixel) tiles at stride per_group, and the tile count of the fullest and the emptiest workgroup; for the tile kernel
    the heads HG and pixels PT of a workgroup.  budget: lavie_debug_temporal_budget (0 = automatic)."""
    nt = 1 if -(-f // 16) <= 1 else 4
    fp, cw = 16 * nt, heads * dh
    wide, narrow = (320, 256) if nt == 1 else (160, 128)
    srl = wide if cw % wide == 0 and wide % dh == 0 else narrow if cw % narrow == 0 and narrow % dh == 0 else 0
    if budget == 0 and srl and srl // dh <= 8:
        pack2 = nt == 1 and f <= 8 and d % 2 == 0
        ngroups = cw // srl
        tiles = b * (d // 2 if pack2 else d)
        per_group = min(max((512 if nt == 1 else 256) // ngroups, 1), tiles)
        counts = [len(range(t0, tiles, per_group)) for t0 in range(per_group)]
        return dict(kernel=f"temporal_stream_kernel<{nt}, {srl}, {2 if pack2 else 1}>", grid=(per_group * ngroups, 1, 1), ngroups=ngroups,
                    per_group=per_group, tiles=tiles, fullest=max(counts), emptiest=min(counts), heads_per_group=srl // dh)

    def row_stride(hg):
        rs = hg * dh * 2 + 32
        return rs + 32 if (rs // 32) % 2 == 0 else rs
    want = budget if budget > 0 else (33000 if nt == 1 else 70000)
    room = max(want, 3 * fp * 256)
    hg = heads
    while hg > 2 and hg % 2 == 0 and 3 * fp * row_stride(hg) > room:
        hg //= 2
    pt = min(max(room // (3 * fp * row_stride(hg)), 1), 4)
    return dict(kernel=f"temporal_attention_kernel<{nt}>", grid=(b * -(-d // pt) * (heads // hg), 1, 1), HG=hg, PT=pt,
                lds=3 * pt * fp * row_stride(hg))


# everything launch_temporal_attention can launch (cross-checked against `hostcheck kernels` by test_gemm_reach_host.py)
TATTN_ROUTES = ([f"temporal_stream_kernel<1, {w}, {p}>" for w in (320, 256) for p in (1, 2)] + [f"temporal_stream_kernel<4, {w}, 1>" for w in (160, 128)]
                + ["temporal_attention_kernel<1>", "temporal_attention_kernel<4>"])


def peaked_rows(f):
    """one query frame per 16-frame block (the 16-row blocks of the kernels' score tiles): frame 5 of the block, or the last frame"""
    return sorted({min(16 * blk + 5, f - 1) for blk in range(-(-f // 16))})


def peak_bias(bias, f):
    """the `peaked` profile: + 48 on the bias of (query frame, last frame) for the frames of peaked_rows, every head.  48 is exact in
    fp32 next to a bias of N(0, 1) to 2^-18; the scores of N(0, 1) operands stay within a few nats."""
    for r in peaked_rows(f):
        bias[:, r, f - 1] += 48.0
    return bias


def assert_peaked(q, k, bias, cos, sin, scale, f):
    """float64, on the values the kernel gets: in the rows of peaked_rows the last frame's logit is more than 30 nats above every other"""
    q, k = d(q) * scale, d(k)
    if cos is not None:
        q, k = rot(q, d(cos), d(sin)), rot(k, d(cos), d(sin))
    s = q @ k.transpose(-1, -2) + d(bias)[None]
    rows = peaked_rows(f)
    if f > 1:
        margin = s[..., rows, f - 1] - s[..., rows, :f - 1].max(-1).values
        assert margin.min() > 30.0, margin.min().item()
    others = [r for r in range(f) if r not in rows]
    if others and f > 1:
        top2 = s[..., others, :].topk(2, -1).values
        assert (top2[..., 0] - top2[..., 1]).median() < 10.0          # the other rows are ordinary


@functools.lru_cache(maxsize=None)
def temporal_attention_case(b, f, dd, c, tiled, plain=False, heads=8, profile="unit"):
    """ops.temporal_attention on qkv [(b f d), 3c].  Rounding points, n = 4: q scaled (and rotated) to fp16
    (temporal_attention.hip:162-163 / :169; tiled kernel :472-473 / :477), k rotated to fp16 (:164-165; :440-441), the normalised P
    (:216; :517), the output (:238; :539).  tiled: the tile kernel through lavie_debug_temporal_budget (True = 33000 bytes, or the
    budget itself), else whatever the launcher picks (temporal_route).  profile "peaked": peak_bias."""
    g = gen("tattn", b, f, dd, c, plain)
    dh = c // heads
    budget = 33000 if tiled is True else int(tiled)
    qkv = rnd(g, b * f * dd, 3 * c)
    bias = torch.zeros(heads, f, f) if plain else rnd(g, heads, f, f, dtype=f32t)
    if profile == "peaked":
        bias = peak_bias(bias, f)
    cos, sin = (None, None) if plain else rotary_tables(f)
    ins = {"qkv": qkv, "bias": bias}
    if not plain:
        ins.update(cos=cos, sin=sin)

    def run(ops, i, o):
        from lavie_amd import _lib
        lib = _lib.load()
        lib.lavie_debug_temporal_budget(budget)
        try:
            ops.temporal_attention(i["qkv"], b, f, dd, heads, i["bias"], i.get("cos"), i.get("sin"), rot_dim=0 if plain else 32, out=o["y"])
        finally:
            lib.lavie_debug_temporal_budget(0)

    seq = lambda: qkv.reshape(b, f, dd, 3, heads, dh).permute(3, 0, 2, 4, 1, 5).reshape(3, b * dd, heads, f, dh)
    back = lambda t: t.reshape(b, dd, heads, f, dh).permute(0, 3, 1, 2, 4).reshape(b * f * dd, c)
    if profile == "peaked":
        qs, ks, _ = seq()
        assert_peaked(qs, ks, bias, cos, sin, dh ** -0.5, f)

    def ref():
        y, sc = temporal_core(*seq(), bias, cos, sin, dh ** -0.5, d, ident, False)
        return {"y": (back(y), back(sc))}

    def model():
        y, _ = temporal_core(*seq(), bias, cos, sin, dh ** -0.5, lambda t: t.float(), h_, False)
        return {"y": back(y).half()}

    mode = "stream" if not budget else "tiled" if budget == 33000 else f"tiled{budget}"
    name = f"temporal_attention[b{b},f{f},d{dd},c{c},{mode},plain{int(plain)}" + (f",h{heads}" if heads != 8 else "") + ("]" if profile == "unit" else f",{profile}]")
    case = Case(name, ins, {"y": ((b * f * dd, c), f16)}, run, ref, oc.round_c(4), model, oc.loc_heads(heads, dh))
    case.troute = temporal_route(b, f, dd, heads, dh, budget)
    return local_calls(case, [call("temporal_attention", ld=3 * c, ldo=c, B=b, F=f, D=dd, heads=heads, dh=dh, rot_dim=0 if plain else 32)],
                       temporal_budget=budget)


TATTN_SHAPES = [(1, 1, 3, 256), (1, 2, 1, 320), (1, 17, 5, 256), (2, 16, 5, 320)]
# Every streaming instantiation at every head / wave split it takes at the models' widths (8 heads: HG heads per 320 / 256 / 160 / 128-wide
# group, wph waves per head), at frame counts with and without a masked tail, and with several tiles per workgroup: per_group =
# (512 | 256) / ngroups workgroups walk a head group's B * D (packed: B * D / 2) tiles at stride per_group, so 2 per_group + 2 tiles
# give workgroups 0 and 1 three tiles (first: wait <PIECES>, steady state: <PIECES + STORES> and issue_tile(n + 2), last: <STORES>)
# and every other workgroup two; B = 2, so the walk t0 + n tstride crosses into the second video (t / Dt).
#  (b, f, d, c)           instantiation                      HG  wph   tiles / per_group   fullest / emptiest   what else
TATTN_STREAM = [
    (2, 13, 5, 640),     # temporal_stream_kernel<1, 320, 1>    4   1     10 / 10             1 / 1                F = 13: masked tail ((2, 16, 5, 320) above: HG 8, two heads per wave)
    (2, 16, 5, 1280),    # temporal_stream_kernel<1, 320, 1>    2   2     10 / 10             1 / 1                waves 2, 3 idle (one query block per head)
    (5, 16, 205, 320),   # temporal_stream_kernel<1, 320, 1>    8   1     1025 / 512          3 / 2                the narrowest: 16400 rows, workgroup 0 alone has three tiles; B = 5
    (2, 13, 129, 1280),  # temporal_stream_kernel<1, 320, 1>    2   2     258 / 128           3 / 2
    (2, 16, 5, 256),     # temporal_stream_kernel<1, 256, 1>    8   1     10 / 10             1 / 1
    (2, 13, 5, 512),     # temporal_stream_kernel<1, 256, 1>    4   1     10 / 10             1 / 1
    (2, 16, 5, 1024),    # temporal_stream_kernel<1, 256, 1>    2   2     10 / 10             1 / 1
    (2, 16, 129, 1024),  # temporal_stream_kernel<1, 256, 1>    2   2     258 / 128           3 / 2
    (2, 8, 6, 320),      # temporal_stream_kernel<1, 320, 2>    8   1     6 / 6               1 / 1                two pixels x 8 frames per tile: the base model's F = 8 route
    (2, 5, 6, 640),      # temporal_stream_kernel<1, 320, 2>    4   1     6 / 6               1 / 1                F = 5 < 8: masked frames inside both pixel halves
    (2, 8, 6, 1280),     # temporal_stream_kernel<1, 320, 2>    2   2     6 / 6               1 / 1
    (2, 5, 258, 1280),   # temporal_stream_kernel<1, 320, 2>    2   2     258 / 128           3 / 2
    (2, 8, 6, 256),      # temporal_stream_kernel<1, 256, 2>    8   1     6 / 6               1 / 1                the VSR UNet's route
    (2, 5, 6, 512),      # temporal_stream_kernel<1, 256, 2>    4   1     6 / 6               1 / 1
    (2, 8, 6, 1024),     # temporal_stream_kernel<1, 256, 2>    2   2     6 / 6               1 / 1
    (2, 8, 258, 1024),   # temporal_stream_kernel<1, 256, 2>    2   2     258 / 128           3 / 2
    (2, 17, 5, 320),     # temporal_stream_kernel<4, 160, 1>    4   2     10 / 10             1 / 1                F = 17: one valid key in the second key tile; the interpolation model's route
    (2, 61, 5, 640),     # temporal_stream_kernel<4, 160, 1>    2   4     10 / 10             1 / 1                F = 61
    (2, 64, 5, 1280),    # temporal_stream_kernel<4, 160, 1>    1   8     10 / 10             1 / 1                F = 64: no masked key
    (2, 17, 129, 320),   # temporal_stream_kernel<4, 160, 1>    4   2     258 / 128           3 / 2
    (2, 61, 33, 1280),   # temporal_stream_kernel<4, 160, 1>    1   8     66 / 32             3 / 2
    (2, 17, 5, 512),     # temporal_stream_kernel<4, 128, 1>    2   4     10 / 10             1 / 1                ((1, 17, 5, 256) above: HG 4, wph 2)
    (2, 61, 5, 256),     # temporal_stream_kernel<4, 128, 1>    4   2     10 / 10             1 / 1
    (2, 64, 5, 1024),    # temporal_stream_kernel<4, 128, 1>    1   8     10 / 10             1 / 1
    (2, 61, 33, 1024),   # temporal_stream_kernel<4, 128, 1>    1   8     66 / 32             3 / 2
]
# (b, f, d, c, heads, budget): the tile kernel through a budget and through shapes the launcher sends there itself (srl == 0: head dim 48
# tiles neither group width)
#                                        instantiation                 HG  PT  what
TATTN_TILE = [
    (2, 16, 5, 256, 8, 60000),         # temporal_attention_kernel<1>    8   2   D % PT = 1: a ragged last pixel tile
    (2, 16, 5, 320, 8, 20000),         # temporal_attention_kernel<1>    4   1   the budget halves HG
    (2, 17, 5, 128, 4, 120000),        # temporal_attention_kernel<4>    4   2   D % PT = 1 ((1, 17, 5, 256) at 33000 above: HG halved twice, to 2)
    (2, 16, 5, 384, 8, 0),             # temporal_attention_kernel<1>    4   1   sent there by the launcher: head dim 48; 33000 halves HG
    (2, 17, 5, 384, 8, 0),             # temporal_attention_kernel<4>    2   1   the same at 17 frames; 70000 halves HG twice
]
TATTN_PEAKED = [(2, 16, 5, 320), (2, 17, 5, 320)]          # one case of each NT under the `peaked` profile (stream), and temporal_block below
TATTN_MULTI = {"temporal_stream_kernel<1, 320, 1>": 2, "temporal_stream_kernel<1, 256, 1>": 1, "temporal_stream_kernel<1, 320, 2>": 1,
               "temporal_stream_kernel<1, 256, 2>": 1, "temporal_stream_kernel<4, 160, 1>": 2, "temporal_stream_kernel<4, 128, 1>": 1}   # cases with 3 / 2 tiles


def temporal_attention_cases():
    cs = [temporal_attention_case(*sh, t) for sh in TATTN_SHAPES for t in (False, True)]
    cs += [temporal_attention_case(1, 17, 5, 256, t, plain=True) for t in (False, True)]
    cs += [temporal_attention_case(*sh, False) for sh in TATTN_STREAM]
    cs += [temporal_attention_case(b, f, dd, c, bud, heads=h) for b, f, dd, c, h, bud in TATTN_TILE]
    cs += [temporal_attention_case(*sh, False, profile="peaked") for sh in TATTN_PEAKED]
    return cs


def ln(x, gamma, beta, cv, eps=1e-5):
    x = cv(x)
    mean = x.mean(-1, keepdim=True)
    return (x - mean) * ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt() * cv(gamma) + cv(beta)


def block_case(name, ins, run, chain, n, C, in_place, outs=None, where=None, cap=0, calls=None, twin=None):
    """A fused block: chain(cv, rq) -> name -> (value, scale); the float64 reference runs it without roundings, the model in
    fp32 with rq = one fp16 rounding at each counted point (the output store included).  cap: lavie_debug_rowfuse_grid around the
    launch (grid_cap; 0 = the production grid).  twin: the out-of-place case of the same inputs, whose reference an in-place case shares."""
    outs = outs or {"y": ((ins["x"].shape[0], C), f16)}

    def model():
        return {k: v.half() for k, (v, _) in chain(lambda t: t.float(), h_).items()}

    c = {k: oc.round_c(v) for k, v in n.items()} if isinstance(n, dict) else oc.round_c(n)
    case = Case(f"{name}[inplace{int(in_place)}]", ins, outs, run, (lambda: twin().ref) if twin else (lambda: chain(d, ident)), c, model,
                where or oc.loc_rows(C), alias={"y": "x"} if in_place else None,
                setup=(lambda restore: grid_cap(cap, restore)) if cap else None)
    case.chain, case.cap = chain, cap
    return local_calls(case, calls, rowfuse_grid=cap)


def rowfuse_walk(tiles, nwg, tiles_per_batch=None):
    """The share rule of the row-resident kernels (rowfuse.hip geglu_mlp_kernel / temporal_block_kernel, rowfuse_pin.hip, rowfuse_cross.hip:
    `share = tiles / nwg, rem = tiles - share * nwg, tile0 = bid * share + min(bid, rem)`): tile (or pixel unit) -> (workgroup, pass, wave).
    A workgroup takes a contiguous run, 8 per pass, one per wave; with tiles_per_batch (cross_block) a pass also ends at a video's last
    tile (`to_end`, rowfuse_cross.hip), since the pass streams that video's K / V image."""
    share, rem = divmod(tiles, nwg)
    out = [None] * tiles
    for bid in range(nwg):
        t, tend, ps = bid * share + min(bid, rem), bid * share + min(bid, rem) + share + (bid < rem), 0
        while t < tend:
            n = min(tend - t, 8)
            if tiles_per_batch:
                n = min(n, tiles_per_batch - t % tiles_per_batch)
            for w in range(n):
                out[t + w] = (bid, ps, w)
            t, ps = t + n, ps + 1
    assert None not in out
    return out


def walk_paths(walk, batch_of=None, ragged_last=False):
    """What a walk contains, as the set of path names the multi-pass cases are chosen for (PATHS below).  batch_of: tile -> video / frame."""
    nwg = 1 + max(w for w, _, _ in walk)
    passes = [1 + max(p for w, p, _ in walk if w == b) for b in range(nwg)]
    got = set()
    if max(passes) >= 3:
        got.add("three_passes")
    if len(set(passes)) > 1:
        got.add("pass_counts_differ")
    width = {}                                                   # (workgroup, pass) -> tiles in it
    for t, (w, p, _) in enumerate(walk):
        width.setdefault((w, p), []).append(t)
    if any(len(width[(b, passes[b] - 1)]) < 8 and passes[b] > 1 for b in range(nwg)):
        got.add("idle_waves_in_last_pass")
    if ragged_last and walk[-1][1] > 0:
        got.add("ragged_tile_in_later_pass")
    if batch_of:
        if any(len({batch_of(t) for t in ts}) > 1 for ts in width.values()):
            got.add("pass_spans_batches")
        for b in range(nwg):
            mine = [t for t, (w, _, _) in enumerate(walk) if w == b]
            if len({batch_of(t) for t in mine}) > 1:
                got.add("run_crosses_batch")
                # a pass cut short at the boundary (fewer than 8 tiles although the run goes on) and a later pass on the next video
                if any(len(width[(b, p)]) < 8 and p + 1 < passes[b] and batch_of(width[(b, p)][0]) != batch_of(width[(b, p + 1)][0]) for p in range(passes[b])):
                    got.add("pass_cut_at_batch_end")
            if mine and (mine[0] == 0 or batch_of(mine[0]) == batch_of(mine[0] - 1)) and mine[0] > 0:
                got.add("starts_mid_batch")
    return got


@functools.lru_cache(maxsize=None)
def geglu_mlp_case(M, in_place, C=320, cap=0):
    """x + W2 (h gelu(g)) + b2 with (h | g) = W1 LN(x) + b1.  n = 3: LN(x) (rowfuse.hip:185-186), h gelu(g) (:224-225), the output
    (:256).  scale = |h gelu(g)| |W2| + |b2| + |x|."""
    g = gen("geglu_mlp", M)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3 * torch.randn(1, C, generator=g)).half()
    w1, b1 = rnd(g, 8 * C, C, s=1 / math.sqrt(C)), rnd(g, 8 * C, s=0.2)
    w2, b2 = rnd(g, C, 4 * C, s=1 / math.sqrt(4 * C)), rnd(g, C, dtype=f32t, s=0.2)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ins = {"x": x, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "gamma": gamma, "beta": beta}

    def run(ops, i, o):
        img, b1img = ops.pack_geglu_mlp(i["w1"], i["b1"], i["w2"])
        ops.geglu_mlp(i["x"], img, b1img, i["gamma"], i["beta"], i["b2"], out=o["y"])

    def chain(cv, rq):
        hh, gate = (rq(ln(x, gamma, beta, cv)) @ cv(w1).t() + cv(b1)).chunk(2, -1)
        hg = rq(hh * gelu64(gate))
        return {"y": (cv(x) + hg @ cv(w2).t() + cv(b2), hg.abs() @ cv(w2).abs().t() + cv(b2).abs() + cv(x).abs())}

    return block_case(f"geglu_mlp[M{M}" + (f",cap{cap}]" if cap else "]"), ins, run, chain, 3, C, in_place, cap=cap,
                      calls=[call("geglu_mlp", M=M, C=C)], twin=(lambda: geglu_mlp_case(M, False, C, cap)) if in_place else None)


@functools.lru_cache(maxsize=None)
def cross_block_case(B, P, L, in_place, C=320, heads=8, cap=0):
    """x1 = x + Wo1 att + bo1; y = x1 + Wo2 attn2(LN(x1) Wq2, K, V) + bo2, K | V bound per video; the long variant above 80 keys.
    n = 5: LN(x1) (rowfuse_cross.hip:430-431), q as the MFMA operand (:488 / :496), P (:571), the attention output (:614 / :622), the
    output store (rowfuse.h:173).  scale = |o| |Wo2| + |bo2| + |att| |Wo1| + |bo1| + |x|."""
    g = gen("cross_block", B, P, L)
    M, dh = B * P, C // heads
    long = L > 80
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3 * torch.randn(1, C, generator=g)).half()
    att = rnd(g, M, C)
    wo1, wq2, wo2 = (rnd(g, C, C, s=1 / math.sqrt(C)) for _ in range(3))
    bo1, bo2 = rnd(g, C, dtype=f32t, s=0.2), rnd(g, C, dtype=f32t, s=0.2)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    kv = rnd(g, B * L, 2 * C)
    ins = dict(x=x, att=att, wo1=wo1, wq2=wq2, wo2=wo2, bo1=bo1, bo2=bo2, gamma=gamma, beta=beta, kv=kv)

    def run(ops, i, o):
        pack, bind, op = ((ops.pack_cross_block_long, ops.bind_cross_block_long, ops.cross_block_long) if long else
                          (ops.pack_cross_block, ops.bind_cross_block, ops.cross_block))
        img = bind(pack(i["wo1"], i["wq2"], i["wo2"]), i["kv"], B, L)
        op(i["att"], i["x"], img, i["bo1"], i["gamma"], i["beta"], i["bo2"], P, L, heads, dh ** -0.5, out=o["y"])

    def chain(cv, rq, video_of=None):
        """video_of (injected defects): the video whose K | V each video's rows attend to, instead of their own"""
        x1 = cv(x) + cv(att) @ cv(wo1).t() + cv(bo1)
        s1 = cv(x).abs() + cv(att).abs() @ cv(wo1).abs().t() + cv(bo1).abs()
        q = rq(rq(ln(x1, gamma, beta, cv)) @ cv(wq2).t()).reshape(B, P, heads, dh).permute(0, 2, 1, 3)
        kvv = kv if video_of is None else kv.reshape(B, L, 2 * C)[list(video_of)].reshape(B * L, 2 * C)
        k = cv(kvv[:, :C]).reshape(B, L, heads, dh).permute(0, 2, 1, 3)
        v = cv(kvv[:, C:]).reshape(B, L, heads, dh).permute(0, 2, 1, 3)
        s = q @ k.transpose(-1, -2) * dh ** -0.5
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        o = rq((rq(e) @ v) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(M, C)
        return {"y": (x1 + o @ cv(wo2).t() + cv(bo2), s1 + o.abs() @ cv(wo2).abs().t() + cv(bo2).abs())}

    entry = "cross_block_long" if long else "cross_block"
    return block_case(f"{entry}[B{B},P{P},L{L}" + (f",cap{cap}]" if cap else "]"), ins, run, chain, 5, C, in_place, cap=cap,
                      calls=[call(entry, M=M, rows_per_batch=P, C=C, heads=heads, ctx_len=L)],
                      twin=(lambda: cross_block_case(B, P, L, False, C, heads, cap)) if in_place else None)


# (videos, rows per video, keys): rows per video must be a multiple of the 16-token wave tile (cross_block_supported); 16 = the
# smallest, 144 = one 128-row pass and a ragged one per video.  CROSS_REFUSED: one row per video, which both kernels refuse
CROSS_BLOCKS = [(1, 16, 1), (2, 144, 5), (3, 16, 77), (1, 144, 80), (1, 16, 81), (2, 144, 160)]
CROSS_REFUSED = [(1, 1, 5), (1, 1, 100)]


@functools.lru_cache(maxsize=None)
def temporal_block_case(B, D, in_place, C=320, heads=8, Fr=16, cap=0, profile="unit"):
    """x + Wo attn_temp(LN(x)) + bo on rows (b f) d.  n = 7: LN(x) (rowfuse.hip:482-483), q scaled and rotated, k rotated, v
    (:521-523), exp() of the scores (:572), the attention output (:577-583), the output store (:641).
    scale = |o| |Wo| + |bo| + |x|."""
    g = gen("temporal_block", B, D)
    M, dh = B * Fr * D, C // heads
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3 * torch.randn(1, C, generator=g)).half()
    wq, wk, wv, wo = (rnd(g, C, C, s=1 / math.sqrt(C)) for _ in range(4))
    bo = rnd(g, C, dtype=f32t, s=0.2)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    relbias = rnd(g, heads, Fr, Fr, dtype=f32t)
    if profile == "peaked":
        relbias = peak_bias(relbias, Fr)
    cos, sin = rotary_tables(Fr)
    ins = dict(x=x, wq=wq, wk=wk, wv=wv, wo=wo, bo=bo, gamma=gamma, beta=beta, relbias=relbias, cos=cos, sin=sin)
    if profile == "peaked":          # on the q and k the kernel forms: projections of the rounded LN(x), in float64
        xn = h_(ln(x, gamma, beta, lambda t: t.float())).double()
        sq = lambda w: (xn @ d(w).t()).reshape(B, Fr, D, heads, dh).permute(0, 2, 3, 1, 4).reshape(B * D, heads, Fr, dh)
        assert_peaked(sq(wq), sq(wk), relbias, cos, sin, dh ** -0.5, Fr)

    def run(ops, i, o):
        img = ops.pack_temporal_block(i["wq"], i["wk"], i["wv"], i["wo"])
        ops.temporal_block(i["x"], img, i["gamma"], i["beta"], i["bo"], i["relbias"], i["cos"], i["sin"], B, Fr, D, heads, 32,
                           dh ** -0.5, out=o["y"])

    def chain(cv, rq):
        xn = rq(ln(x, gamma, beta, cv))
        seq = lambda w: (xn @ cv(w).t()).reshape(B, Fr, D, heads, dh).permute(0, 2, 3, 1, 4).reshape(B * D, heads, Fr, dh)
        # q and k are rounded after scale / rotary (inside temporal_core), v as it leaves its projection
        o, _ = temporal_core(seq(wq), seq(wk), rq(seq(wv)), relbias, cos, sin, dh ** -0.5, ident, rq, True)
        o = rq(o).reshape(B, D, heads, Fr, dh).permute(0, 3, 1, 2, 4).reshape(M, C)
        return {"y": (cv(x) + o @ cv(wo).t() + cv(bo), cv(x).abs() + o.abs() @ cv(wo).abs().t() + cv(bo).abs())}

    tag = (f",cap{cap}" if cap else "") + ("" if profile == "unit" else f",{profile}")
    return block_case(f"temporal_block[B{B},D{D}{tag}]", ins, run, chain, 7, C, in_place, cap=cap,
                      calls=[call("temporal_block", B=B, F=Fr, D=D, C=C, heads=heads, rot_dim=32)],
                      twin=(lambda: temporal_block_case(B, D, False, C, heads, Fr, cap, profile)) if in_place else None)


@functools.lru_cache(maxsize=None)
def proj_qkv_case(NB, D, C=320, cap=0):
    """tx = Wpin (a x + b) + bpin with the per-(frame, channel) GroupNorm pairs (a, b) as an input; qkv = Wqkv LN(tx).
    tx: n = 2 — a x + b (rowfuse_pin.hip:153-160), the store (rowfuse.h:173).  qkv: n = 3 — a x + b, LN(tx) taken from the fp32
    accumulators (rowfuse_pin.hip:223-224), the store."""
    g = gen("proj_qkv", NB, D)
    M, G = NB * D, 32
    x = (torch.randn(M, C, generator=g) * 1.3 + 0.4 * torch.randn(NB, 1, C, generator=g).repeat_interleave(D, 0).reshape(M, C)).half()
    gn_g, gn_b = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wpin, bpin = rnd(g, C, C, s=1 / math.sqrt(C)), rnd(g, C, dtype=f32t, s=0.2)
    ln_g, ln_b = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wqkv = rnd(g, 3 * C, C, s=1 / math.sqrt(C))
    xg = x.float().reshape(NB, D, G, C // G)
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    a = (var + 1e-6).rsqrt().repeat_interleave(C // G, 1) * gn_g
    ab = torch.stack([a, gn_b - mean.repeat_interleave(C // G, 1) * a], -1).contiguous()          # [NB, C, 2]
    ins = dict(x=x, ab=ab, wpin=wpin, wqkv=wqkv, bpin=bpin, ln_g=ln_g, ln_b=ln_b)

    def run(ops, i, o):
        ops.proj_qkv(i["x"], i["ab"], D, ops.pack_proj_qkv(i["wpin"], i["wqkv"]), i["bpin"], i["ln_g"], i["ln_b"], tx=o["tx"], qkv=o["qkv"])

    def chain(cv, rq):
        aa, bb = cv(ab[..., 0]).repeat_interleave(D, 0), cv(ab[..., 1]).repeat_interleave(D, 0)
        xb = rq(cv(x) * aa + bb)
        tx = xb @ cv(wpin).t() + cv(bpin)
        xb2 = rq(ln(tx, ln_g, ln_b, cv))
        return {"tx": (tx, xb.abs() @ cv(wpin).abs().t() + cv(bpin).abs()), "qkv": (xb2 @ cv(wqkv).t(), xb2.abs() @ cv(wqkv).abs().t())}

    return block_case(f"proj_qkv[NB{NB},D{D}" + (f",cap{cap}]" if cap else "]"), ins, run, chain, {"tx": 2, "qkv": 3}, C, False,
                      outs={"tx": ((M, C), f16), "qkv": ((M, 3 * C), f16)}, where={"tx": oc.loc_rows(C), "qkv": oc.loc_rows(3 * C)}, cap=cap,
                      calls=[call("proj_qkv", rows_per_domain=D, M=M, C=C)])


# Past one tile per workgroup.  All four launchers start min(tiles, 256) workgroups, so every case above gives each workgroup one
# tile and only wave 0 of it real rows; a second pass needs 2049 tiles (32784 rows).  The capped cases run the same kernels on
# lavie_debug_rowfuse_grid workgroups (the kernels read gridDim.x and nothing else about the grid): rowfuse_walk is the share rule, PATHS
# what the case set as a whole must contain (test_opcheck_host.py::test_multi_pass_cases_contain_every_path).
#  case                                       tiles, shares, passes            path it provides
#  geglu_mlp M = 795, cap 3                   50: 17 / 17 / 16, 3 / 3 / 2      first, steady-state and last pass (issue_group past PASS_GROUPS, the counted vmcnt(5) with a next
#                                                                              pass behind it); last pass of workgroups 0, 1 = one wave of eight; pass counts differ; the ragged
#                                                                              tile 49 (rows 784..794, the rowc clamp) is wave 7 of workgroup 2's second pass
#  temporal_block B = 5, D = 10, cap 3        50 pixels: 17 / 17 / 16          the same three; passes of eight pixels span two videos (unit / p.D: pixels 8..15 = videos 0 | 1)
#                                                                              (B = 2, D = 25 cuts its passes exactly at the video boundary, 17 + 8 = 25: it has no such pass)
#  cross_block B = 4, P = 224, L = 77, cap 3  56 (14 a video): 19 / 19 / 18,   workgroup 0: tiles 0..7, 8..13 (cut at the video's end, six waves), 14..18 on video 1's image;
#    and cross_block_long at L = 160          passes 3 / 4 / 3                 workgroup 1 starts at tile 19, mid-video 1, and runs 19..26, 27 (one tile left of video 1), 28..35,
#                                                                              36..37; workgroup 2 starts mid-video 2.  (B = 4, P = 208 gives 3 / 3 / 3 passes: none differ)
#  proj_qkv NB = 5, D = 160, cap 3            50 (10 a frame): 17 / 17 / 16    the same three; every full pass has waves under two frames' (a, b) pairs
#  temporal_block B = 3, D = 683, cap 0       2049 pixels on 256 workgroups    the production launch: workgroup 0 has nine pixels = a second pass of one wave, the others eight
# The natural grid is run for temporal_block alone: its float64 reference and scale are 1.3e10 + 3.4e9 multiply-adds, under DESIGN.md's
# 2^34; at 32784 rows geglu_mlp needs 5.0e10 + 1.7e10, proj_qkv 2.7e10 + 2.7e10 and cross_block 2.3e10 (L = 77), all above it: their
# natural-grid cover stays the 40960-row rel-L2 tests of tests/test_gpu_rowfuse.py.
PATHS = {"geglu_mlp": {"three_passes", "idle_waves_in_last_pass", "pass_counts_differ", "ragged_tile_in_later_pass"},
         "temporal_block": {"three_passes", "idle_waves_in_last_pass", "pass_counts_differ", "pass_spans_batches"},
         "cross_block": {"three_passes", "idle_waves_in_last_pass", "pass_counts_differ", "run_crosses_batch", "pass_cut_at_batch_end", "starts_mid_batch"},
         "cross_block_long": {"three_passes", "idle_waves_in_last_pass", "pass_counts_differ", "run_crosses_batch", "pass_cut_at_batch_end", "starts_mid_batch"},
         "proj_qkv": {"three_passes", "idle_waves_in_last_pass", "pass_counts_differ", "pass_spans_batches"}}
MULTI_GEGLU = [(795, 3)]                         # (M, cap)
MULTI_TEMPORAL = [(5, 10, 3), (3, 683, 0)]       # (B, D, cap)
MULTI_CROSS = [(4, 224, 77, 3), (4, 224, 160, 3)]   # (B, P, L, cap)
MULTI_PROJ = [(5, 160, 3)]                       # (NB, D, cap)
NATURAL_GRID = "temporal_block[B3,D683]"


def multi_pass_cases(in_place=False):
    """the multi-pass cases, out of place (or, where the block takes aliasing, in place)"""
    cs = [geglu_mlp_case(M, in_place, cap=cap) for M, cap in MULTI_GEGLU]
    cs += [temporal_block_case(B, D, in_place, cap=cap) for B, D, cap in MULTI_TEMPORAL]
    cs += [cross_block_case(B, P_, L, in_place, cap=cap) for B, P_, L, cap in MULTI_CROSS]
    return cs if in_place else cs + [proj_qkv_case(NB, D, cap=cap) for NB, D, cap in MULTI_PROJ]


def case_walk(case):
    """(family, walk, paths) of a block case, from the integers of its call and its cap (0: the launcher's min(tiles, 256))"""
    entry, a = case.calls[0]
    cap = case.cap or 256
    if entry == "geglu_mlp":
        tiles = -(-a["M"] // 16)
        walk = rowfuse_walk(tiles, min(tiles, cap))
        return entry, walk, walk_paths(walk, ragged_last=a["M"] % 16 != 0)
    if entry == "temporal_block":
        units = a["B"] * a["D"]
        walk = rowfuse_walk(units, min(units, cap))
        return entry, walk, walk_paths(walk, batch_of=lambda t: t // a["D"])
    if entry == "proj_qkv":
        tiles, per = -(-a["M"] // 16), a["rows_per_domain"] // 16
        walk = rowfuse_walk(tiles, min(tiles, cap))
        return entry, walk, walk_paths(walk, batch_of=lambda t: t // per)
    tiles, per = a["M"] // 16, a["rows_per_batch"] // 16
    walk = rowfuse_walk(tiles, min(tiles, cap), per)
    return entry, walk, walk_paths(walk, batch_of=lambda t: t // per)


# ------------------------------------------------------------------ sampler steps and lora_merge
STEP_KINDS = ["cfg_ddpm_step", "sampler_step", "cfg_multistep_step", "multistep_step", "latents_to_model_input", "latents_to_model_input1"]
STEP_LENGTHS = [1, 7, 8, 9, 4097]


@functools.lru_cache(maxsize=None)
def step_case(kind, n):
    """Elementwise fp32 updates; x (and x0_prev) are rewritten in place, model_in is the fp16 output.  Bound: the GEMM family's with
    K_terms = 6 (at most six fp32 operations per element) on the sum of the absolute terms."""
    g = gen("step", kind, n)
    cfg = kind.startswith("cfg") or kind == "latents_to_model_input"
    multi = "multistep" in kind
    copy_only = kind.startswith("latents")
    guidance, in_scale = 7.5, 0.8125
    kx, ke, c0, ct, last = 1.25, 0.75, 0.375, 0.625, 0.5          # last: sigma (ddpm) or c_prev (multistep)
    x = rnd(g, n, dtype=f32t)
    ins = {"x": x}
    outs = {"model_in": ((2 * n if cfg else n,), f16)}
    alias = {}
    if not copy_only:
        ins["eps"] = rnd(g, 2 * n if cfg else n)
        ins["aux"] = rnd(g, n, dtype=f32t)                          # noise or x0_prev
        outs["x"] = ((n,), f32t)
        alias["x"] = "x"
        if multi:
            outs["aux"] = ((n,), f32t)
            alias["aux"] = "aux"

    def run(ops, i, o):
        co = (kx, ke, c0, ct, last)
        if kind == "cfg_ddpm_step":
            ops.cfg_ddpm_step(i["eps"], i["x"], i["aux"], o["model_in"], guidance, co, in_scale)
        elif kind == "sampler_step":
            ops.sampler_step(i["eps"], i["x"], i["aux"], o["model_in"], co, in_scale)
        elif kind == "cfg_multistep_step":
            ops.cfg_multistep_step(i["eps"], i["x"], i["aux"], o["model_in"], guidance, co, in_scale)
        elif kind == "multistep_step":
            ops.multistep_step(i["eps"], i["x"], i["aux"], o["model_in"], co, in_scale)
        elif kind == "latents_to_model_input":
            ops.latents_to_model_input(i["x"], o["model_in"], in_scale)
        else:
            ops.latents_to_model_input1(i["x"], o["model_in"], in_scale)

    def compute(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        s = (lambda a, b: a + b) if absval else (lambda a, b: a - b)     # a difference counts with both magnitudes
        k = abs if absval else (lambda t: t)
        xt = p(cv(x))
        res = {}
        if copy_only:
            xn = xt
        else:
            e = p(cv(ins["eps"]))
            eps = e[:n] + k(guidance) * s(e[n:], e[:n]) if cfg else e
            x0 = s(k(kx) * xt, k(ke) * eps)
            aux = p(cv(ins["aux"]))
            if multi:
                xn = k(c0) * (x0 + k(last) * s(x0, aux)) + k(ct) * xt
                res["aux"] = x0
            else:
                xn = k(c0) * x0 + k(ct) * xt + k(last) * aux
            res["x"] = xn
        mi = xn * in_scale
        res["model_in"] = torch.cat([mi, mi]) if cfg else mi
        return res

    def ref():
        r, sc = compute(d, False), compute(d, True)
        return {kk: (r[kk], sc[kk]) for kk in r}

    def model():
        r = compute(lambda t: t.float(), False)
        r["model_in"] = r["model_in"].half()
        return r

    return Case(f"{kind}[{n}]", ins, outs, run, ref, oc.gemm_c(6), model, lambda i: f"element {i}", alias=alias)


LORA_SHAPES = [(1, 8, 1), (3, 24, 2), (320, 320, 16)]


@functools.lru_cache(maxsize=None)
def lora_case(N, K, r, in_place):
    g = gen("lora", N, K, r)
    w0, a, b = rnd(g, N, K), rnd(g, r, K, dtype=f32t), rnd(g, N, r, dtype=f32t, s=0.1)
    scale = 0.75
    ins = {"w0": w0, "a": a, "b": b}

    def run(ops, i, o):
        ops.lora_merge(i["w0"], i["a"], i["b"], scale, out=o["y"])

    terms = lambda cv, p: p(cv(w0)) + scale * (p(cv(b)) @ p(cv(a)))
    ident, ab_ = (lambda t: t), (lambda t: t.abs())
    return Case(f"lora_merge[{N}x{K},r{r},inplace{int(in_place)}]", ins, {"y": ((N, K), f16)}, run,
                lambda: {"y": (terms(d, ident), terms(d, ab_))}, oc.gemm_c(r + 2),
                lambda: {"y": terms(lambda t: t.float(), ident).half()}, oc.loc_rows(K), alias={"y": "w0"} if in_place else None)


# ------------------------------------------------------------------ the forward's ends and glue: time embedding, the NCFHW boundary, load-time packs
# Every kernel here has one entry point of its own (lavie_amd/ops.py, "end and glue kernels").  fp32 outputs are checked with
# u = U32.  Pure moves and exact conversions are compared bit for bit (Case.exact) against the index formula of the kernel's header
# comment written out in torch indexing.
GEOMS = [(1, 1, 1, 1), (1, 1, 3, 5), (2, 3, 3, 5), (1, 2, 8, 8)]          # (B, F, H, W): M = 1, 15 (< a wave's 16 pixels), 90, 128
LOG2E32 = torch.tensor(LOG2E, dtype=f32t)


def wave_sum32(t):
    """common.h wave_sum on the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1, in fp32; lane 0's value"""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        t = t + t[..., lanes ^ o]
    return t[..., 0]


def silu32(x):
    """common.h silu_f in torch fp32: x / (1 + exp2(-x log2 e))"""
    return x / (1.0 + torch.exp2(-x * LOG2E32))


def silu_rel(x):
    """The error of silu_f relative to |silu(x)|, counted in its source (common.h:61, x / (1.0f + __expf(-x)), __expf = exp2 of the
    product with fp32 log2 e), in units of 2^-23 = one fp32 ulp, with s = e / (1 + e) = sigmoid(-x) <= 1 the factor by which a
    relative error of e = exp(-x) reaches the quotient:
      the product -x log2(e): one rounding and the constant's own, 2 * 2^-24 |x log2 e| absolute in the exponent, times ln 2:  |x| s
      the hardware exp2 (v_exp_f32, 1 ulp):                                                                                    1 s
      the add 1 + e (half an ulp of the sum):                                                                                  0.5
      the divide (correctly rounded or not: 1 ulp):                                                                            1
    = 2.5 + |x| s at first order, counted as 3 + |x| s."""
    return oc.U32 * (3.0 + x.abs() * torch.sigmoid(-x))


def frames_nchw(x5):
    """[B, C, F, H, W] -> per-frame images [(B F), C, H, W]"""
    B, Cc, Fr, H, W = x5.shape
    return x5.permute(0, 2, 1, 3, 4).reshape(B * Fr, Cc, H, W)


def im2col(xf, cin):
    """per-frame images [N, cin, H, W] -> [N H W, 9 cin] in (tap, channel) order, zeros outside the image"""
    N, _, H, W = xf.shape
    xp = F.pad(xf, (1, 1, 1, 1))
    cols = [xp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1).reshape(N * H * W, cin) for ky in range(3) for kx in range(3)]
    return torch.cat(cols, 1)


def conv_out_route(cin, cout):
    """launch_conv_out's choice (elementwise.hip), as the name the launch trace shows"""
    slots = 9 * (cin // 8)
    if cout == 4 and slots <= 64 * 6:
        return "conv_out4_kernel<5>" if slots <= 64 * 5 else "conv_out4_kernel<6>"
    return "conv_out_kernel"


def conv_out_lanes(P, Wk, drop_from=None):
    """conv_out_kernel / conv_out4_kernel in fp32: P [M, 9 cin] (im2col), Wk [cout, 9 cin]; slot i = (tap, 8-channel vector) belongs
    to lane i % 64 and is its (i / 64)-th; a lane adds its slots' eight exact products in order (four fdot2, each as two fp32 fmas),
    then the butterfly.  drop_from: slots from this one on are left out (an injected defect)."""
    M, K = P.shape
    slots = K // 8
    nv = -(-slots // 64)
    pad = nv * 64 * 8 - K
    Pp, Wp_ = F.pad(P, (0, pad)).reshape(M, nv, 64, 8), F.pad(Wk, (0, pad)).reshape(-1, nv, 64, 8)
    if drop_from is not None:
        keep = (torch.arange(nv * 64) < drop_from).reshape(nv, 64, 1).float()
        Wp_ = Wp_ * keep
    acc = torch.zeros(M, Wk.shape[0], 64)
    for j in range(nv):
        for e in range(8):
            acc = acc + Pp[:, None, j, :, e] * Wp_[None, :, j, :, e]
    return wave_sum32(acc)


@functools.lru_cache(maxsize=None)
def conv_out_case(cin, cout, geom):
    """channels-last rows [M, cin] -> NCFHW [B, cout, F, H, W]; GEMM family, K_terms = 9 cin (the bias add and the store are in the
    8 of gemm_c)."""
    B, Fr, H, W = geom
    g = gen("conv_out", cin, cout, geom)
    x5 = rnd(g, B, cin, Fr, H, W)
    wt, b = rnd(g, cout, cin, 3, 3, s=1 / math.sqrt(9 * cin)), rnd(g, cout, dtype=f32t, s=0.5)
    ins = {"x": rows(frames_nchw(x5)), "wt": wt, "b": b}
    back = lambda y: y.reshape(B, Fr, cout, H, W).permute(0, 2, 1, 3, 4).contiguous()

    def run(ops, i, o):
        wp = ops.pack_conv_out(i["wt"], out=torch.empty(cout, 9 * cin, dtype=f16, device=i["wt"].device))
        ops.conv_out(i["x"], wp, i["b"], B, Fr, H, W, out=o["y"])

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        return back(F.conv2d(p(cv(frames_nchw(x5))), p(cv(wt)), p(cv(b)), padding=1))

    def model(drop_from=None):
        P = im2col(frames_nchw(x5).float(), cin)
        Wk = wt.float().permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        y = (conv_out_lanes(P, Wk, drop_from) + b).half()                       # [M, cout]
        return {"y": back(y.reshape(B * Fr, H, W, cout).permute(0, 3, 1, 2))}

    border = torch.ones(B, cout, Fr, H, W, dtype=torch.bool)
    if H > 2 and W > 2:
        border[..., 1:-1, 1:-1] = False
    m = torch.arange(B * Fr * H * W)
    crossed = ((m // 16 * 16) // (H * W) != m // (H * W)).reshape(B, 1, Fr, H, W).expand(B, cout, Fr, H, W)   # a wave's 16-pixel run began in another image
    case = Case(f"conv_out[{cin}->{cout},{'x'.join(map(str, geom))}]", ins, {"y": ((B, cout, Fr, H, W), f16)}, run,
                lambda: {"y": (terms(d, False), terms(d, True))}, oc.gemm_c(9 * cin), model,
                lambda i: "(batch %d, channel %d, frame %d, y %d, x %d)" % (i // (cout * Fr * H * W), i // (Fr * H * W) % cout, i // (H * W) % Fr, i // W % H, i % W),
                regions={"border": border.reshape(-1), "run_from_another_image": crossed.reshape(-1)})
    case.kernel = conv_out_route(cin, cout)
    return with_calls(case, [call("pack_conv_out", Cout=cout, Cin=cin), call("conv_out", B=B, Cin=cin, F=Fr, H=H, W=W, Cout=cout)])


# (cin, cout): conv_out4<5> at 288 and 72 slots (lanes above 8 idle in the second register slot), conv_out4<6> at 360 and 378 (the
# most it takes), the general kernel at the first cin past the register kernel and at cout != 4
CONV_OUT_SHAPES = [(256, 4), (64, 4), (320, 4), (336, 4), (344, 4), (64, 8), (64, 3)]
CONV_OUT_REFUSED = [(60, 4), (64, 9), (4096, 8)]          # cin % 8, cout > 8, LDS


@functools.lru_cache(maxsize=None)
def conv_in_case(cin, cout, geom):
    """NCFHW [B, cin, F, H, W] -> channels-last rows; GEMM family, K_terms = 9 cin.  A thread starts from the bias and adds the
    taps inside the image in (tap, channel) order, two channels per fdot2."""
    B, Fr, H, W = geom
    g = gen("conv_in", cin, cout, geom)
    x5 = rnd(g, B, cin, Fr, H, W)
    wt, b = rnd(g, cout, cin, 3, 3, s=1 / math.sqrt(9 * cin)), rnd(g, cout, dtype=f32t, s=0.5)
    ins = {"x": x5, "wt": wt, "b": b}

    def run(ops, i, o):
        wp = ops.pack_conv_in(i["wt"], out=torch.empty(9 * cin * cout, dtype=f16, device=i["wt"].device))
        ops.conv_in(i["x"], wp, i["b"], cout, out=o["y"])

    def terms(cv, absval):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        return rows(F.conv2d(p(cv(frames_nchw(x5))), p(cv(wt)), p(cv(b)), padding=1))

    def model(swap_pair=None):
        """swap_pair: the K pair whose two channels are exchanged on the activation side (an injected defect)"""
        P = im2col(frames_nchw(x5).float(), cin)
        if swap_pair is not None:
            P = P.clone()
            P[:, [2 * swap_pair, 2 * swap_pair + 1]] = P[:, [2 * swap_pair + 1, 2 * swap_pair]]
        Wk = wt.float().permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        acc = b.float().expand(P.shape[0], cout).clone()
        for k in range(9 * cin):
            acc = acc + P[:, k:k + 1] * Wk[None, :, k]
        return {"y": acc.half()}

    case = Case(f"conv_in[{cin}->{cout},{'x'.join(map(str, geom))}]", ins, {"y": ((B * Fr * H * W, cout), f16)}, run,
                lambda: {"y": (terms(d, False), terms(d, True))}, oc.gemm_c(9 * cin), model, oc.loc_image(B * Fr, H, W, cout),
                regions={"border": border_mask(B * Fr, H, W, cout)})
    return with_calls(case, [call("pack_conv_in", Cout=cout, Cin=cin), call("conv_in", B=B, Cin=cin, F=Fr, H=H, W=W, Cout=cout)])


CONV_IN_SHAPES = [(ci, co) for ci in (4, 8, 2) for co in (8, 256, 320)]
CONV_IN_REFUSED = [(7, 8), (4, 12), (8, 512)]             # cin odd, cout % 8, LDS: 9 * 8 * 512 * 2 > 65536


def conv_in_fits(cin, cout):
    return 9 * cin * cout * 2 <= 65536


def move_case(name, ins, outs, run, expect, where=None, partial=None, calls=None):
    """A pure move or an exact conversion: expect() -> name -> the expected tensor, compared bit for bit (and, trivially, through the
    bound with u = c = 0).  partial outputs hold the finite poison outside their mask in what run_guarded returns."""
    def ref():
        return {k: (v.to(f64), torch.zeros(v.shape, dtype=f64)) for k, v in expect().items()}
    case = Case(name, ins, outs, run, ref, 0.0, expect, where or (lambda i: f"element {i}"), u=0.0, partial=partial)
    case.exact = _Lazy(expect)
    return with_calls(case, calls) if calls else case


class _Lazy(dict):
    """name -> tensor, computed on first use"""

    def __init__(self, fn):
        super().__init__()
        self._fn = fn

    def items(self):
        if not len(self):
            self.update(self._fn())
        return super().items()


@functools.lru_cache(maxsize=None)
def pack_conv_in_case(cin, cout):
    """out[(k / 2) * cout * 2 + co * 2 + k % 2] = w[co, ci, ky, kx], k = (ky * 3 + kx) * cin + ci (elementwise.hip pack_conv_in_kernel)"""
    w = rnd(gen("pack_conv_in", cin, cout), cout, cin, 3, 3)

    def expect():
        wk = w.permute(2, 3, 1, 0).reshape(9 * cin, cout)                      # [k, co]
        return {"y": wk.reshape(9 * cin // 2, 2, cout).permute(0, 2, 1).reshape(-1).contiguous()}
    return move_case(f"pack_conv_in[{cin}->{cout}]", {"w": w}, {"y": ((9 * cin * cout,), f16)}, lambda ops, i, o: ops.pack_conv_in(i["w"], out=o["y"]),
                     expect, calls=[call("pack_conv_in", Cout=cout, Cin=cin)])


@functools.lru_cache(maxsize=None)
def pack_conv_out_case(cin, cout):
    """the unchunked pack_conv3x3: out[co, tap * cin + ci] = w[co, ci, tap]"""
    w = rnd(gen("pack_conv_out", cin, cout), cout, cin, 3, 3)
    return move_case(f"pack_conv_out[{cin}->{cout}]", {"w": w}, {"y": ((cout, 9 * cin), f16)}, lambda ops, i, o: ops.pack_conv_out(i["w"], out=o["y"]),
                     lambda: {"y": w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()}, where=oc.loc_rows(9 * cin),
                     calls=[call("pack_conv_out", Cout=cout, Cin=cin)])


PACK_CONV_OUT_SHAPES = [(64, 4), (320, 4), (8, 3)]


@functools.lru_cache(maxsize=None)
def pack_geglu_vec_case(N):
    v = rnd(gen("pack_geglu_vec", N), N, dtype=f32t)
    return move_case(f"pack_geglu_vec[{N}]", {"v": v}, {"y": ((N,), f32t)}, lambda ops, i, o: ops.pack_geglu_vec(i["v"], out=o["y"]),
                     lambda: {"y": v[geglu_perm(N)].contiguous()}, calls=[call("pack_geglu_vec", N=N)])


COPY_ROWS = [(1, 1, 1, 1, 0), (3, 64, 64, 640, 576), (5, 7, 9, 31, 11), (320, 64, 64, 2944, 2880)]        # (rows, cols, ld_src, ld_dst, col0)
COPY_ROWS_REFUSED = [(3, 8, 7, 16, 0), (3, 8, 8, 15, 8)]                                                   # ld_src < cols, ld_dst < col0 + cols


@functools.lru_cache(maxsize=None)
def copy_rows_case(nrows, cols, ld_src, ld_dst, col0, shift=0):
    """dst[r, col0 + c] = src[r, c], c < cols: a sub-rectangle of dst — every other element keeps its poison (partial)"""
    src = rnd(gen("copy_rows", nrows, cols, ld_src, ld_dst, col0), nrows, ld_src)
    mask = torch.zeros(nrows, ld_dst, dtype=torch.bool)
    mask[:, col0:col0 + cols] = True

    def expect(shift=shift):
        y = torch.full((nrows, ld_dst), oc.SENTINEL, dtype=f16)
        y[:, col0 + shift:col0 + shift + cols] = src[:, :cols]
        return {"y": y}
    return move_case(f"copy_rows[{nrows}x{cols},ld{ld_src}->{ld_dst},col{col0}]", {"src": src}, {"y": ((nrows, ld_dst), f16)},
                     lambda ops, i, o: ops.copy_rows(i["src"], o["y"], col0, cols=cols), expect, where=oc.loc_rows(ld_dst), partial={"y": mask},
                     calls=[call("copy_rows", ld_src=ld_src, ld_dst=ld_dst, rows=nrows, cols=cols, col0=col0)])


@functools.lru_cache(maxsize=None)
def f16_to_f32_case(n, two):
    """float(a) (+ float(b)): the sum of two fp16 values is exact in fp32"""
    g = gen("f16_to_f32", n, two)
    ins = {"a": rnd(g, n)}
    if two:
        ins["b"] = rnd(g, n, s=37.0)

    def expect():
        return {"y": ins["a"].float() + ins["b"].float() if two else ins["a"].float()}
    return move_case(f"f16_to_f32[{n},{'a+b' if two else 'a'}]", ins, {"y": ((n,), f32t)}, lambda ops, i, o: ops.f16_to_f32(i["a"], i.get("b"), out=o["y"]),
                     expect, calls=[call("f16_to_f32", n=n, b=two)])


def relpos_table(Fr, num_buckets, max_distance):
    """relpos_bucket_table (elementwise.hip) in Python: the T5 bucket of (query i, key j)"""
    half_b = num_buckets // 2
    exact = half_b // 2
    out = torch.zeros(Fr, Fr, dtype=torch.int32)
    for i in range(Fr):
        for j in range(Fr):
            n = i - j
            bkt = half_b if n < 0 else 0
            n = abs(n)
            if n < exact:
                bkt += n
            else:
                bkt += min(exact + int(math.floor(math.log(n / exact) / math.log(max_distance / exact) * (half_b - exact) + 1e-9)), half_b - 1)
            out[i, j] = bkt
    return out


# (heads, F, max distance): 32 buckets.  The fixture tests/golden/relpos_buckets.pt holds F = 16 and 61 at the models' max distance 32,
# so those two run at 32 against the fixture's table and at 128 like the others, whose table lavie_relpos_buckets builds
RELPOS = [(8, 1, 128), (8, 16, 128), (8, 61, 128), (5, 17, 128), (8, 16, 32), (8, 61, 32)]


@functools.lru_cache(maxsize=None)
def relpos_case(heads, Fr, max_distance, nb=32):
    """out[h, i, j] = float(emb[buckets[i, j], h]).  The wrapper builds the table with lavie_relpos_buckets and writes it over the
    `buckets` operand: the input-unchanged check then says the library's table is the one here (the fixture's where it holds F)."""
    emb = rnd(gen("relpos", heads, Fr, max_distance), nb, heads)
    table = relpos_table(Fr, nb, max_distance)

    def expect():
        if max_distance == 32 and Fr in (16, 61):
            fx = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relpos_buckets.pt"))
            fx = {int(k): v for k, v in fx.items()}
            assert torch.equal(fx[Fr].to(torch.int32), table), "the bucket table differs from tests/golden/relpos_buckets.pt"
        return {"y": emb[table.long()].permute(2, 0, 1).float().contiguous()}
    return move_case(f"fill_relpos_bias[h{heads},F{Fr},d{max_distance}]", {"emb": emb, "buckets": table}, {"y": ((heads, Fr, Fr), f32t)},
                     lambda ops, i, o: ops.fill_relpos_bias(i["emb"], Fr, max_distance, buckets=i["buckets"], out=o["y"]), expect,
                     where=lambda i: "(head %d, query %d, key %d)" % (i // (Fr * Fr), i // Fr % Fr, i % Fr),
                     calls=[call("fill_relpos_bias", heads=heads, F=Fr, num_buckets=nb)])


LN_FOLD = [(1, 64), (5, 320), (130, 320), (64, 1280), (3, 72)]


@functools.lru_cache(maxsize=None)
def ln_fold_case(N, K, with_bias):
    """Wout = fp16(fp32(W gamma)), bit for bit.  s = sum_k Wout[n, k] and b = sum_k beta[k] W[n, k] (+ bias) in fp32: lane l adds
    its ceil(K / 64) terms k = l, l + 64, ... serially, then six butterfly levels, so the summation depth is ceil(K / 64) + 6 and
    c = depth 2^-23 (first order depth 2^-24, doubled); b has one more rounding per term (beta w) and the bias add: depth + 2.
    gemm_c(K) would be ~30 times looser at K = 320 and pass an s summed from the unrounded W gamma."""
    g = gen("ln_fold", N, K, with_bias)
    w = rnd(g, N, K, s=1 / math.sqrt(K))
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    ins = {"w": w, "gamma": gamma, "beta": beta}
    if with_bias:
        ins["bias"] = rnd(g, N, s=0.3)
    wout = (w.float() * gamma).half()
    depth = -(-K // 64)

    def run(ops, i, o):
        ops.ln_fold(i["w"], i["gamma"], i["beta"], i.get("bias"), w_out=o["wout"], s_out=o["s"], b_out=o["b"])

    def ref():
        bb = (d(w) * d(beta)).sum(1)
        sb = (d(w) * d(beta)).abs().sum(1)
        if with_bias:
            bb, sb = bb + d(ins["bias"]), sb + d(ins["bias"]).abs()
        return {"wout": (d(wout), torch.zeros(N, K, dtype=f64)), "s": (d(wout).sum(1), d(wout).abs().sum(1)), "b": (bb, sb)}

    def model(unrounded_s=False):
        """unrounded_s: s summed from the fp32 product before its fp16 rounding (an injected defect)"""
        pad = depth * 64 - K
        lanes = lambda t: F.pad(t, (0, pad)).reshape(N, depth, 64)
        ws = lanes(w.float() * gamma if unrounded_s else wout.float())
        wb = lanes(beta * w.float())
        s, b = torch.zeros(N, 64), torch.zeros(N, 64)
        for t in range(depth):
            s, b = s + ws[:, t], b + wb[:, t]
        b = wave_sum32(b)
        return {"wout": wout, "s": wave_sum32(s), "b": b + ins["bias"].float() if with_bias else b}

    case = Case(f"ln_fold[{N}x{K},bias{int(with_bias)}]", ins, {"wout": ((N, K), f16), "s": ((N,), f32t), "b": ((N,), f32t)}, run, ref,
                {"wout": 0.0, "s": (depth + 6) * oc.U32, "b": (depth + 8) * oc.U32}, model,
                {"wout": oc.loc_rows(K), "s": lambda i: f"row {i}", "b": lambda i: f"row {i}"}, u={"wout": 0.0, "s": oc.U32, "b": oc.U32},
                exact={"wout": wout})
    return with_calls(case, [call("ln_fold", N=N, K=K, bias_f16=with_bias)])


GEMV_SMALL = [(1, 1, 8), (2, 31, 320), (8, 33, 1280), (3, 64, 520), (8, 32, 2048)]
GEMV_WIDE = (2, 19840, 320)                       # the engine's stacked time_emb_proj width, once, without activations
GEMV_REFUSED = [(9, 32, 64), (2, 32, 12), (8, 32, 2056)]


@functools.lru_cache(maxsize=None)
def gemv_case(B, N, K, act_in, act_out, with_bias):
    """out[b, n] = act_out(sum_k act_in(x[b, k]) W[n, k] + bias[n]) in fp32.  c = gemm_c(K) on sum |act_in(x) w| + |bias|; the error of
    silu_f (silu_rel) enters relative to |silu(x)|: for act_in through the scale (sum_k |w| |silu(x_k)| silu_rel(x_k)), for act_out on
    the result, whose pre-activation error passes through |silu'| < 1.1.  Batch rows 0 and B - 1 hold the same vector: their
    outputs must have the same bits (the kernel's fixed fma order)."""
    g = gen("gemv", B, N, K, act_in, act_out, with_bias)
    x = rnd(g, B, K, dtype=f32t, s=1.5)
    x[B - 1] = x[0]
    w = rnd(g, N, K, s=1 / math.sqrt(K))
    ins = {"x": x, "w": w}
    if with_bias:
        ins["bias"] = rnd(g, N, dtype=f32t, s=0.5)
    c = oc.gemm_c(K)

    def run(ops, i, o):
        ops.gemv(i["x"], i["w"], i.get("bias"), act_in=act_in, act_out=act_out, out=o["y"])

    def ref():
        xa = silu64(d(x)) if act_in else d(x)
        pre, sc = xa @ d(w).t(), xa.abs() @ d(w).abs().t()
        extra = (xa.abs() * silu_rel(d(x))) @ d(w).abs().t() if act_in else torch.zeros_like(sc)
        if with_bias:
            pre, sc = pre + d(ins["bias"]), sc + d(ins["bias"]).abs()
        if act_out:
            y = silu64(pre)
            return {"y": (y, 1.1 * (sc + extra / c) + y.abs() * silu_rel(pre) / c)}
        return {"y": (pre, sc + extra / c)}

    def model(row_from=None, clamp_spill=False):
        """row_from: {b: b'} — batch row b reads row b''s staged vector (an injected defect)"""
        xs = silu32(x) if act_in else x.clone()
        for bdst, bsrc in (row_from or {}).items():
            xs[bdst] = xs[bsrc]
        trips = -(-K // 512)
        xl = F.pad(xs, (0, trips * 512 - K)).reshape(B, 1, trips, 64, 8).double()
        wl = F.pad(w.float(), (0, trips * 512 - K)).reshape(1, N, trips, 64, 8).double()
        acc = torch.zeros(B, N, 64)
        for t in range(trips):
            for j in range(8):
                acc = (acc.double() + xl[:, :, t, :, j] * wl[:, :, t, :, j]).float()           # one fma: the product is exact in float64
        y = wave_sum32(acc)
        if with_bias:
            y = y + ins["bias"]
        return {"y": silu32(y) if act_out else y}

    def post(got):
        if B > 1:
            y = got["y"].detach().cpu()
            assert torch.equal(y[0].view(torch.int32), y[B - 1].view(torch.int32)), \
                f"gemv[{B}x{N}x{K}]: batch rows 0 and {B - 1} hold one input vector but differ in {(y[0] != y[B - 1]).sum()} outputs"

    case = Case(f"gemv[{B}x{N}x{K},in{int(act_in)},out{int(act_out)},bias{int(with_bias)}]", ins, {"y": ((B, N), f32t)}, run, ref, c, model,
                oc.loc_rows(N), u=oc.U32, post=post)
    return with_calls(case, [call("gemv", B=B, N=N, K=K, act_in=act_in, act_out=act_out, bias=with_bias)])


SINUSOID = [(1, 2), (2, 256), (8, 320)]
TIMESTEPS = [0.0, 1.0, 999.0, 500.5, 0.001]
# c_t: the relative error of the fp32 argument a = t w_k, counted in units of 2^-23 from timestep_sinusoid_kernel's source,
#   w = expf(-logf(10000.0f) * (float)k / (float)half_dim):  z = the exponent, |z| <= ln 10000 = 9.22
#     logf, 1 ulp in the HIP math API's table, taken as 2:  2        the product with k: 0.5        the divide: 1       -> 3.5 relative in z,
#     3.5 * 9.22 = 32.3 absolute, which is the relative error it leaves in w;  expf, 1 ulp in the table, taken as 2:  2   -> 34.3
#   a = t * w: 0.5  -> 34.8, counted as 35; doubled for the second-order terms: c_t = 70 * 2^-23 = 8.3e-6.
# |cos(a') - cos(a)| <= |a' - a| <= c_t |a|, and cosf / sinf's own 2 ulp of a value <= 1 are below c_t * 1: bound (1 + |a|) c_t + U32 |ref|.
# A frequency index off by one moves a by 6 % at dim = 320, four orders of magnitude above c_t.
SINUSOID_CT = 70 * oc.U32


@functools.lru_cache(maxsize=None)
def sinusoid_case(B, dim):
    half = dim // 2
    t = torch.tensor([TIMESTEPS[i % len(TIMESTEPS)] for i in range(B)] if B > 1 else [999.0], dtype=f32t)
    if B == 8:
        t[5:] = torch.tensor([37.0, 250.25, 980.0])

    def angle(cv, shift=0):
        k = torch.arange(half) + shift
        return cv(t)[:, None] * torch.exp(-math.log(10000.0) * cv(k) / half)[None]

    def ref():
        a = angle(d)
        return {"y": (torch.cat([a.cos(), a.sin()], 1), torch.cat([1 + a.abs(), 1 + a.abs()], 1))}

    def model(swap=False, shift=0):
        k = (torch.arange(half) + shift).float()
        wk = torch.exp(-torch.log(torch.tensor(10000.0)) * k / float(half))
        a = t[:, None] * wk[None]
        return {"y": torch.cat([a.sin(), a.cos()] if swap else [a.cos(), a.sin()], 1)}

    case = Case(f"timestep_sinusoid[{B}x{dim}]", {"t": t}, {"y": ((B, dim), f32t)}, lambda ops, i, o: ops.timestep_sinusoid(i["t"], dim, out=o["y"]),
                ref, SINUSOID_CT, model, oc.loc_rows(dim), u=oc.U32)
    return with_calls(case, [call("timestep_sinusoid", B=B, dim=dim)])


CLASS_EMB = [(1, 8, (4,)), (3, 1024, (0, 4, 4)), (8, 1280, (0, 4, 2, 2, 1, 3, 0, 4))]
CLASS_EMB_REFUSED = [(2, 8, (0, 5)), (2, 8, (-1, 0)), (9, 8, (0,) * 9)]


@functools.lru_cache(maxsize=None)
def class_emb_case(B, N, labels, classes=5):
    """emb = silu(emb + table[label]) in place: one fp32 add (2^-24 of the sum, doubled: c = 2^-23 on |emb| + |table|, through
    |silu'| < 1.1) and silu_f's own error relative to the result."""
    g = gen("class_emb", B, N, labels)
    emb, table = rnd(g, B, N, dtype=f32t, s=1.5), rnd(g, classes, N)
    lab = torch.tensor(labels)

    def ref():
        x = d(emb) + d(table)[lab]
        y = silu64(x)
        return {"y": (y, 1.1 * (d(emb).abs() + d(table)[lab].abs()) + y.abs() * silu_rel(x) / oc.U32)}

    case = Case(f"add_class_emb_silu[{B}x{N}]", {"emb": emb, "table": table}, {"y": ((B, N), f32t)},
                lambda ops, i, o: ops.add_class_emb_silu(o["y"], i["table"], labels), ref, oc.U32,
                lambda: {"y": silu32(emb + table.float()[lab])}, oc.loc_rows(N), alias={"y": "emb"}, u=oc.U32)
    return with_calls(case, [call("add_class_emb_silu", B=B, N=N, num_classes=classes)])


def ends_cases():
    """The cases of tests/test_gpu_ends_local.py, by family"""
    fam = {}
    fam["conv_out"] = [conv_out_case(ci, co, gm) for ci, co in CONV_OUT_SHAPES for gm in GEOMS]
    fam["conv_in"] = [conv_in_case(ci, co, gm) for ci, co in CONV_IN_SHAPES if conv_in_fits(ci, co) for gm in GEOMS]
    fam["pack"] = ([pack_conv_in_case(ci, co) for ci, co in CONV_IN_SHAPES if conv_in_fits(ci, co)] + [pack_conv_out_case(*s) for s in PACK_CONV_OUT_SHAPES]
                   + [pack_geglu_vec_case(n) for n in (32, 64, 2560)] + [copy_rows_case(*s) for s in COPY_ROWS]
                   + [f16_to_f32_case(n, two) for n in (1, 255, 256, 257) for two in (False, True)])
    fam["ln_fold"] = [ln_fold_case(n, k, wb) for n, k in LN_FOLD for wb in (False, True)]
    fam["gemv"] = ([gemv_case(*s, ai, ao, wb) for s in GEMV_SMALL for ai in (False, True) for ao in (False, True) for wb in (True, False)]
                   + [gemv_case(*GEMV_WIDE, False, False, True)])
    fam["timestep_sinusoid"] = [sinusoid_case(*s) for s in SINUSOID]
    fam["add_class_emb_silu"] = [class_emb_case(*s) for s in CLASS_EMB]
    fam["fill_relpos_bias"] = [relpos_case(*s) for s in RELPOS]
    for cs in fam.values():
        for c in cs:
            c.variants = ("auto",)                 # none of these kernels depends on the GEMM choice: replayed once
    return fam


def restricted(case, variants):
    case.variants = variants
    return case


def reach_cases():
    """The cases of the reach tables (REACH_*), each with the variants it runs under"""
    cs = [restricted(linear_case(M, N, K, o), v) for M, N, K, o, v in REACH_LINEAR]
    cs += [restricted(lnfold_case(M, N, K), v) for M, N, K, v in REACH_LNFOLD]
    cs += [restricted(geglu_case(M, c), v) for M, c, v in REACH_GEGLU]
    cs += [restricted(lnfold_geglu_case(M, c), v) for M, c, v in REACH_LNFOLD_GEGLU]
    cs += [restricted(temporal_conv_case(*s), v) for *s, v in REACH_TCONV]
    return cs


def deep_cases():
    """The cases at model depth (tests/test_gpu_ops_local.py::test_deep_reduction_case): 80 K-tiles under the automatic split and unsplit
    on each kernel; unequal multi-slab segments under forced splits, on the gather kernels and on the halo-patch kernel"""
    cs = [restricted(linear_case(M, N, K, o), v) for M, N, K, o, v in DEEP_LINEAR]
    cs += [linear_case(160, 320, 5120, "bias_residual", force=f) for f in DEEP_UNSPLIT]
    cs += [conv_case(**SEG_SC, force=t, splits=s) for t, s in SEG_FORCED]
    cs += [conv_case(**k, force=5, splits=s) for k in HALO_SEG_CASES for s in HALO_SEG_SPLITS]
    return cs


def gemm_family_cases():
    """Every case that describes its C-ABI calls: what gemm_reach replays (the halo-patch cases under both of their forced loops)"""
    cs = [c for c in all_cases() if c.calls]
    return cs + [conv_case(**k, force=3) for k in HALO_CASES] + list(stats_cases()) + list(stats_local_cases())


def vae_cases():
    """The cases of tests/test_gpu_vae_local.py: the autoencoder's kernels past one workgroup / one grid-stride step, GroupNorm at its width"""
    cs = wide_past_cases()
    cs += [edge_out_case(*e) for e in EDGE_OUT_PAST] + [edge_in_case(*e) for e in EDGE_IN_PAST]
    return cs + [group_norm_case(**k) for k in GN_VAE]


def all_cases():
    """Every case both test files run (the host file: the model of each against its own bound)."""
    cs = [linear_case(*s, o) for s in LINEAR_SHAPES for o in LINEAR_OPTIONS]
    cs += [geglu_case(129, 64), geglu_case(154, 320), lnfold_case(154, 320, 320), lnfold_case(161, 192, 64)]
    cs += reach_cases()
    cs += [conv_case(**k) for k in CONV_CASES]
    cs += [conv_case(**k, force=5) for k in HALO_CASES]            # force = 3 has the same model and reference
    cs += [conv_case(n=n, c1=c, cout=c, h=h, w=w, ups=1, parity=True) for n, c, h, w in PARITY_CASES]
    cs += [restricted(parity_case(n, c, h, w), ("auto",)) for n, c, h, w, _ in PARITY_SPLIT_CASES] + deep_cases()
    cs += [temporal_conv_case(*s, t) for s in TCONV_SHAPES for t in (3, 5)] + [temporal_conv_case(*s, t, force=5) for s in TCONV_FORCED for t in (3, 5)]
    cs += [edge_in_case(*e, dt, tap) for e in EDGE_IN for dt in (f16, f32t) for tap in (False, True)]
    cs += [edge_out_case(*e, dt) for e in EDGE_OUT for dt in (f16, f32t)]
    cs += [group_norm_case(**k) for k in GN_CASES + GN_PAST_SLAB]
    cs += vae_cases()
    cs += [layer_norm_case(*s) for s in LN_CASES]
    cs += [attention_case(*s) for s in SELF_ATTN]
    cs += [attention_case(3, 40, 320, lk=lk, kv_div=div) for lk, div in CROSS_ATTN]
    cs += [attention_case(1, l, c, heads=1) for l, c in WIDE_ATTN]
    cs += [sparse_causal_case(*s) for s in SPARSE_CAUSAL]
    cs += attention_hard_cases()
    cs += temporal_attention_cases()
    cs += [geglu_mlp_case(M, False) for M in (1, 129)] + [cross_block_case(*sh, False) for sh in CROSS_BLOCKS]
    cs += [temporal_block_case(1, 1, False), temporal_block_case(2, 13, False), temporal_block_case(2, 13, False, profile="peaked")]
    cs += [proj_qkv_case(nb, dd) for nb in (1, 5) for dd in (16, 48)]
    cs += multi_pass_cases()
    cs += [step_case(k, n) for k in STEP_KINDS for n in STEP_LENGTHS]
    cs += [lora_case(*s, ip) for s in LORA_SHAPES for ip in (False, True)]
    # the forward's ends and glue kernels (tests/test_gpu_ends_local.py)
    cs += [c for fam in ends_cases().values() for c in fam]
    return cs


# ------------------------------------------------------------------ producer-side norm statistics (tests/statcheck.py, tests/test_gpu_stats_local.py)
# A GEMM-family case run once more with the statistics sink of lavie_debug_op_statistics armed: "cs" column statistics (what a consuming
# GroupNorm folds), "rs" row statistics (what a consuming LayerNorm finalizes), "cs+rs" both, as the engine's proj_out runs.  C is
# checked against the case's own float64 reference under its own bound, the partials against float64 sums of the C that was written.
# (base case, kind, variants): the variants whose plan (`hostcheck optrace`, asserted by test_gemm_reach_host.py) is the kernel named.
def _lin(M, N, K, o):
    return lambda: linear_case(M, N, K, o)


def _cv(**k):
    return lambda: conv_case(**k)


STATS_TABLE = [
    # 128-row kernel, ragged M: 64-, 160- and 128-wide tiles (one wave tile of the last row tile lies past M: a padding block)
    (_lin(130, 192, 64, "bias2"), "cs", ("auto",)), (_lin(154, 320, 320, "bias_residual"), "cs", ("row128-tiles",)),
    (_lin(8193, 512, 64, "bias_residual"), "cs", ("auto",)),
    # ping-pong kernel, plain (M = 154: two blocks; M = 161: three announced, four stored) and gather
    (_lin(154, 320, 320, "residual_in_place"), "cs", ("pingpong",)), (_lin(161, 320, 320, "bias2"), "cs", ("pingpong",)),
    (_cv(n=1, c1=64, cout=320, h=5, w=7), "cs", ("pingpong",)),
    # persistent kernel at 160 and 320 rows, both tile widths, with and without residual and LayerNorm fold
    (_lin(160, 320, 320, "plain"), "cs", ("ppx-persistent",)), (_lin(160, 320, 320, "bias_residual"), "cs", ("ppx-persistent",)),
    (_lin(320, 256, 320, "bias_residual"), "cs", ("ppx-persistent",)), (_lin(320, 256, 320, "plain"), "cs", ("ppx-persistent",)),
    (lambda: lnfold_case(320, 320, 320), "cs", ("ppx-persistent",)), (lambda: lnfold_case(160, 256, 320), "cs", ("ppx-persistent",)),
    # ... and past its cap of 256 workgroups: a second and a steady-state tile finish with the counted statistics stores in flight
    (_lin(20640, 1280, 320, "bias_residual"), "cs", ("auto",)), (_lin(20640, 640, 320, "plain"), "cs", ("auto",)),
    (_lin(20640, 1024, 320, "bias_residual"), "cs", ("auto",)), (_lin(20640, 512, 320, "plain"), "cs", ("auto",)),
    (lambda: lnfold_case(13760, 960, 320), "cs", ("auto",)), (lambda: lnfold_case(20640, 512, 320), "cs", ("auto",)),
    # gathered A on the 128-row kernel: stride 2, folded upsample, fused shortcut, the downsampler's pad, the 128-wide tile
    (_cv(n=2, c1=64, cout=64, h=5, w=7, stride=2), "cs", ("auto",)), (_cv(n=3, c1=64, cout=128, h=4, w=6, ups=1), "cs", ("auto",)),
    (_cv(n=2, c1=64, c2=64, cout=64, h=3, w=5, csc=64), "cs", ("auto", "row128-tiles")),
    (_cv(n=1, c1=128, cout=128, h=13, w=18, stride=2, pad=(0, 1)), "cs", ("auto",)), (_cv(n=1, c1=64, cout=512, h=91, w=91), "cs", ("auto",)),
    (_cv(n=1, c1=64, cout=320, h=5, w=7), "cs", ("row128-tiles",)),
    # split-K: the reduce kernel with statistics writes C (32-row blocks; 2689 = 84 * 32 + 1), plain and conv
    (_lin(2689, 512, 192, "bias2_residual"), "cs", ("split-k-3",)), (_cv(n=1, c1=64, cout=512, h=52, w=52), "cs", ("split-k-3",)),
    # the 256-wide ping-pong tile by its grid rule, plain and on the temporal gather (the reach table's shapes)
    (_lin(34721, 256, 640, "plain"), "cs", ("auto",)), (lambda: temporal_conv_case(1, 128, 256, 8, 4341, 5), "cs", ("auto",)),
    # the temporal gather on the 128-row kernel, unsplit and through the reduce; the parity form (four sets of source-row blocks)
    (lambda: temporal_conv_case(2, 64, 128, 8, 80, 3), "cs", ("auto", "split-k-3")), (lambda: temporal_conv_case(3, 128, 64, 2, 7, 5), "cs", ("auto",)),
] + [((lambda n=n, c=c, h=h, w=w: conv_case(n=n, c1=c, cout=c, h=h, w=w, ups=1, parity=True)), "cs", ("auto",)) for n, c, h, w in PARITY_CASES] + [
    # the parity form under split-K: the reduce writes the statistics, 32-row blocks of output rows in one set
    ((lambda n=n, c=c, h=h, w=w: parity_case(n, c, h, w)), "cs", ("auto",)) for n, c, h, w, _ in PARITY_SPLIT_CASES] + [
    # row statistics: each slot width (bn / 2 of the 128-row kernel: 32, 80, 64; bn / 4 of the ping-pong and persistent kernels: 80, 64)
    (_lin(130, 192, 64, "plain"), "rs", ("auto",)), (_lin(154, 320, 320, "bias_residual"), "rs", ("row128-tiles",)),
    (_lin(8193, 512, 64, "bias_residual"), "rs", ("auto",)), (_lin(161, 320, 320, "plain"), "rs", ("pingpong",)),
    (_lin(34721, 256, 640, "plain"), "rs", ("auto",)), (_lin(160, 320, 320, "bias_residual"), "rs", ("ppx-persistent",)),
    (_lin(320, 256, 320, "plain"), "rs", ("ppx-persistent",)), (_lin(20640, 640, 320, "plain"), "rs", ("auto",)),
    (_lin(2689, 512, 192, "bias_residual"), "rs", ("split-k-3",)),          # armed row statistics: planned unsplit under forced split-K
    # both kinds in one launch
    (_lin(160, 320, 320, "residual_in_place"), "cs+rs", ("ppx-persistent",)), (_lin(161, 320, 320, "bias_residual"), "cs+rs", ("pingpong", "auto")),
    (_lin(20640, 1280, 320, "residual_in_place"), "cs+rs", ("auto",)),
]
# the halo-patch kernel's modes (each case forces its own kernel): whole-row tiles, 2-D tiles, split-K over slabs, temporal taps 3 / 5
STATS_FORCED = ([_cv(**k, force=5) for k in HALO_CASES]
                + [(lambda s=s, t=t: temporal_conv_case(*s, t, force=5)) for s in TCONV_FORCED for t in (3, 5)])


def with_stats(base, kind, variants=None):
    """`base` run with the statistics sink armed.  The outputs "cs" / "rs" are not in `outputs`: their sizes are the plan's, which
    depends on the variant (statcheck: ops.op_statistics(plan=...) on the GPU, the "## stats" line of the replay on the host)."""
    import copy
    c = copy.copy(base)
    c.__dict__.pop("ref", None)
    c._ref = lambda: base.ref
    c.base, c.kind = base, kind
    c.name = f"{base.name}+{kind}"
    c.knobs = dict(base.knobs, **{k: 1 for k in (["stats_cs"] if "cs" in kind else []) + (["stats_rs"] if "rs" in kind else [])})
    if variants is not None:
        c.variants = variants
    c.parity = None
    if base.calls[0][0] == "upsample_conv3x3":
        a = base.calls[0][1]
        c.parity = (2 * a["Hi"], 2 * a["Wi"])

    def run(ops, i, o):
        with ops.op_statistics(colstat=o.get("cs"), rowstat=o.get("rs")):
            base.run(ops, i, o)
    c.run = run
    return c


# gn_fold_kernel through lavie_group_norm_stats_f16 on synthetic partials (nb, P, c1, c2, rows, nsets, parity grid of a frame, offset): one
# block per domain and many; one tensor and two with a straddling group (60 channels per group over 1280 + 640); four parity sets; more
# than 4 * 256 items per workgroup (70 blocks x 15..16 quads: the unrolled loop runs twice, its tail clamped); group means at 8 sigma
GN_FOLD = [(2, 64, 320, 0, 64, 1, None, 0.0), (2, 160, 320, 0, 80, 1, None, 0.0), (2, 160, 1280, 640, 80, 1, None, 0.0),
           (1, 2240, 1280, 640, 32, 1, None, 0.0), (2, 320, 320, 0, 80, 4, (16, 20), 0.0), (2, 160, 320, 0, 80, 1, None, 8.0)]
# descriptors that cannot serve the GroupNorm (norm.hip gn_colstat_usable): the two-pass path runs, no producer fold is counted.  C % 4
# != 0 cannot reach the choice: launch_group_norm refuses C % 8 != 0 before it.
GN_UNUSABLE = {"P % span != 0": dict(span=320), "C mismatch": dict(desc_c=640)}
ROWSTAT_FINALIZE = [(M, slots, off) for M in (1, 255, 256, 257) for slots in (1, 2, 4, 5) for off in (0.0, 8.0)]


@functools.lru_cache(maxsize=None)
def gn_fold_case(nb, P, c1, c2, rows, nsets, parity, offset, span=None, desc_c=None):
    """group_norm_case's tensor, reference and bound behind ops.group_norm_stats with host-made partials (fp32 block sums of the fp16
    tensor in a producer's layout: statcheck.model_colstat).  Outputs: y and the scratch whose head holds (mean, rstd)."""
    import statcheck as S
    base = group_norm_case(nb, P, c1, c2, silu=True, eps=1e-5, offset=offset, tag="fold:")
    xs = [base.inputs["x1"]] + ([base.inputs["x2"]] if c2 else [])
    ins = dict(base.inputs)
    set_blocks = nb * P // (rows * nsets)
    plan = {"rows": rows, "sets": nsets, "set_blocks": set_blocks, "contiguous": 1, "blocks_stored": nsets * set_blocks}
    descs = []
    for t, x in enumerate(xs):
        part = S.model_colstat(x, plan, parity=parity)
        if desc_c:                                     # a buffer the wider description fits
            part = torch.cat([part] + [torch.full_like(part, float("nan"))] * (-(-desc_c // x.shape[1]) - 1))
        ins[f"p{t + 1}"] = part
        descs.append((part, x.shape[1], rows, nsets, set_blocks))
    groups = 32

    def run(ops, i, o):
        d = [ops.producer_stats(i[f"p{t + 1}"], desc_c or x.shape[1], rows, nsets, set_blocks, span or rows * nsets) for t, x in enumerate(xs)]
        ops.group_norm_stats(i["x1"], i["gamma"], i["beta"], nb, groups, 1e-5, True, x2=i.get("x2"), cs1=d[0], cs2=d[1] if c2 else None,
                             out=o["y"], ws=o.get("ws"))
    case = Case(f"gn_fold[nb{nb},P{P},{c1}+{c2},rows{rows},sets{nsets},off{offset},span{span},dc{desc_c}]", ins, dict(base.outputs), run,
                lambda: base.ref, base.c, base.model, base.where)
    case.descs, case.gn, case.groups, case.usable = descs, (nb, P, c1 + c2), groups, span is None and desc_c is None
    d = {f"cs{t + 1}_{k}": v for t, x in enumerate(xs) for k, v in dict(C=desc_c or x.shape[1], rows=rows, nsets=nsets, set_blocks=set_blocks, span=span or rows * nsets).items()}
    return local_calls(case, [call("group_norm_stats", C1=c1, C2=c2, NB=nb, P=P, groups=groups, silu=1, x2=bool(c2), **d)])


@functools.lru_cache(maxsize=None)
def rowstat_finalize_case(M, slots, offset, cols=64):
    import statcheck as S
    g = gen("rowstat_finalize", M, slots, offset)
    x = (torch.randn(M, slots * cols, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + offset).half()
    part = S.model_rowstat(x, {"slots": slots, "cols": cols})

    def run(ops, i, o):
        ops.rowstat_finalize(i["p"], slots * cols, 1e-5, out=o["out"])
    case = Case(f"rowstat_finalize[M{M},slots{slots},off{offset}]", {"p": part}, {"out": ((M, 2), f32t)}, run, lambda: {}, 0.0, None,
                lambda i: "(row %d, %s)" % (i // 2, ("mean", "rstd")[i % 2]))
    case.row_len = slots * cols
    return local_calls(case, [call("rowstat_finalize", slots=slots, M=M, row_len=slots * cols)])


def stats_local_cases():
    cs = [gn_fold_case(*s) for s in GN_FOLD] + [gn_fold_case(2, 160, 320, 0, 80, 1, None, 0.0, **kw) for kw in GN_UNUSABLE.values()]
    return cs + [rowstat_finalize_case(*s) for s in ROWSTAT_FINALIZE]


@functools.lru_cache(maxsize=None)
def stats_cases():
    cs = [with_stats(mk(), kind, variants) for mk, kind, variants in STATS_TABLE]
    return cs + [with_stats(mk(), "cs") for mk in STATS_FORCED]


# ------------------------------------------------------------------ which kernels the GEMM-family cases reach
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lavie_amd", "csrc")


def optrace_line(entry, ints, tile, splits, knobs=None):
    return " ".join([entry] + [f"{k}={v}" for k, v in ints.items()] + [f"force_tile={tile}", f"force_splits={splits}"]
                    + [f"{k}={v}" for k, v in (knobs or {}).items()])


def hostcheck(*args):
    """Builds the host-only driver (lavie_amd/csrc/hostcheck: every kernel launch is a record of name, grid, block and LDS) and
    runs one of its modes."""
    r = subprocess.run(["make", "-C", CSRC, "-j", "8", "build_asan/hostcheck"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("building the host-only driver failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build_asan", "hostcheck"), *args], cwd=CSRC, capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0 or " written" not in r.stdout:
        raise RuntimeError(f"hostcheck {args[0]} failed:\n" + r.stdout[-3000:] + r.stderr[-3000:])


def registered_kernels():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.txt")
        hostcheck("kernels", out)
        with open(out) as f:
            return set(f.read().splitlines())


def launch_name(line):
    """a launch line of the stub: "<kernel name> gx,gy,gz bx,by,bz lds"; the name itself holds blanks"""
    return line.rsplit(" ", 3)[0]


def launch_grid(line):
    return tuple(int(v) for v in line.rsplit(" ", 3)[1].split(","))


def gemm_runs(cases):
    """(case, variant name, (tile, splits)) of every replay: a case that forces a mode of its own runs under that alone ("forced"),
    a case with a variant list under those, every other case under all six VARIANTS."""
    runs = []
    for c in cases:
        if c.force is not None:
            runs.append((c, "forced", c.force))
        else:
            runs += [(c, v, VARIANTS[v]) for v in (c.variants or VARIANTS)]
    return runs


def gemm_reach(cases):
    """{(case name, variant): launch lines, or None where the library refused a call} through `hostcheck optrace`: the library's own
    planner on the CPU, given the integers each case's `run` passes."""
    runs = gemm_runs(cases)
    lines = [optrace_line(e, ints, *fs, c.knobs) for c, _, fs in runs for e, ints in c.calls]
    blocks = optrace(lines)
    reach, it = {}, iter(blocks)
    for c, v, _ in runs:
        launches = []
        for _ in c.calls:
            launches += next(it)[1]
        NOTES[(c.name, v)] = [l for l in launches if l.startswith("## ")]
        launches = [l for l in launches if not l.startswith("## ")]
        reach[(c.name, v)] = None if "!! refused" in launches else launches
    return reach


# (case name, variant) -> the "## ..." lines of the last gemm_reach that replayed it: the statistics plan of a launch with the sink
# armed ("## stats ...", statcheck.parse_stats_line), the producer-count delta of a group_norm_stats call ("## fold=n")
NOTES = {}


def optrace(lines):
    """[(line, launch lines)] of `hostcheck optrace` for the given call lines"""
    with tempfile.TemporaryDirectory() as tmp:
        inp, out = os.path.join(tmp, "calls.txt"), os.path.join(tmp, "launches.txt")
        with open(inp, "w") as f:
            f.write("\n".join(lines) + "\n")
        hostcheck("optrace", inp, out)
        with open(out) as f:
            got = f.read().splitlines()
    blocks = []
    for l in got:
        if l.startswith("== "):
            blocks.append((l[3:], []))
        else:
            blocks[-1][1].append(l)
    assert [b[0] for b in blocks] == lines, "optrace output does not follow its input"
    return blocks
