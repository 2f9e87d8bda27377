"""The cases of the launches only the encoder and FVD objects reach: the pinned GEMM plan of the text encoder, the
vision tower and the mapper (csrc/pinned_linear.h), the BatchNorm-folding conv pack of lavie_r3d_finalize, and the mapper's add_rows.
Shared by tests/test_opcheck_host.py (CPU: injected defects must be rejected) and tests/test_gpu_encoder_launches.py (the kernels).

pinned_linear: float64 A W^T + bias (+ R) on the fp16-rounded operands, scale = the sum of the magnitudes, c = gemm_c(K + 2): K exact
fp16 products summed in fp32, the bias and the residual added in fp32, one store rounding (the u |ref| term).  conv3d_fold_pack and
add_rows are compared bit for bit.  Nothing in here is measured."""
import functools
import math

import numpy as np
import torch

import opcheck as oc
from opcases import d, gen, rnd

f16, f32t = torch.float16, torch.float32

# every (N, K) an encoder hands to pinned_linear: in_proj | out_proj | fc1 | fc2 of a CLIP layer; the mapper's image projection, its
# cross-attention k | v projection and its feed-forward (its C x C and 3C x C launches are the ViT-L ones)
PAIRS = {
    "text ViT-L": [(2304, 768), (768, 768), (3072, 768), (768, 3072)],
    "ViT-H text and the ViT-L/14 tower": [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)],
    "mapper": [(768, 1024), (1536, 768), (2048, 768), (768, 2048)],
    "tiny": [(384, 128), (128, 128), (256, 128), (128, 256)],
}
M_RAGGED = (77, 129)                               # ragged under one 128-row tile, one row past one tile
M_EDGES = (1, 7, 127, 128, 257, 2 * 257)
EDGE_PAIRS = PAIRS["tiny"] + [(768, 768)]
FORMS = ("separate", "alias", "table", "a_block", "c_block", "sigma8")
FORM_PAIRS = [(384, 128), (768, 3072)]             # one small and one production pair
BLOCK = 64                                         # halfs a column block lies from the start of its wider buffer (16-byte aligned)
TABLE_IMAGES = 3                                   # "table": launches per case, one per image, all reading the same position table


class PinnedCase:
    """One launch (form "table": TABLE_IMAGES launches) of ops.pinned_linear; take(outs) is the [M, N] result inside what the call wrote"""

    def __init__(self, name, M, N, K, form, inputs, outputs, run, terms, take, alias=None, partial=None):
        self.name, self.M, self.N, self.K, self.form = name, M, N, K, form
        self.inputs, self.outputs, self.run, self.terms, self.take = inputs, outputs, run, terms, take
        self.alias, self.partial = alias or {}, partial or {}
        self.c = oc.gemm_c(K + 2)
        self.where = oc.loc_rows(N)

    @functools.cached_property
    def ref(self):
        """(ref64, scale64), each [M, N]"""
        return self.terms(False), self.terms(True)

    def check(self, outs, label=""):
        oc.assert_elementwise(self.take(outs), *self.ref, self.c, where=self.where, label=f"{label}{self.name}")

    def model(self):
        """the kernel's arithmetic in torch fp32, rounded once: must meet the case's own bound"""
        return self.terms(False, lambda t: t.float()).half()

    def offenders(self, got):
        ref, scale = self.ref
        return ~((got.double() - ref).abs() <= oc.U16 * ref.abs() + self.c * scale)


@functools.lru_cache(maxsize=None)
def pinned_case(M, N, K, form="separate"):
    """form: "separate" R of its own | "alias" R is C | "table" M rows per image, TABLE_IMAGES images, R the [M, N] column block of one
    wider position table read by every image's launch (ldr != ldc, fewer rows than the batch: image_engine.cpp, the image projection) |
    "a_block" A a column block of a wider buffer (lda > K), NaN beside it | "c_block" C a column block (ldc > N), the columns beside it
    poisoned and required unchanged | "sigma8" three rows of A and of R drawn at 8 sigma"""
    assert form in FORMS
    g = gen("pinned", M, N, K, form)
    images = TABLE_IMAGES if form == "table" else 1
    rows = M * images
    a, w, bias = rnd(g, rows, K), rnd(g, N, K, s=1 / math.sqrt(K)), rnd(g, N, dtype=f32t)
    r = rnd(g, M, N) if form == "table" else rnd(g, rows, N)
    if form == "sigma8":
        hot = sorted({0, M // 2, M - 1})
        a[hot] = (a[hot].float() * 8).half()
        r[hot] = (r[hot].float() * 8).half()
    ins = {"a": a, "w": w, "bias": bias, "r": r}
    outs = {"y": ((rows, N), f16)}
    take = lambda o: o["y"]
    alias = partial = None
    if form == "a_block":
        wide = torch.full((rows, K + 2 * BLOCK), float("nan"), dtype=f16)
        wide[:, BLOCK:BLOCK + K] = a
        ins["a"] = wide
    if form == "table":
        wide = torch.full((M, N + 2 * BLOCK), float("nan"), dtype=f16)
        wide[:, BLOCK:BLOCK + N] = r
        ins["r"] = wide
    if form == "c_block":
        outs = {"y": ((rows, N + 2 * BLOCK), f16)}
        mask = torch.zeros(rows, N + 2 * BLOCK, dtype=torch.bool)
        mask[:, BLOCK:BLOCK + N] = True
        partial = {"y": mask}
        take = lambda o: o["y"][:, BLOCK:BLOCK + N]
    if form == "alias":
        alias = {"y": "r"}

    def run(ops, i, o):
        av = i["a"][:, BLOCK:BLOCK + K] if form == "a_block" else i["a"]
        yv = o["y"][:, BLOCK:BLOCK + N] if form == "c_block" else o["y"]
        if form == "table":
            tab = i["r"][:, BLOCK:BLOCK + N]
            for b in range(images):
                ops.pinned_linear(av[b * M:(b + 1) * M], i["w"], i["bias"], residual=tab, out=yv[b * M:(b + 1) * M])
        else:
            ops.pinned_linear(av, i["w"], i["bias"], residual=i["r"], out=yv)

    def terms(absval, cv=d):
        p = (lambda t: t.abs()) if absval else (lambda t: t)
        return p(cv(a)) @ p(cv(w)).t() + p(cv(bias)) + p(cv(r)).repeat(images if form == "table" else 1, 1)

    return PinnedCase(f"pinned_linear[{M}x{N}x{K},{form}]", rows, N, K, form, ins, outs, run, terms, take, alias, partial)


def ragged_cases():
    return [pinned_case(M, N, K) for pairs in PAIRS.values() for (N, K) in pairs for M in M_RAGGED]


def edge_cases():
    return [pinned_case(M, N, K) for (N, K) in EDGE_PAIRS for M in M_EDGES]


def form_cases():
    return [pinned_case(77, N, K, form) for (N, K) in FORM_PAIRS for form in FORMS]


def pinned_cases():
    seen, out = set(), []
    for c in ragged_cases() + edge_cases() + form_cases():
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


# ------------------------------------------------------------------ conv3d_fold_pack
# (label, cout, cin, (kt, kh, kw)): the geometries of R3D-18's packs; the stem's 441 weights end 7 halfs short of its 448-half row
FOLD_GEOMETRIES = [("3x3x3 64->64", 64, 64, (3, 3, 3)), ("3x3x3 64->128", 128, 64, (3, 3, 3)), ("1x1x1 64->128", 128, 64, (1, 1, 1)),
                   ("stem 3x7x7 3->64", 64, 3, (3, 7, 7)), ("3x3x3 256->512", 512, 256, (3, 3, 3))]
FOLD_EPS = 1e-5
VAR0_CHANNEL, NEG_GAMMA_CHANNEL = 3, 5


def fold_reference(w, gamma, beta, mean, var, eps=FOLD_EPS, use_eps=True, swap=False, via_fp32=False):
    """NumPy, from float32 arrays: scale in double, (w scale) rounded ONCE to fp16 (NumPy converts float64 to float16 directly; torch's
    CPU .half() goes through fp32), laid out [Cout][tap Cin + ci] with zeros behind taps Cin; shift = fp32(beta - mean scale).  The
    keyword arguments inject the defects of tests/test_opcheck_host.py: eps left out, tap and ci exchanged, fp32 as an intermediate
    rounding."""
    cout, cin = w.shape[:2]
    taps = int(np.prod(w.shape[2:]))
    with np.errstate(all="ignore"):                 # (the injected "eps left out" divides by var = 0: inf and NaN are what it should give)
        scale = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + (eps if use_eps else 0.0))
        prod = w.astype(np.float64).reshape(cout, cin, taps) * scale[:, None, None]
        if via_fp32:
            prod = prod.astype(np.float32)
        h = prod.astype(np.float16)
        shift = (beta.astype(np.float64) - mean.astype(np.float64) * scale).astype(np.float32)
    h = h.reshape(cout, taps * cin) if swap else h.transpose(0, 2, 1).reshape(cout, taps * cin)
    kpad = -(-taps * cin // 64) * 64
    out = np.zeros((cout, kpad), np.float16)
    out[:, :taps * cin] = h
    return out, shift


def plant_double_rounding(w, scale, co):
    """One in 2^14 random products rounds differently through fp32 than directly, too few for the small geometries to hold one by
    chance: the first weight of row `co` is moved to the nearest fp32 value (within 2^16 units in the last place: well under 1 % of
    the value) whose double product with the row's scale lies within half an fp32 unit of an fp16 rounding midpoint, on the side the
    tie does not break to."""
    row = w[co].reshape(-1)
    base = int(row[:1].view(np.int32)[0])
    cand = (base + np.arange(-(1 << 16), 1 << 16, dtype=np.int64)).astype(np.int32).view(np.float32)
    p = cand.astype(np.float64) * scale[co]
    hit = np.nonzero(p.astype(np.float16).view(np.uint16) != p.astype(np.float32).astype(np.float16).view(np.uint16))[0]
    assert hit.size, (co, float(row[0]))
    row[0] = cand[hit[np.abs(hit - (1 << 16)).argmin()]]


@functools.lru_cache(maxsize=None)
def fold_case(label):
    """BatchNorm values drawn as r3d_reference.make_r3d18 draws them (running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5), gamma ~
    U(0.5, 1.5), beta ~ N(0, 0.1)), with var = 0 in one channel and gamma < 0 in another; weights N(0, 1 / sqrt(K)) in fp32.  The case
    carries the number of elements that round differently through fp32 than directly: the test asserts it is at least 1."""
    _, cout, cin, kernel = next(gm for gm in FOLD_GEOMETRIES if gm[0] == label)
    g = gen("fold", label)
    k = cin * kernel[0] * kernel[1] * kernel[2]
    w = torch.randn(cout, cin, *kernel, generator=g) / math.sqrt(k)
    mean = torch.randn(cout, generator=g) * 0.1
    var = torch.rand(cout, generator=g) + 0.5
    gamma = torch.rand(cout, generator=g) + 0.5
    beta = torch.randn(cout, generator=g) * 0.1
    var[VAR0_CHANNEL] = 0.0
    gamma[NEG_GAMMA_CHANNEL] = -gamma[NEG_GAMMA_CHANNEL]
    ins = {"w": w, "gamma": gamma, "beta": beta, "mean": mean, "var": var}
    arrays = {name: t.numpy() for name, t in ins.items()}           # (views: planting below changes the tensors too)
    scale = arrays["gamma"].astype(np.float64) / np.sqrt(arrays["var"].astype(np.float64) + FOLD_EPS)
    for co in (0, VAR0_CHANNEL, NEG_GAMMA_CHANNEL):
        plant_double_rounding(arrays["w"], scale, co)
    out, shift = fold_reference(**arrays)
    twice, _ = fold_reference(**arrays, via_fp32=True)
    return {"label": label, "inputs": ins, "arrays": arrays, "out": torch.from_numpy(out), "shift": torch.from_numpy(shift),
            "double_rounding_differs": int((out.view(np.uint16) != twice.view(np.uint16)).sum()), "kpad": out.shape[1], "k": k}


def loc_packed(cin, kpad):
    def loc(i):
        co, kk = divmod(i, kpad)
        return "(cout %d, tap %d, cin %d)" % (co, kk // cin, kk % cin)
    return loc


# ------------------------------------------------------------------ add_rows
ADD_ROWS_SHAPES = [(1, 1, 8), (3, 7, 128), (2, 77, 768), (16, 77, 768)]


@functools.lru_cache(maxsize=None)
def add_rows_case(b, l, c):
    g = gen("add_rows", b, l, c)
    x, pos = rnd(g, b, l, c), rnd(g, l, c)
    return {"inputs": {"x": x, "pos": pos}, "want": (x.float() + pos.float()).half()}
