"""The FreeU operator cases (lavie_freeu_f16, lavie_amd/csrc/freeu.hip), shared by tests/test_freeu_host.py (CPU: formula, fp32 model
of the two kernels, injected defects, launch mirror) and tests/test_gpu_freeu_local.py (the kernels).

Reference: diffusers' `fourier_filter` restated with torch.fft in float64 (diffusers is not installed: the formula is
restated, not imported).  Bound per output element of the skip:

    |got - ref64| <= 2^-11 |ref64| + c scale,   scale = |in| + |s - 1| (|S| / (H W)) sum |in|,   c = (terms + K_FREEU) 2^-23

`terms` is the summation depth of the kernels' geometry (slabs a pixel lane walks + 8 + 4 lane folds + the runs the apply kernel folds),
K_FREEU the rounding points counted in freeu.hip.  Nothing in here is measured."""
import functools
import math

import torch

import opcheck as oc
from opcases import call, gen

f16, f32t, f64 = torch.float16, torch.float32, torch.float64

# ------------------------------------------------------------------ the launch geometry of freeu.hip (ops.h kFreeu*, freeu_geom)
SLAB, MAX_RUNS, MIN_RUN_SLABS, SUMS = 32, 8, 4, 7
TILE_C, APPLY_PIXELS = 64, 16
K_FREEU = 32          # per mode: trig factors on the sums side (13) and on the apply side (13), gain, chain and last add (3), rounded up


def cdiv(a, b):
    return -(-a // b)


def geom(H, W):
    """(pixels, slabs, slabs per run, runs) of an H x W image: from the image size alone"""
    P = H * W
    nslabs = cdiv(P, SLAB)
    spr = max(MIN_RUN_SLABS, cdiv(nslabs, MAX_RUNS))
    return P, nslabs, spr, cdiv(nslabs, spr)


def terms(H, W):
    """summation depth: slabs of a run in one register, 8 + 4 lane folds, the runs in the apply kernel"""
    P, nslabs, spr, runs = geom(H, W)
    return min(spr, nslabs) + 8 + 4 + runs


def launches(C_h, C2, NI, H, W, b, s, in_place):
    """[(kernel, grid)] the call enqueues: the mirror of launch_freeu"""
    P, nslabs, spr, runs = geom(H, W)
    skip_mode = 2 if s != 1.0 else (0 if in_place else 1)
    h_cols = C_h if not in_place else (C_h // 2 if b != 1.0 else 0)
    items = (NI * cdiv(P, APPLY_PIXELS) * (C2 // 8) if skip_mode else 0) + NI * P * (h_cols // 8)
    out = []
    if skip_mode == 2:
        out.append(("freeu_sums_kernel", (cdiv(C2, TILE_C), runs, NI)))
    if items:
        out.append(("freeu_apply_kernel", (cdiv(items, 256), 1, 1)))
    return out


# ------------------------------------------------------------------ references in float64
def fourier_filter_fft(x, s):
    """diffusers.utils.torch_utils.fourier_filter(x, threshold=1, scale=s) on [N, C, H, W] float64"""
    H, W = x.shape[-2:]
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - 1:crow + 1, ccol - 1:ccol + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(X * mask, dim=(-2, -1)), dim=(-2, -1)).real


def mode_set(H, W):
    """the filtered block as a set of (ky, kx)"""
    return sorted({(ky % H, kx % W) for ky in (0, -1) for kx in (0, -1)})


def fourier_filter_modes(x, s, drop_sine_of=None):
    """the same by mode sums: out = in + (s - 1) / (H W) sum_k [cos phi_k A_k + sin phi_k B_k]; drop_sine_of: a mode whose sine sum is
    left out (an injected defect)"""
    H, W = x.shape[-2:]
    y = torch.arange(H, dtype=f64).reshape(H, 1)
    xx = torch.arange(W, dtype=f64).reshape(1, W)
    corr = torch.zeros_like(x)
    for k in mode_set(H, W):
        phi = 2 * math.pi * (k[0] * y / H + k[1] * xx / W)
        A = (x * phi.cos()).sum((-2, -1), keepdim=True)
        B = (x * phi.sin()).sum((-2, -1), keepdim=True)
        if k == drop_sine_of:
            B = torch.zeros_like(B)
        corr = corr + phi.cos() * A + phi.sin() * B
    return x + (s - 1) / (H * W) * corr


def images(rows, NI, H, W):
    """rows [(n y x), C] -> [N, C, H, W]"""
    return rows.reshape(NI, H, W, -1).permute(0, 3, 1, 2)


def as_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# ------------------------------------------------------------------ the two kernels in torch fp32
def trig32(H, W):
    """(cx, sx, cy, sy, cxy, sxy) per pixel [P] as the kernels form them: the quotient 2 y / H in fp32, sin / cos of pi times it rounded to
    fp32, the xy mode by the angle sum in fp32"""
    p = torch.arange(H * W)
    y, x = p // W, p % W
    ty = ((2 * y).to(f32t) / torch.tensor(float(H), dtype=f32t)).to(f64) * math.pi
    tx = ((2 * x).to(f32t) / torch.tensor(float(W), dtype=f32t)).to(f64) * math.pi
    cy, sy, cx, sx = ty.cos().to(f32t), ty.sin().to(f32t), tx.cos().to(f32t), tx.sin().to(f32t)
    return cx, sx, cy, sy, cy * cx - sy * sx, sy * cx + cy * sx


def model_sums(skip, NI, H, W, skip_last_slab_of=None):
    """partials [NI, runs, 7, C2] in fp32, in the kernel's order: per pixel lane slab after slab, lanes 8 q .. 8 q + 7 one after the
    other, then q = 0 .. 3.  skip_last_slab_of: an image whose last pixel slab is left out (an injected defect)"""
    P, nslabs, spr, runs = geom(H, W)
    C2 = skip.shape[1]
    x = skip.to(f32t).reshape(NI, P, C2)
    pad = runs * spr * SLAB - P
    x = torch.cat([x, torch.zeros(NI, pad, C2)], 1)
    if skip_last_slab_of is not None:
        x = x.clone()
        x[skip_last_slab_of, (nslabs - 1) * SLAB:] = 0
    one = torch.ones(H * W)
    factors = (one,) + trig32(H, W)
    part = torch.empty(NI, runs, SUMS, C2)
    for m, f in enumerate(factors):
        fpad = torch.cat([f, torch.zeros(pad)]).reshape(1, runs, spr, SLAB, 1)
        t = x.reshape(NI, runs, spr, SLAB, C2) * fpad
        acc = torch.zeros(NI, runs, SLAB, C2)
        for i in range(spr):
            acc = acc + t[:, :, i]
        acc = acc.reshape(NI, runs, 4, 8, C2)
        q = acc[:, :, :, 0]
        for i in range(1, 8):
            q = q + acc[:, :, :, i]
        part[:, :, m] = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
    return part


def model_apply(skip, part, NI, H, W, s, sums_of=None):
    """the filtered skip [rows, C2] fp16 from the partials.  sums_of: image n -> the image whose sums it is filtered with (a defect)"""
    P, nslabs, spr, runs = geom(H, W)
    C2 = skip.shape[1]
    if sums_of:
        part = part.clone()[[sums_of.get(n, n) for n in range(NI)]]
    tot = torch.zeros(NI, SUMS, C2)
    for r in range(runs):
        tot = tot + part[:, r]
    gain = torch.tensor((s - 1.0), dtype=f32t) / torch.tensor(float(P), dtype=f32t)
    live = [1.0, float(W > 1), float(W > 1), float(H > 1), float(H > 1), float(W > 1 and H > 1), float(W > 1 and H > 1)]
    g = [tot[:, m] * (gain * live[m]) for m in range(SUMS)]
    cx, sx, cy, sy, cxy, sxy = (t.reshape(1, P, 1) for t in trig32(H, W))
    corr = g[0].unsqueeze(1).expand(NI, P, C2)
    for f, gm in zip((cx, sx, cy, sy, cxy, sxy), g[1:]):
        corr = f * gm.unsqueeze(1) + corr
    return (skip.to(f32t).reshape(NI, P, C2) + corr).to(f16).reshape(NI * P, C2)


def model_h(h, b, cols=None):
    """h with its first C_h / 2 (or `cols`: an injected defect) channels scaled: fp16(fp32(b) * h)"""
    out = h.clone()
    n = h.shape[1] // 2 if cols is None else cols
    out[:, :n] = (torch.tensor(b, dtype=f32t) * h[:, :n].to(f32t)).to(f16)
    return out


# ------------------------------------------------------------------ cases
SHAPES = [   # (NI, H, W, C_h, C2)
    (2, 1, 1, 32, 32), (2, 1, 2, 32, 32), (2, 2, 2, 32, 32), (2, 3, 1, 32, 32),        # deduplicated mode sets
    (2, 5, 8, 64, 64), (2, 5, 8, 1280, 1280),                                          # base level 3, non-power-of-two H
    (3, 10, 16, 1280, 640),                                                            # base level 2; channel counts differ; image boundaries
    (3, 37, 53, 32, 64),                                                               # ragged slabs, odd sizes
    (2, 40, 64, 64, 64), (1, 80, 128, 64, 64),                                         # VSR sizes: many slabs per image
]
FACTORS = [(1.2, 0.9), (1.6, 0.2), (1.0, 1.5), (1.4, 1.0)]      # (b, s)
DATA = ["normal", "offset8"]
FORMULA_SIZES = [(1, 1), (1, 2), (2, 2), (1, 3), (3, 1), (2, 3), (3, 5), (5, 8), (10, 16), (4, 4), (7, 9), (37, 53)]


class FreeuCase:
    def __init__(self, NI, H, W, C_h, C2, b, s, data, in_place=False):
        self.NI, self.H, self.W, self.C_h, self.C2, self.b, self.s, self.data, self.in_place = NI, H, W, C_h, C2, b, s, data, in_place
        self.name = f"freeu[{NI}x{H}x{W},{C_h}/{C2},b={b},s={s},{data}{',in-place' if in_place else ''}]"
        self.calls = [call("freeu", C_h=C_h, C2=C2, NI=NI, H=H, W=W, b_milli=round(b * 1000), s_milli=round(s * 1000), in_place=int(in_place))]
        self.c = (terms(H, W) + K_FREEU) * oc.U32
        self.inputs = tensors(NI, H, W, C_h, C2, data)
        rows = NI * H * W
        self.outputs = {"h_out": ((rows, C_h), f16), "skip_out": ((rows, C2), f16)}
        self.alias = {"h_out": "h", "skip_out": "skip"} if in_place else {}

    def run(self, ops, i, o):
        ops.freeu(i["h"], i["skip"], self.NI, self.H, self.W, self.b, self.s, out=(o["h_out"], o["skip_out"]))

    @functools.cached_property
    def ref(self):
        """(ref64 of the skip, its scale): the torch.fft form, shared per (shape, data, s)"""
        return skip_ref(self.NI, self.H, self.W, self.C_h, self.C2, self.data, self.s)

    def check(self, got, label=""):
        check_skip(self, got["skip_out"], label)
        check_h(self, got["h_out"], label)

    def model(self):
        i = self.inputs
        part = model_sums(i["skip"], self.NI, self.H, self.W)
        skip = model_apply(i["skip"], part, self.NI, self.H, self.W, self.s) if self.s != 1.0 else i["skip"].clone()
        return {"h_out": model_h(i["h"], self.b) if self.b != 1.0 else i["h"].clone(), "skip_out": skip}

    def where(self, C):
        return oc.loc_image(self.NI, self.H, self.W, C)


@functools.lru_cache(maxsize=None)
def tensors(NI, H, W, C_h, C2, data):
    g = gen("freeu", NI, H, W, C_h, C2)
    rows = NI * H * W
    h, skip = torch.randn(rows, C_h, generator=g), torch.randn(rows, C2, generator=g)
    if data == "offset8":                                # a per-channel mean offset of 8: the constant mode dominates
        h, skip = h + 8.0, skip + 8.0
    return {"h": h.to(f16), "skip": skip.to(f16)}


@functools.lru_cache(maxsize=None)
def skip_ref(NI, H, W, C_h, C2, data, s):
    x = images(tensors(NI, H, W, C_h, C2, data)["skip"].to(f64), NI, H, W)
    ref = fourier_filter_fft(x, s)
    scale = x.abs() + abs(s - 1.0) * (len(mode_set(H, W)) / (H * W)) * x.abs().sum((-2, -1), keepdim=True)
    return as_rows(ref), as_rows(scale.expand_as(x))


def check_skip(case, got, label=""):
    skip = case.inputs["skip"]
    if case.s == 1.0:
        oc.assert_bits(got, skip, where=case.where(case.C2), label=f"{label}{case.name}:skip_out")
        return
    ref, scale = case.ref
    oc.assert_elementwise(got, ref, scale, case.c, where=case.where(case.C2), label=f"{label}{case.name}:skip_out")


def check_h(case, got, label=""):
    """channels below C_h / 2 within one fp16 rounding of fp32(b) * in, every other element bit-equal"""
    h, half = case.inputs["h"], case.C_h // 2
    name = f"{label}{case.name}:h_out"
    got = got.detach().cpu()
    if case.b == 1.0:
        oc.assert_bits(got, h, where=case.where(case.C_h), label=name)
        return
    keep = torch.ones(h.shape, dtype=torch.bool)
    keep[:, :half] = False
    same = got.view(torch.int16) == h.view(torch.int16)
    bad = (keep & ~same).nonzero()
    assert not bad.numel(), f"{name}: {bad.shape[0]} elements at or above channel {half} changed, first at row {int(bad[0][0])}, channel {int(bad[0][1])}"
    exact = torch.tensor(case.b, dtype=f32t).to(f64) * h[:, :half].to(f64)
    err = (got[:, :half].to(f64) - exact).abs()
    bound = oc.U16 * exact.abs() + oc.U32 * exact.abs() + 2.0 ** -25          # the fp32 product, one fp16 rounding (its subnormal step)
    bad = (~(err <= bound)).nonzero()
    assert not bad.numel(), (f"{name}: {bad.shape[0]} scaled elements outside one fp16 rounding, first at row {int(bad[0][0])}, channel {int(bad[0][1])}: "
                             f"got {got[bad[0][0], bad[0][1]].item()!r}, exact {exact[bad[0][0], bad[0][1]].item()!r}")


@functools.lru_cache(maxsize=None)
def case(NI, H, W, C_h, C2, b, s, data, in_place=False):
    return FreeuCase(NI, H, W, C_h, C2, b, s, data, in_place)


def all_cases():
    return [case(*shape, b, s, data) for shape in SHAPES for data in DATA for (b, s) in FACTORS]


def in_place_cases():
    """every shape once in place, with both tensors changed, plus the two one-sided settings on a shape with C_h != C2"""
    cs = [case(*shape, 1.2, 0.9, "normal", True) for shape in SHAPES]
    return cs + [case(3, 10, 16, 1280, 640, b, s, "offset8", True) for (b, s) in ((1.0, 1.5), (1.4, 1.0))]
