"""Per-element operator checking: guard bands around every operand, poisoned outputs, and a bound per output element against
a float64 reference ("Per-element operator checks").  A plain module: the host tests run it on CPU tensors, the GPU
tests on the device.

    |got_i - ref_i| <= u |ref_i| + c scale_i              u = U16 = 2^-11, the unit roundoff of fp16, for an fp16 output;
                                                          u = U32 = 2^-23 for an fp32 one

`scale_i` is the float64 sum of the absolute values of everything that is added up into element i, `c` comes from the operator's
family: (K_terms + 8) 2^-23 for fp32 accumulation of exact fp16 products (gemm_c), n U16 for a path with n fp16 rounding points
(round_c).  Nothing in here is measured."""
import math

import torch

U16 = 2.0 ** -11
U32 = 2.0 ** -23
NAN16 = 0x7E5A               # fp16 quiet NaN with a recognisable payload
NAN32 = 0x7FC5A5A5           # fp32 quiet NaN with a recognisable payload
SENTINEL = 12345.0           # the finite poison (fp16 stores it as 12344)
BAND_BYTES = 64 * 1024       # a multiple of 512: the payload keeps the allocator's alignment

WORST = {}                   # label -> worst observed |err| / bound of a whole-tensor check (reported, never read by an assertion)

_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}
_NAN = {torch.float16: NAN16, torch.float32: NAN32}


def _signed(pattern, dtype):
    bits = 16 if dtype == torch.float16 else 32
    return pattern - (1 << bits) if pattern >= 1 << (bits - 1) else pattern


def gemm_c(k_terms):
    return (k_terms + 8) * U32


def round_c(n):
    return n * U16


class Guarded:
    """A contiguous tensor in the middle of a larger buffer, with a band of a fixed bit pattern on either side.  An int32 tensor
    (an index table) is an input only: it has no poison, and its bands hold 0 whatever `band` says — an index a kernel may read."""

    def __init__(self, shape, dtype, fill=None, data=None, band="nan", device="cuda"):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = math.prod(self.shape)
        esz = 2 if dtype == torch.float16 else 4
        self.lo = BAND_BYTES // esz
        self.hi = BAND_BYTES // esz
        self.nan = _signed(_NAN[dtype], dtype) if dtype in _NAN else None
        self.band_value = self.nan if band == "nan" and self.nan is not None else 0
        self.buf = torch.full((self.lo + self.n + self.hi,), self.band_value, dtype=_INT[dtype], device=device)
        self.bits = self.buf[self.lo:self.lo + self.n]                 # integer view of the payload
        self.t = (self.bits if dtype == torch.int32 else self.bits.view(dtype)).view(self.shape)
        assert self.t.data_ptr() % 512 == self.buf.data_ptr() % 512 and self.t.is_contiguous()
        self.poisoned = None
        if data is not None:
            assert tuple(data.shape) == self.shape and data.dtype == dtype
            self.t.copy_(data)
        elif fill is not None:
            self.poison(fill)
        self.saved = self.bits.clone()

    def poison(self, kind):
        """kind "nan": the NaN bit pattern; "finite": SENTINEL."""
        if kind == "nan":
            self.bits.fill_(self.nan)
        else:
            self.t.fill_(SENTINEL)
        self.poisoned = kind

    def _where(self, off):
        s = f"offset {off} relative to the tensor ({self.n} elements)"
        if len(self.shape) == 2 and self.shape[1] > 0:
            s += f" = row {off // self.shape[1]}, column {off % self.shape[1]}"
        return s

    def check_bands(self, name="tensor"):
        for start, band in ((0, self.buf[:self.lo]), (self.lo + self.n, self.buf[self.lo + self.n:])):
            bad = (band != self.band_value).nonzero()
            if bad.numel():
                off = start + int(bad[0]) - self.lo
                raise AssertionError(f"{name}: guard band damaged in {bad.shape[0]} elements, first at {self._where(off)}, "
                                     f"bits 0x{int(band[int(bad[0])]) & 0xFFFFFFFF:x}")

    def check_unchanged(self, name="tensor"):
        bad = (self.bits != self.saved).nonzero()
        if bad.numel():
            raise AssertionError(f"{name}: input changed in {bad.shape[0]} elements, first at {self._where(int(bad[0]))}")

    def unwritten(self):
        """Elements that still hold the NaN poison pattern."""
        return (self.bits == self.nan).nonzero().flatten()

    def check_written(self, name="output", mask=None):
        """mask (bool, the tensor's shape): the elements the call must write; every other one must still hold the poison."""
        assert self.poisoned == "nan"
        bad = self.unwritten()
        if mask is not None:
            m = mask.reshape(-1).to(self.bits.device)
            bad = ((self.bits == self.nan) & m).nonzero().flatten()
            self.check_untouched(name, mask)
        if bad.numel():
            raise AssertionError(f"{name}: {bad.numel()} elements never written, first at {self._where(int(bad[0]))}")

    def check_untouched(self, name, mask):
        """the elements outside `mask` still hold the poison of this run, bit for bit"""
        m = mask.reshape(-1).to(self.bits.device)
        if self.poisoned == "nan":
            stray = ((self.bits != self.nan) & ~m).nonzero().flatten()
        else:
            stray = ((self.t.reshape(-1) != torch.tensor(SENTINEL, dtype=self.dtype)) & ~m).nonzero().flatten()
        if stray.numel():
            raise AssertionError(f"{name}: {stray.numel()} elements outside the written region were stored to, first at {self._where(int(stray[0]))}")


def guarded(shape, dtype, fill="nan", band="nan", device="cuda"):
    return Guarded(shape, dtype, fill=fill, band=band, device=device)


def guarded_like(cpu_tensor, band="nan", device="cuda"):
    return Guarded(cpu_tensor.shape, cpu_tensor.dtype, data=cpu_tensor.contiguous(), band=band, device=device)


# ------------------------------------------------------------------ index -> location callbacks
def loc_rows(ncols):
    return lambda i: "(row %d, column %d)" % divmod(i, ncols)


def loc_image(f, h, w, c):
    """channels-last rows [(f h w), c]"""
    def loc(i):
        p, ch = divmod(i, c)
        fr, p = divmod(p, h * w)
        return "(frame %d, y %d, x %d, channel %d)" % (fr, p // w, p % w, ch)
    return loc


def loc_nchw(c, h, w):
    def loc(i):
        p, x = divmod(i, w)
        p, y = divmod(p, h)
        return "(frame %d, y %d, x %d, channel %d)" % (p // c, y, x, p % c)
    return loc


def loc_heads(heads, dh):
    def loc(i):
        t, col = divmod(i, heads * dh)
        return "(token %d, head %d, dim %d)" % (t, col // dh, col % dh)
    return loc


def assert_elementwise(got, ref64, scale64, c, where=None, label="", mask=None, u=U16):
    """Every element: |got - ref| <= u |ref| + c scale, u the unit roundoff of the output's format (U16; U32 for an fp32 output).
    No element is left out: `mask` only restricts a SECOND look at a region (halo rows, borders) after the whole tensor has been
    checked by a call without it."""
    got = got.detach().cpu().to(torch.float64).reshape(-1)
    ref = ref64.detach().to(torch.float64).reshape(-1)
    scale = scale64.detach().to(torch.float64).reshape(-1)
    assert got.numel() == ref.numel() == scale.numel(), (got.numel(), ref.numel(), scale.numel())
    bound = u * ref.abs() + c * scale
    err = (got - ref).abs()
    if mask is None and label and got.numel():
        WORST[label] = max(WORST.get(label, 0.0), float((err / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf).max()))
    bad = ~(err <= bound)                                            # a NaN in `got` is an offender
    if mask is not None:
        bad &= mask.reshape(-1)
    n_bad = int(bad.sum())
    if n_bad:
        ratio = torch.where(bad, torch.where(err.isnan(), torch.full_like(err, math.inf), err / bound.clamp_min(1e-300)),
                            torch.zeros_like(err))
        i = int(ratio.argmax())
        loc = where(i) if where else f"index {i}"
        raise AssertionError(f"{label}: {n_bad} of {got.numel()} elements outside the bound; worst at {loc} [flat {i}]: got {got[i].item()!r}, "
                             f"ref {ref[i].item()!r}, |err| {err[i].item():.3e} > bound {bound[i].item():.3e}")


def assert_bits(got, want, where=None, label=""):
    """A pure move or an exact conversion: every element has the bits of `want`."""
    got, want = got.detach().cpu().contiguous(), want.detach().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    bad = (got.view(_INT[got.dtype]).reshape(-1) != want.view(_INT[want.dtype]).reshape(-1)).nonzero().flatten()
    if bad.numel():
        i = int(bad[0])
        loc = where(i) if where else f"index {i}"
        raise AssertionError(f"{label}: {bad.numel()} of {got.numel()} elements differ in their bits; first at {loc} [flat {i}]: got "
                             f"{got.reshape(-1)[i].item()!r}, expected {want.reshape(-1)[i].item()!r}")


def run_guarded(fn, inputs, outputs, alias=None, device="cuda", sync=None, partial=None):
    """Runs fn(ins, outs) twice on guarded operands: NaN-poisoned outputs between NaN bands, then SENTINEL-poisoned outputs with
    zero bands around the inputs.  inputs: name -> CPU tensor; outputs: name -> (shape, dtype); alias: output name -> the input
    it overwrites (aliased operands are not poisoned); partial: output name -> bool mask of the elements the call must write — every
    other element of that output must still hold its poison after either run (a sub-rectangle of a wider buffer: a store into the
    neighbouring columns is the defect).  Checks every band, every input that is not an aliased output, that the NaN
    run wrote every output element, and that both runs agree bit for bit.  Returns name -> CPU tensor of the outputs."""
    alias = alias or {}
    partial = partial or {}
    assert not (set(partial) & set(alias)), "an aliased output is not poisoned: it cannot be partial"
    runs = []
    for poison, band in (("nan", "nan"), ("finite", "zero")):
        gi = {k: guarded_like(v, band=band, device=device) for k, v in inputs.items()}
        go = {k: gi[alias[k]] if k in alias else guarded(shape, dtype, fill=poison, band="nan", device=device)
              for k, (shape, dtype) in outputs.items()}
        try:
            fn({k: g.t for k, g in gi.items()}, {k: g.t for k, g in go.items()})
        except RuntimeError:                      # a refusal: nothing may have been touched on the way out
            if sync:
                sync()
            for k, g in {**gi, **go}.items():
                g.check_bands(f"{k} (refused call)")
            raise
        if sync:
            sync()
        for k, g in {**gi, **go}.items():
            g.check_bands(f"{k} ({poison} poison)")
        for k, g in gi.items():
            if k not in alias.values():
                g.check_unchanged(k)
        if poison == "nan":
            for k, g in go.items():
                if k not in alias:
                    g.check_written(k, mask=partial.get(k))
        else:
            for k, m in partial.items():
                go[k].check_untouched(k, m)
        runs.append({k: torch.where(partial[k].reshape(-1), g.bits.cpu(), torch.zeros_like(g.bits.cpu())) if k in partial else g.bits.cpu().clone()
                     for k, g in go.items()})
        res = {k: g.t.cpu().clone() for k, g in go.items()}
    for k in outputs:
        diff = (runs[0][k] != runs[1][k]).nonzero().flatten()
        if diff.numel():
            g = go[k]
            raise AssertionError(f"{k}: {diff.numel()} elements depend on what surrounds the operands (output poison / input bands), "
                                 f"first at {g._where(int(diff[0]))}")
    return res


def check_case(ops, case, forced=(0, 0), sync=None, device="cuda"):
    """One case of tests/opcases.py through run_guarded and its per-element bound.  forced: the (tile, splits) the caller's fixture
    set, which a case that forces a kernel of its own restores afterwards."""
    def fn(i, o):
        if case.setup is not None:
            with case.setup(tuple(forced)):
                case.run(ops, i, o)
        else:
            case.run(ops, i, o)
    case.check(run_guarded(fn, case.inputs, case.outputs, alias=case.alias, device=device, sync=sync, partial=case.partial))
