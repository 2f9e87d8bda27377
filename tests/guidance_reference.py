"""Test-side float64 model of guidance from a per-latent table (lavie_guidance_table and the `_scaled` steps,
csrc/sampler_guidance.hip), its launch rule, and the published rescale rule.  TEST INFRASTRUCTURE: nothing under lavie_amd/ imports it.

eps2 = [negative | prompt], fp16, P latents of `per` elements.  For latent p:
  e_i = fma(g_p, ec_i - eu_i, eu_i) in fp32; sums of ec, ec^2, e, e^2; both unbiased variances; f_p = phi s_t / s_e + (1 - phi);
  eps_i = f_p e_i, then the plain step of the family.
The checks are split where the kernel chain splits: chunk sums against float64 sums of the same terms, the table against float64
from the sums read back, the step against float64 with the table read back.

Bounds.  Chunk sums: |got - S64| <= (DEPTH + 10) 2^-23 sum|terms|, DEPTH = 8 + 6 + 3 the fp32 summation depth of the moments kernel
(eight elements per lane, a six-level butterfly in the wave, the four waves added in order).  Table: g_p bit-equal to fp32(g_p),
|f_p - f64| <= 2^-22 |f64| (a double computation stored as fp32).  Steps: |got - f64| <= K 2^-24 M with M the sum of term magnitudes
and K twice the number of fp32 roundings, the bound of known_reference.py / window_reference.py with ONE more rounding, the multiply
by f_p: plain forms 8 + 1 (five), 9 + 1 (multistep), 4 + 1 (its history); around known latents 12 + 1, 13 + 1, 6 + 1; over windows
window_reference.bound_k + 2."""
import math

import numpy as np
import torch

CH = 2048                  # kGuidanceChunk: elements of one chunk of the moments kernel
DEPTH = 8 + 6 + 3
U32 = 2.0 ** -24
ROUNDINGS = {"five": 9, "multistep": 10, "history": 5, "known_five": 13, "known_multistep": 14, "known_history": 7}


def f32s(v):
    return float(np.float32(v))


def launch_rule(latents, per):
    """Mirror of the launchers: which form runs and over what grid."""
    vec = per % 8 == 0
    return dict(vector=vec, chunks=-(-per // CH), moments_grid=(-(-per // CH), latents),
                step_grid=(-(-(per // 8 if vec else per) // 256), latents), last_chunk=per - (-(-per // CH) - 1) * CH)


def guided_e32(eu, ec, g):
    """[P, per] fp32 e as the kernels form it: d = fp32(ec - eu) (exact in float64), e = fp32(g d + eu) (g d is exact in float64; the
    sum is rounded twice on rare elements, one fp32 ulp at most, far inside every bound here).  g: [P] or a number."""
    g = torch.as_tensor(g, dtype=torch.float64).reshape(-1, 1).float().double()
    d = (ec.double() - eu.double()).float().double()
    return (g * d + eu.double()).float()


def terms(eu, ec, g):
    """[P, per, 4] float64: the summands ec, ec^2, e, e^2."""
    e = guided_e32(eu, ec, g).double()
    c = ec.double()
    return torch.stack([c, c * c, e, e * e], dim=-1)


def chunk_sums(t):
    """[P, per, 4] -> ([P, chunks, 4] sums, the same of magnitudes)."""
    p, per, _ = t.shape
    pad = -per % CH
    t = torch.cat([t, t.new_zeros(p, pad, 4)], dim=1).reshape(p, -1, CH, 4)
    return t.sum(2), t.abs().sum(2)


def factor64(sums, per, phi):
    """[P, 4] float64 sums -> [P] f in float64.  s_e == 0 gives 1; a NaN sum gives NaN."""
    n = float(per)
    var_t = (sums[:, 1] - sums[:, 0] ** 2 / n) / (n - 1.0)
    var_e = (sums[:, 3] - sums[:, 2] ** 2 / n) / (n - 1.0)
    f = phi * var_t.clamp_min(0).sqrt() / var_e.sqrt() + (1.0 - phi)
    f = torch.where(var_e > 0, f, torch.ones_like(f))
    return torch.where(var_t.isnan() | var_e.isnan(), torch.full_like(f, math.nan), f)


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale):
    """Lin et al. 2023, section 3.4, as diffusers' function of this name states it: per sample, over all other dimensions."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1.0 - guidance_rescale) * noise_cfg


def scaled_eps64(eu, ec, table):
    """([P, per] eps = f (eu + g (ec - eu)) in float64, its magnitude sum) with (g, f) = table[p] read back from the device."""
    g, f = table[:, 0].double().reshape(-1, 1), table[:, 1].double().reshape(-1, 1)
    u, c = eu.double(), ec.double()
    return f * (u + g * (c - u)), f.abs() * (u.abs() + g.abs() * (c.abs() + u.abs()))


def step64(family, eps, m_eps, x, aux, coeffs):
    """The plain step of `family` ("five" / "multistep") from eps in float64.  Returns (x', M, x0, M0)."""
    k_x, k_e, c_x0, c_xt, c4 = (f32s(c) for c in coeffs)
    xd = x.double()
    x0, m0 = k_x * xd - k_e * eps, abs(k_x) * xd.abs() + abs(k_e) * m_eps
    if family == "multistep":
        d, md = (x0 + c4 * (x0 - aux.double()), m0 + abs(c4) * (m0 + aux.double().abs())) if c4 != 0.0 else (x0, m0)
        return c_xt * xd + c_x0 * d, abs(c_xt) * xd.abs() + abs(c_x0) * md, x0, m0
    xn, m = c_xt * xd + c_x0 * x0, abs(c_xt) * xd.abs() + abs(c_x0) * m0
    if c4 != 0.0:
        xn, m = xn + c4 * aux.double(), m + abs(c4) * aux.double().abs()
    return xn, m, None, None


def known64(family, xm, mm, x0, m0, known, mask, noise_known, level):
    """The known-region replacement of sampler_known.hip on top of step64; mask has the element shape."""
    a, s = f32s(level[0]), f32s(level[1])
    kd, md = known.double(), mask.double()
    xk, mk = a * kd + s * noise_known.double(), abs(a) * kd.abs() + abs(s) * noise_known.double().abs()
    sel = lambda fv, pv: torch.where(md == 0, fv, torch.where(md == 1, pv, fv + md * (pv - fv)))
    mag = lambda fm, pm: torch.where(md == 0, fm, torch.where(md == 1, pm, fm + md * (pm + fm)))
    if family != "multistep":
        return sel(xm, xk), mag(mm, mk), None, None
    return sel(xm, xk), mag(mm, mk), sel(x0, kd), mag(m0, kd.abs())


def once_rounded_f16(x, scale):
    return torch.from_numpy((x.detach().cpu().double().numpy() * f32s(scale)).astype(np.float16))


def twice_rounded_f16(x, scale):
    return (x.detach().cpu() * f32s(scale)).half()


def model_input(family, x, scale):
    """[2, ...] the fp16 model input the family's kernel writes from its own fp32 x': both halves the same value."""
    h = (twice_rounded_f16 if family == "multistep" else once_rounded_f16)(x, scale)
    return torch.cat([h, h])


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def window64(family, eps, x, aux, starts, profile, table, coeffs):
    """The windowed step in float64: every window's prediction scaled with (g, f) = table[w][p], then averaged per frame with the
    exact normalised weights, then step64 on the whole clip.  x [P, C, F, hw]; eps[w] fp16 [2 P, C, L, hw]."""
    import window_reference as W
    p, c, frames, hw = x.shape
    fused, m_eps = torch.zeros(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.float64)
    for (w, f), n in W.exact_weights(frames, starts, profile).items():
        e = eps[w][:, :, f - starts[w]]
        v, m = scaled_eps64(e[:p].reshape(p, -1), e[p:].reshape(p, -1), table[w])
        fused[:, :, f] += n * v.reshape(p, c, hw)
        m_eps[:, :, f] += n * m.reshape(p, c, hw)
    return step64(family, fused, m_eps, x, aux, coeffs)


# ------------------------------------------------------------------ the checks, shared by the GPU tests and the injected-defect tests
def check_chunk_sums(partials, eu, ec, g, label=""):
    """partials [P, chunks, 4] (fp32 from the kernel) against float64 sums of the same terms; names latent, chunk and sum."""
    ref, mag = chunk_sums(terms(eu, ec, g))
    err, bound = (partials.double() - ref).abs(), (DEPTH + 10) * 2.0 ** -23 * mag
    bad = ~(err <= bound)
    worst = float((err / bound.clamp_min(1e-300)).max())
    if bool(bad.any()):
        p, c, k = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{label}: chunk sum outside its bound at latent {p}, chunk {c}, sum {'ec ec2 e e2'.split()[k]}: got "
                             f"{float(partials[p, c, k])!r}, float64 {float(ref[p, c, k])!r}; worst |err| / bound {worst:.3g}")
    return worst


def check_latent_sums(sums, eu, ec, g, label=""):
    """sums [P, 4] (the fold's doubles) against float64 sums over the whole latent, same bound on the latent's magnitudes."""
    t = terms(eu, ec, g)
    ref, mag = t.sum(1), t.abs().sum(1)
    bad = ~((sums.double() - ref).abs() <= (DEPTH + 10) * 2.0 ** -23 * mag)
    if bool(bad.any()):
        p, k = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{label}: latent sum outside its bound at latent {p}, sum {'ec ec2 e e2'.split()[k]}: got "
                             f"{float(sums[p, k])!r}, float64 {float(ref[p, k])!r}")


def check_table(table, sums, per, g, phi, label=""):
    """table [P, 2] fp32 from the sums read back: g_p bit-equal to fp32(g_p), |f_p - f64| <= 2^-22 |f64|."""
    want_g = torch.tensor([f32s(v) for v in g], dtype=torch.float32)
    if not torch.equal(table[:, 0].view(torch.int32), want_g.view(torch.int32)):
        raise AssertionError(f"{label}: guidance column {table[:, 0].tolist()} is not fp32 of {list(g)}")
    f64 = factor64(sums.double(), per, f32s(phi))
    err = (table[:, 1].double() - f64).abs()
    bad = ~((err <= 2.0 ** -22 * f64.abs()) | (f64.isnan() & table[:, 1].isnan()))
    if bool(bad.any()):
        p = int(bad.nonzero()[0])
        raise AssertionError(f"{label}: f of latent {p} is {float(table[p, 1])!r}, float64 from the sums {float(f64[p])!r}")
    return float((err / f64.abs()).nan_to_num(0.0).max())
