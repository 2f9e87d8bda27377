"""Test-side restatement of the sampler step over overlapping frame windows (lavie_window_step, csrc/sampler_window.hip) in float64
and in unfused torch fp32, with the per-element error bound of the fused kernel.  TEST INFRASTRUCTURE: nothing under lavie_amd/
imports it.

Shapes: x / aux [P, C, F, hw] fp32; one eps tensor per window, fp16 [nb, C, L, hw] with nb = 2 P = [negative | prompt] under
guidance (guidance is a number) and nb = P without (guidance is None); window w covers frames [starts[w], starts[w] + L).

The bound |got - f64| <= K * 2^-24 * M per element, with M the sum of term magnitudes and K twice the number of fp32 roundings of
the form spelled out in sampler_window.hip / sampler_element.h (each fma is ONE rounding), for a frame that m windows cover:
  e_w   = fma(g, ec_w - eu_w, eu_w)            sub, fma             2   (the windows' terms sit side by side in the sum: once)
  S     = p_1 + ... + p_m                      m - 1 adds           m - 1   the normalisation
  n_w   = p_w / S                              one division         } 2 per covering window: its weight and its place in
  eps   = fma(n_w, e_w, eps)                   one fma              } the weighted sum
  x0    = fma(-ke, eps, kx x)                  mul, fma             2      -> x0 (the multistep history): 2 + 2 = 4 plain
  D     = fma(cp, x0 - x0_prev, x0)            sub, fma             2      (multistep family)
  x'    = ct x + c0 D                          mul, mul, add        3
  x'   += sigma noise (one fma)                fma                  1      (five-coefficient family)
Plain roundings (what the plain kernel of the family spends): five-coefficient 2 + 2 + 3 + 1 = 8, multistep 2 + 2 + 2 + 3 = 9, its
history 4.  With the windows: roundings(m) = plain + 2 m + (m - 1), K(m) = 2 roundings(m): m = 1 .. 4 gives 20 / 26 / 32 / 38
(five), 22 / 28 / 34 / 40 (multistep), 12 / 18 / 24 / 30 (history).  As in dpm_reference.py each rounding perturbs an intermediate
by at most 2^-24 relative, every intermediate is bounded by the sum of the magnitudes of its terms, and the perturbation reaches
the output multiplied by coefficients M already carries (the normalised weights sum to 1); the factor two covers the second-order
terms and the rounding of the stored result.  The float64 form uses the exact weights p_w / S, so the rounding of the kernel's
own fp32 weights is part of what the bound allows (the normalisation rows above).
The unfused torch fp32 form rounds every multiply and add: guidance 3, S m - 1, per window 1 + 2, x0 3, D 3, x' 3, noise 2: at
m = 1 .. 4 that is 14 / 18 / 22 / 26 (five), 15 / 19 / 23 / 27 (multistep), 9 / 13 / 17 / 21 (history): all below K(m), so the
torch form is held to the same bound, which checks the bound against the reference's own error."""
import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
PLAIN_ROUNDINGS = {"five": 8, "multistep": 9, "history": 4}


def f32s(v):
    """A Python scalar as the fp32 value the C ABI receives."""
    return float(np.float32(v))


def cover_count(frames, length, starts):
    """[F] how many windows cover each frame."""
    return torch.tensor([sum(1 for s in starts if s <= f < s + length) for f in range(frames)])


def bound_k(what, frames, length, starts):
    """[1, 1, F, 1] K per element: twice (plain roundings + 2 m + (m - 1)) for a frame under m windows (module docstring)."""
    m = cover_count(frames, length, starts).double()
    return (2.0 * (PLAIN_ROUNDINGS[what] + 2.0 * m + (m - 1.0))).reshape(1, 1, frames, 1)


def exact_weights(frames, starts, profile):
    """{(w, f): p_w / S in float64} for every (window, covered frame)."""
    length = len(profile)
    out = {}
    for f in range(frames):
        cov = [w for w, s in enumerate(starts) if s <= f < s + length]
        total = sum(float(profile[f - starts[w]]) for w in cov)
        for w in cov:
            out[(w, f)] = float(profile[f - starts[w]]) / total
    return out


def fp32_weights(frames, starts, profile):
    """The same as the kernel forms them: S added in fp32 in window order, one fp32 division per window."""
    length = len(profile)
    out = {}
    for f in range(frames):
        cov = [w for w, s in enumerate(starts) if s <= f < s + length]
        total = np.float32(0.0)
        for w in cov:
            total = np.float32(total + np.float32(profile[f - starts[w]]))
        for w in cov:
            out[(w, f)] = float(np.float32(np.float32(profile[f - starts[w]]) / total))
    return out


def _halves(e, p, guided):
    return (e[:p], e[p:]) if guided else (e, None)


def window_form_f64(family, eps, x, aux, starts, profile, guidance, coeffs):
    """The whole step in float64 from the kernel's own inputs.  Returns (x', M, x0, M0); the last two are None unless family ==
    "multistep" (the history the kernel writes)."""
    k_x, k_e, c_x0, c_xt, c4 = (f32s(c) for c in coeffs)
    guided = guidance is not None
    g = f32s(guidance) if guided else 0.0
    p, _, frames, _ = x.shape
    xd = x.double()
    fused, m_eps = torch.zeros_like(xd), torch.zeros_like(xd)
    for (w, f), n in exact_weights(frames, starts, profile).items():
        eu, ec = _halves(eps[w][:, :, f - starts[w]].double(), p, guided)
        e, mag = (eu + g * (ec - eu), eu.abs() + abs(g) * (ec.abs() + eu.abs())) if guided else (eu, eu.abs())
        fused[:, :, f] += n * e
        m_eps[:, :, f] += n * mag
    x0 = k_x * xd - k_e * fused
    m0 = abs(k_x) * xd.abs() + abs(k_e) * m_eps
    if family == "multistep":
        if c4 != 0.0:
            pd = aux.double()
            d, md = x0 + c4 * (x0 - pd), m0 + abs(c4) * (m0 + pd.abs())
        else:
            d, md = x0, m0
        return c_xt * xd + c_x0 * d, abs(c_xt) * xd.abs() + abs(c_x0) * md, x0, m0
    xn, mag = c_xt * xd + c_x0 * x0, abs(c_xt) * xd.abs() + abs(c_x0) * m0
    if c4 != 0.0:
        xn, mag = xn + c4 * aux.double(), mag + abs(c4) * aux.double().abs()
    return xn, mag, None, None


def torch_form_f32(family, eps, x, aux, starts, profile, guidance, coeffs):
    """The same step composed from plain torch fp32 ops, one rounding per operation.  Returns (x', x0 or None)."""
    k_x, k_e, c_x0, c_xt, c4 = (f32s(c) for c in coeffs)
    guided = guidance is not None
    p, _, frames, _ = x.shape
    fused = torch.zeros_like(x)
    for (w, f), n in fp32_weights(frames, starts, profile).items():
        eu, ec = _halves(eps[w][:, :, f - starts[w]].float(), p, guided)
        e = eu + f32s(guidance) * (ec - eu) if guided else eu
        fused[:, :, f] = fused[:, :, f] + n * e
    x0 = k_x * x - k_e * fused
    if family == "multistep":
        d = x0 + c4 * (x0 - aux) if c4 != 0.0 else x0
        return c_xt * x + c_x0 * d, x0
    xn = c_xt * x + c_x0 * x0
    if c4 != 0.0:
        xn = xn + c4 * aux
    return xn, None


def once_rounded_f16(x, scale):
    """fp16 of the exact product x * scale, rounded once (the five-coefficient family): fp32 x fp32 is exact in float64, and numpy
    converts float64 to float16 directly."""
    prod = x.detach().cpu().double().numpy() * f32s(scale)
    return torch.from_numpy(prod.astype(np.float16))


def twice_rounded_f16(x, scale):
    """fp16 of the fp32 product (the multistep family): what torch's (x * scale).half() gives."""
    return (x.detach().cpu() * f32s(scale)).half()
