"""Test-side UniPC in float64, written from the paper's derivation (Zhao et al., arXiv:2302.04867, data-prediction form, B(h) = e^h
- 1) without importing the product's scheduler; the Gaussian problem whose probability-flow ODE has a closed form; and the fused
step kernel's per-element update in float64 and in plain fp32 torch.  TEST INFRASTRUCTURE: nothing under lavie_amd/ imports it.

The derivation the code follows.  With lambda = log(alpha / sigma), the exact solution from s to t (h = lambda_t - lambda_s) is
    x_t = (sigma_t / sigma_s) x_s + alpha_t sum_{k >= 0} I_k(h) m^(k)(lambda_s),     I_k(h) = e^{-h} int_0^h e^u u^k / k! du,
m^(k) the k-th derivative of the x0 prediction along lambda.  I_0 = 1 - e^{-h} and, by parts, I_k = h^k / k! - I_{k-1}.  UniPC
replaces the derivative terms by differences at nodes lambda_s + r_j h:  alpha_t I_0 sum_j a_j (m(node_j) - m(s)) / r_j.  Matching
the Taylor coefficients gives  sum_j a_j r_j^{k-1} = k! I_k / (h^k I_0),  k = 1 .. number of nodes.  Where there is ONE node the
published implementation (and diffusers) takes a = 1/2, the limit of the right-hand side as h -> 0, instead of solving.  The
corrector's nodes are the earlier model outputs and the target itself (r = 1); the predictor's are the earlier outputs only."""
import math

import numpy as np
import torch


def abar_table(beta_start=1e-4, beta_end=0.02, n=1000):
    """fp32 cumulative product as the schedulers build it, as float64 numbers."""
    betas = torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    return torch.cumprod(1.0 - betas, dim=0).double().numpy()


def leading_timesteps(steps, n=1000, offset=1):
    return [int(t) + offset for t in (np.arange(0, steps) * (n // steps))[::-1]]


def level(abar):
    """(alpha, sigma, lambda); abar = 1: the end of the run."""
    if abar >= 1.0:
        return 1.0, 0.0, math.inf
    return math.sqrt(abar), math.sqrt(1.0 - abar), 0.5 * (math.log(abar) - math.log1p(-abar))


def integrals(h, count):
    """I_0 .. I_count of the module docstring."""
    out = [-math.expm1(-h)]
    for k in range(1, count + 1):
        out.append(h ** k / math.factorial(k) - out[-1])
    return out


def uni_update(x, base, target, nodes):
    """One UniPC update from `base` = (alpha, sigma, lambda, m) to `target` = (alpha, sigma, lambda) with difference nodes
    [(lambda_j, m_j)].  A target of sigma = 0 (h infinite) has I_0 = 1 and takes no nodes: the update is m itself."""
    _, sig_b, lam_b, m_b = base
    alpha_t, sig_t, lam_t = target
    h = lam_t - lam_b
    if math.isinf(h):
        assert not nodes
        return m_b
    big_i = integrals(h, len(nodes))
    out = (sig_t / sig_b) * x + alpha_t * big_i[0] * m_b
    if not nodes:
        return out
    r = [(lam_j - lam_b) / h for lam_j, _ in nodes]
    if len(nodes) == 1:
        a = [0.5]
    else:
        lhs = np.array([[rj ** k for rj in r] for k in range(len(nodes))], dtype=np.float64)
        rhs = np.array([math.factorial(k) * big_i[k] / (h ** k * big_i[0]) for k in range(1, len(nodes) + 1)], dtype=np.float64)
        a = np.linalg.solve(lhs, rhs)
    diff = sum(float(aj) * (m_j - m_b) / rj for aj, rj, (_, m_j) in zip(a, r, nodes))
    return out + alpha_t * big_i[0] * diff


def x0_of(model_output, x, alpha, sigma, prediction="epsilon"):
    if prediction == "epsilon":
        return (x - sigma * model_output) / alpha
    if prediction == "v_prediction":
        return alpha * x - sigma * model_output
    return model_output


def trajectory(model, x_start, timesteps, ab, order=2, corrector=True, prediction="epsilon", keep=None):
    """Whole-trajectory UniPC: `model(x, t)` is evaluated once per position, at the predicted sample.  Position i >= 1 first
    corrects x_i from the previous corrected sample (order = the order of the predictor that produced x_i), then predicts x_{i+1}
    (order 1 at position 0 and at the last position, whose target is sigma = 0).  keep: a list that receives, per position,
    (x_i, model output, x_i^c, m_i, x_{i+1})."""
    n = len(timesteps)
    lv = [level(ab[t]) for t in timesteps] + [level(1.0)]
    x, x_c_prev, ms, produced_by = x_start, None, [], None
    for i, t in enumerate(timesteps):
        out = model(x, t)
        m = x0_of(out, x, lv[i][0], lv[i][1], prediction)
        x_c = x
        if i >= 1 and corrector:
            earlier = [(lv[i - 1 - j][2], ms[i - 1 - j]) for j in range(1, produced_by)]
            x_c = uni_update(x_c_prev, lv[i - 1] + (ms[i - 1],), lv[i], earlier + [(lv[i][2], m)])
        ms.append(m)
        p = min(order, i + 1, n - i)
        x_next = uni_update(x_c, lv[i] + (m,), lv[i + 1], [(lv[i - j][2], ms[i - j]) for j in range(1, p)])
        if keep is not None:
            keep.append((x, out, x_c, m, x_next))
        x, x_c_prev, produced_by = x_next, x_c, p
    return x


# ---------------------------------------------------------------- the Gaussian problem: data x0 ~ N(mu, s^2) per element
def gaussian_eps(x, abar, mu, s):
    """The exact noise prediction: eps*(x, t) = sigma_t (x - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2)."""
    return math.sqrt(1.0 - abar) * (x - math.sqrt(abar) * mu) / (abar * s * s + (1.0 - abar))


def gaussian_flow(x_start, abar_start, abar, mu, s):
    """The probability-flow ODE's solution at `abar` from x_start at abar_start."""
    var = lambda a: a * s * s + (1.0 - a)      # noqa: E731
    return math.sqrt(abar) * mu + math.sqrt(var(abar) / var(abar_start)) * (x_start - math.sqrt(abar_start) * mu)


GAUSSIAN_S = 0.06


def gaussian_case(seed=0, n=64):
    """(mu, s, x_T draws): per-element means in [-1, 1], one s, standard-normal draws scaled to the start level by the caller.
    s = 0.06: concentrated data.  The end error is linear in the draws, so which solver wins depends on s alone, and on the
    "leading" table of the linear-beta schedule (whose last steps are long in lambda: h = 3.1 from t = 101 to t = 1 at 10 steps)
    the corrector wins at 10, 20 and 40 steps for s <= 0.07 only; for s in 0.1 .. 32 it loses at one of the three step counts at
    least (test_unipc_host.py prints the table, DESIGN 7.22 records it)."""
    g = torch.Generator().manual_seed(seed)
    mu = (torch.rand(n, generator=g, dtype=torch.float64) * 2.0 - 1.0)
    z = torch.randn(n, generator=g, dtype=torch.float64)
    return mu, GAUSSIAN_S, z


def gaussian_end_error(solver, steps, seed=0):
    """`solver(model, x_T, timesteps, ab) -> x_0` on the Gaussian problem -> max |x_0 - closed form| over the elements."""
    ab = abar_table()
    ts = leading_timesteps(steps)
    mu, s, z = gaussian_case(seed)
    a_t = ab[ts[0]]
    x_start = math.sqrt(a_t) * mu + math.sqrt(a_t * s * s + 1.0 - a_t) * z
    want = gaussian_flow(x_start, a_t, 1.0, mu, s)
    got = solver(lambda x, t: gaussian_eps(x, ab[t], mu, s), x_start, ts, ab)
    return float((got - want).abs().max())


# ---------------------------------------------------------------- the fused kernel's update
U32, U64 = 2.0 ** -24, 2.0 ** -53


def _f32(v):
    return float(np.float32(v))


def kernel_form_f64(eps_u, eps_c, x, x_last, m1, m2, guidance, factor, c):
    """The kernel's update in float64 from the kernel's own inputs (fp16 eps, fp32 tensors, fp32 scalars).  eps_c = None: no
    guidance; factor: the table's rescale factor (1 without).  c: (k_x, k_eps, corr, c_l, c_0, c_1, c_2, p_x, p_0, p_1).
    Returns (m, xc, x') and the magnitude sums (M_m, M_c, M_n) that scale their rounding-error bounds."""
    k_x, k_e, corr, c_l, c_0, c_1, c_2, p_x, p_0, p_1 = [bool(v) if j == 2 else _f32(v) for j, v in enumerate(c)]
    g, f = _f32(guidance), _f32(factor)
    eu, xd = eps_u.double(), x.double()
    if eps_c is None:
        eps, m_eps = eu, eu.abs()
    else:
        ec = eps_c.double()
        eps = f * (eu + g * (ec - eu))
        m_eps = abs(f) * (eu.abs() + abs(g) * (ec.abs() + eu.abs()))
    m = k_x * xd - k_e * eps
    mm = abs(k_x) * xd.abs() + abs(k_e) * m_eps
    if corr:
        xc = c_l * x_last.double() + c_0 * m
        mc = abs(c_l) * x_last.double().abs() + abs(c_0) * mm
        if c_1 != 0.0:
            xc, mc = xc + c_1 * m1.double(), mc + abs(c_1) * m1.double().abs()
        if c_2 != 0.0:
            xc, mc = xc + c_2 * m2.double(), mc + abs(c_2) * m2.double().abs()
    else:
        xc, mc = xd, xd.abs()
    xn = p_x * xc + p_0 * m
    mn = abs(p_x) * mc + abs(p_0) * mm
    if p_1 != 0.0:
        xn, mn = xn + p_1 * m1.double(), mn + abs(p_1) * m1.double().abs()
    return (m, xc, xn), (mm, mc, mn)


def torch_form_f32(eps_u, eps_c, x, x_last, m1, m2, guidance, factor, c):
    """The same update in plain torch fp32, one rounding per operation."""
    k_x, k_e, corr, c_l, c_0, c_1, c_2, p_x, p_0, p_1 = [bool(v) if j == 2 else _f32(v) for j, v in enumerate(c)]
    eu = eps_u.float()
    eps = eu if eps_c is None else _f32(factor) * (eu + _f32(guidance) * (eps_c.float() - eu))
    m = k_x * x - k_e * eps
    xc = x
    if corr:
        xc = c_l * x_last + c_0 * m
        if c_1 != 0.0:
            xc = xc + c_1 * m1
        if c_2 != 0.0:
            xc = xc + c_2 * m2
    xn = p_x * xc + p_0 * m
    if p_1 != 0.0:
        xn = xn + p_1 * m1
    return m, xc, xn
