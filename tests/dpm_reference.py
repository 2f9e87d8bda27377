"""Test-side restatement of DPM-Solver++ (2M) in float64, written from the formulas (Lu et al. 2022, arXiv:2211.01095, eq. of
Algorithm 2) without importing the product's scheduler, plus the toy problem with a known solution and the per-element error
bound of the fused step kernel.  TEST INFRASTRUCTURE: nothing under lavie_amd/ imports it."""
import math

import numpy as np
import torch


def abar_table(beta_start=1e-4, beta_end=0.02, n=1000, schedule="linear"):
    """fp32 cumulative product as the schedulers build it (the table the reference's DDIM class uses), as float64 numbers."""
    if schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    else:
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).double().numpy()


def leading_timesteps(steps, n=1000, offset=0):
    return [int(t) + offset for t in (np.arange(0, steps) * (n // steps))[::-1]]


def lam(abar):
    return 0.5 * (math.log(abar) - math.log1p(-abar)) if abar < 1.0 else math.inf


def step_constants(ab, timesteps, i, order, final_abar, lower_order_final=True):
    """(alpha_s, sigma_s, c_x0, c_xt, c_prev) of step i: x_t = c_xt x_s + c_x0 D, D = x0_s + c_prev (x0_s - x0_prev)."""
    s = timesteps[i]
    a_s = ab[s]
    a_t = ab[timesteps[i + 1]] if i + 1 < len(timesteps) else final_abar
    alpha_s, sigma_s, alpha_t, sigma_t = math.sqrt(a_s), math.sqrt(1 - a_s), math.sqrt(a_t), math.sqrt(1 - a_t)
    if sigma_t == 0.0:
        return alpha_s, sigma_s, 1.0, 0.0, 0.0
    h = lam(a_t) - lam(a_s)
    c_x0, c_xt = -alpha_t * math.expm1(-h), sigma_t / sigma_s
    last = i == len(timesteps) - 1
    if order == 1 or i == 0 or (last and lower_order_final and len(timesteps) < 15):
        return alpha_s, sigma_s, c_x0, c_xt, 0.0
    h_prev = lam(a_s) - lam(ab[timesteps[i - 1]])
    r = h_prev / h
    return alpha_s, sigma_s, c_x0, c_xt, 1.0 / (2.0 * r)


def gaussian_eps(x, abar, s):
    """The exact noise model for data N(0, s^2 I): eps(x, t) = sigma_t x / (alpha_t^2 s^2 + sigma_t^2)."""
    return math.sqrt(1 - abar) * x / (abar * s * s + (1 - abar))


def gaussian_flow_error(solver_step, timesteps, ab, s):
    """Drives `solver_step(i, t, eps, x) -> x_next` from x_T = sqrt(alpha_T^2 s^2 + sigma_T^2) (so that the exact probability-
    flow solution x_t = x_T sqrt((alpha_t^2 s^2 + sigma_t^2) / (alpha_T^2 s^2 + sigma_T^2)) ends at x_0 = s); returns
    |x_0 - s| / s."""
    a_T = ab[timesteps[0]]
    x = torch.full((4,), math.sqrt(a_T * s * s + (1 - a_T)), dtype=torch.float64)
    for i, t in enumerate(timesteps):
        x = solver_step(i, t, gaussian_eps(x, ab[t], s), x)
    return abs(float(x[0]) - s) / s


def restated_error(steps, order, s, offset=0):
    """The toy problem through this file's own restatement (float64 throughout), final step to abar = 1."""
    ab = abar_table()
    ts = leading_timesteps(steps, offset=offset)
    hist = {}

    def solver_step(i, t, eps, x):
        alpha_s, sigma_s, c_x0, c_xt, c_prev = step_constants(ab, ts, i, order, 1.0)
        x0 = (x - sigma_s * eps) / alpha_s
        d = x0 + c_prev * (x0 - hist["x0"]) if c_prev != 0.0 else x0
        hist["x0"] = x0
        return c_xt * x + c_x0 * d

    return gaussian_flow_error(solver_step, ts, ab, s)


# ---------------------------------------------------------------- the fused kernel's update and its error bound
U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)


def kernel_form_f64(eps_u, eps_c, x, x0_prev, guidance, coeffs):
    """The kernel's update evaluated in float64 from the kernel's own inputs (fp16 eps, fp32 x / history, fp32 scalars).
    eps_c = None: the unguided variant.  Returns (x0, x_next, M0, M) where M0 / M are the magnitude sums that scale the
    rounding-error bound of x0 / x_next (below)."""
    k_x, k_e, c_x0, c_xt, c_prev = (float(np.float32(c)) for c in coeffs)
    g = float(np.float32(guidance))
    eu, xd = eps_u.double(), x.double()
    if eps_c is None:
        eps, m_eps = eu, eu.abs()
    else:
        ec = eps_c.double()
        eps = eu + g * (ec - eu)
        m_eps = eu.abs() + abs(g) * (ec.abs() + eu.abs())
    x0 = k_x * xd - k_e * eps
    m0 = abs(k_x) * xd.abs() + abs(k_e) * m_eps
    if c_prev != 0.0:
        pd = x0_prev.double()
        d = x0 + c_prev * (x0 - pd)
        md = m0 + abs(c_prev) * (m0 + pd.abs())
    else:
        d, md = x0, m0
    xn = c_xt * xd + c_x0 * d
    m = abs(c_xt) * xd.abs() + abs(c_x0) * md
    return x0, xn, m0, m


# Every fp32 evaluation of the update, whatever it fuses, is a chain of at most 12 roundings (eps: sub, mul, add; x0: mul, mul,
# sub; D: sub, mul, add; x': mul, mul, add), fewer where a multiply-add is fused.  Each rounding perturbs its result by at most
# U32 relative, and every intermediate is bounded in magnitude by the sum of the magnitudes of its terms, which is what M0 (for
# x0) and M (for x') add up; a perturbation of an intermediate reaches the output multiplied by the coefficients that M already
# carries.  To first order |fp32 - exact| <= (number of roundings) * U32 * M; 16 instead of 12 (8 instead of 6 for x0) covers
# the second-order terms and the rounding of the fp32 result itself.  The bound is absolute per element, scaled by M: a
# relative bound on x' alone would be meaningless where k_x x - k_eps eps cancels.
X0_ROUNDINGS, XN_ROUNDINGS = 8, 16


def torch_form_f32(eps_u, eps_c, x, x0_prev, guidance, coeffs):
    """The same update in plain torch fp32, one rounding per operation, in the scheduler's `step()` order."""
    k_x, k_e, c_x0, c_xt, c_prev = (float(np.float32(c)) for c in coeffs)
    eu = eps_u.float()
    eps = eu if eps_c is None else eu + float(np.float32(guidance)) * (eps_c.float() - eu)
    x0 = k_x * x - k_e * eps
    d = x0 + c_prev * (x0 - x0_prev) if c_prev != 0.0 else x0
    return x0, c_xt * x + c_x0 * d
