"""float64 restatement of the two kernels of lavie_amd/csrc/denoise_loss.hip from the same Philox words
(tests/noise_reference.py), and of `snr` / `min_snr_weights`.  Nothing here calls the library."""
import numpy as np

import noise_reference as R

KINDS = ("epsilon", "v_prediction", "sample")
_NOISE = {}


def noise(seed: int, draw: int, per: int, offset=None):
    """float64 [per]: the training noise of one latent; offset = (coef, draw_offset, hw) adds coef times the normal of element e // hw
    of (seed, draw_offset): one value per plane of hw elements."""
    key = (seed, draw, per, None if offset is None or offset[0] == 0.0 else tuple(offset))
    if key not in _NOISE:
        n = R.normal(seed, draw, 0, per)
        if key[3] is not None:
            coef, draw_offset, hw = offset
            assert per % hw == 0
            n = n + float(coef) * np.repeat(R.normal(seed, draw_offset, 0, per // hw), hw)
        n.setflags(write=False)
        _NOISE[key] = n                                          # computed once, shared by the tests, never changed
    return _NOISE[key]


def noisy(x0, seeds, draw, levels, offset=None):
    """float64 [P, per] = a_p x0 + s_p n (levels[p] = (a_p, s_p) as fp32 values); x0 [P, per] of any float dtype."""
    x0 = np.asarray(x0, dtype=np.float64)
    out = np.empty_like(x0)
    for p, seed in enumerate(seeds):
        a, s = (float(v) for v in levels[p])
        out[p] = a * x0[p] + (s * noise(seed, draw, x0.shape[1], offset) if s != 0.0 else 0.0)
    return out


def target(x0, seeds, draw, levels, kind, offset=None):
    """float64 [P, per]: n, a n - s x0, or x0."""
    assert kind in KINDS
    x0 = np.asarray(x0, dtype=np.float64)
    if kind == "sample":
        return x0.copy()
    out = np.empty_like(x0)
    for p, seed in enumerate(seeds):
        a, s = (float(v) for v in levels[p])
        n = noise(seed, draw, x0.shape[1], offset)
        out[p] = n if kind == "epsilon" else a * n - s * x0[p]
    return out


def target_scale(x0, seeds, draw, levels, kind, offset=None):
    """float64 [P, per]: the sum of the magnitudes that are added up into a target element (|n|, |a n| + |s x0|, or |x0|)."""
    x0 = np.abs(np.asarray(x0, dtype=np.float64))
    if kind == "sample":
        return x0
    n = np.abs(np.stack([noise(seed, draw, x0.shape[1], offset) for seed in seeds]))        # |n| with the offset term in it
    if kind == "epsilon":
        return n
    lv = np.asarray(levels, dtype=np.float64)
    return np.abs(lv[:, :1]) * n + np.abs(lv[:, 1:]) * x0


def mse(pred, tgt):
    """float64 [P]: mean over the latent of (pred - target)^2."""
    d = np.asarray(pred, dtype=np.float64) - tgt
    return (d * d).mean(axis=1)


def abar(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02):
    """cumprod(1 - beta) of the linear schedule in float64 from fp32 betas, as the scheduler's fp32 cumprod approximates it."""
    betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
    return np.cumprod(1.0 - betas)


def snr(ab):
    return ab / (1.0 - ab)


def min_snr_weights(snr_, gamma, kind):
    snr_ = np.asarray(snr_, dtype=np.float64)
    m = np.minimum(snr_, gamma)
    return m / snr_ if kind == "epsilon" else m / (snr_ + 1.0)
