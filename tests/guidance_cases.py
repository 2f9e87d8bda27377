"""Shapes and inputs of the guidance-table tests (test_guidance_host.py, test_gpu_guidance.py).  TEST INFRASTRUCTURE."""
import functools

import torch

import guidance_reference as R

CH = R.CH
# (P, C, inner): per = C inner.  What each reaches (asserted from R.launch_rule in test_guidance_host.py):
SHAPES = {
    "3x420": (3, 4, 105),            # one element per lane; two step blocks per latent, the second ragged; one ragged chunk
    "2x(CH+8)": (2, 1, CH + 8),      # 16-byte route; a second chunk of one vector
    "2x3CH": (2, 4, 3 * CH // 4),    # first, middle and last chunk, all full
    "1x8": (1, 1, 8),                # one vector: fewer elements than lanes
    "base": (1, 4, 163840),          # 1 x 655,360: 320 full chunks
}
SMALL = [k for k in SHAPES if k != "base"]
GUIDANCE = (7.5, 3.0, 9.0)           # per latent; the first P are used
PHI = 0.7
COEFFS = {"five": (1.0206, 0.2041, 0.1234, 0.8803, 0.35), "multistep": (1.0206, 0.2041, 0.1234, 0.8803, 0.45)}
IN_SCALE = 0.8125
LEVEL = (0.9, 0.4)
WINDOWS = dict(P=2, C=4, F=6, L=4, starts=(0, 2), hws=(8, 35))


def per_of(name):
    p, c, inner = SHAPES[name]
    return c * inner


@functools.lru_cache(maxsize=None)
def inputs(name, offset=0.0, seed=0):
    """CPU operands of shape `name`.  eps2 = [negative | prompt] fp16 [2 P, C, inner] with |mean| <= 0.1 std per latent in both the
    prompt half and the guided combination (asserted here in float64; `offset` = 2 moves the means to about 2 std)."""
    p, c, inner = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=g)
    # the prompt prediction = the negative one plus a small difference, as a model's two outputs are; both centred per latent,
    # then moved by `offset` (in units of about one standard deviation, 0.625)
    centred = lambda t: t - t.mean(dim=(1, 2), keepdim=True)
    eu, delta = centred(rnd(p, c, inner)) * 0.6, centred(rnd(p, c, inner)) * 0.03
    eps = (torch.cat([eu, eu + delta]) + offset * 0.625).half()
    d = dict(eps=eps, x=rnd(p, c, inner), aux=rnd(p, c, inner), known=rnd(p, c, inner) * 0.8, noise_known=rnd(p, c, inner))
    m = torch.rand(p, 1, inner, generator=g)
    d["mask"] = torch.where(m < 0.4, torch.zeros_like(m), torch.where(m > 0.7, torch.ones_like(m), m))
    per = c * inner
    if per >= 64:            # the statistics are meaningful: hold the conditioning the table bound assumes
        t = R.terms(eps[:p].reshape(p, per), eps[p:].reshape(p, per), GUIDANCE[:p])
        for k in (0, 2):
            mean, std = t[:, :, k].mean(1), t[:, :, k].std(1)
            ok = (mean.abs() <= 0.1 * std) if offset == 0.0 else ((mean.abs() - 2 * std).abs() <= 0.5 * std)
            assert bool(ok.all()), (name, offset, mean, std)
    return d


@functools.lru_cache(maxsize=None)
def window_inputs(hw, seed=0):
    w = WINDOWS
    g = torch.Generator().manual_seed(2000 + hw + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    shape = (w["P"], w["C"], w["F"], hw)
    return dict(eps=[(rnd(2 * w["P"], w["C"], w["L"], hw) * 0.6).half() for _ in w["starts"]], x=rnd(*shape), aux=rnd(*shape))
