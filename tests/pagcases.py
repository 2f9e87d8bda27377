"""Test-side references of perturbed-attention guidance (PAG).  TEST INFRASTRUCTURE: nothing under lavie_amd/ imports it.

1. The forward.  `patched_oracle(layers, batch, perturbed)` temporarily replaces oracle.unet_fp32.cross_attention, which
   transformer_block looks up as a module global, so nothing under oracle/ changes.  The wrapper applies to the spatial self-attention
   (`ctx is None`, parameter prefix ending in ".attn1.") of a transformer whose prefix is selected the way lavie_unet_set_pag selects
   it.  There it returns the original result with the rows of the perturbed entries replaced by
   F.linear(F.linear(x, to_v), to_out.weight, to_out.bias).  Rows are (b f), so the perturbed rows are the trailing perturbed * f ones.
   The original runs on ALL rows first: the leading entries keep the bits the plain oracle gives them.

2. The steps (lavie_*pag*_step, csrc/sampler_pag.hip) in float64, restated from the fp16 / fp32 inputs:
     e = cfg ? eu + g (ec - eu) : ec;  eps = e + s (ec - ep);  then the family's plain step (guidance_reference.step64).
   Bound per element, derived as DESIGN.md 3a does: |got - f64| <= 2 R 2^-24 M with M the sum of the magnitudes of the terms and R
   the fp32 rounding points of the spelled-out arithmetic.  guidance_reference.py counts 8 for the plain guided five-coefficient
   step, 9 for the multistep step and 4 for its history; PAG adds two in front of them, the difference ec - ep and the fma that
   adds s times it: R = 10, 11, 6.  Without classifier-free guidance two of the counted points (ec - eu and its fma) do not exist:
   the same R is then an upper bound.  Nothing here is measured."""
import contextlib

import torch
import torch.nn.functional as F

import guidance_reference as R

f16, f32t, f64 = torch.float16, torch.float32, torch.float64

# ------------------------------------------------------------------ 1. the forward
WIDTHS, ATTN = (256, 256, 512, 512), (True, True, True, False)          # the reduced base structure of tests/test_gpu_freeu.py
BASE_KW = dict(sample_size=16, block_out_channels=WIDTHS, cross_attention_dim=128)
SEED = 11
FORWARD_CASES = {"F4-16x16": (3, 4, 16, 16, 500), "F3-24x40": (3, 3, 24, 40, 321)}      # B, F, h, w, timestep
# The layer sets, fixed by tests/test_pag_host.py::test_separation_of_the_perturbed_entry: the forward-parity case needs the
# perturbed entry farther than 3 TOL_UNET from its unperturbed twin, which `mid_block` alone (a 2 x 2 / 3 x 5 image at these
# shapes, one block of sixteen) does not give; `mid_block` alone stays as a bit-property case.
LAYERS_PARITY = ("mid_block", "up_blocks.1")
LAYERS_BITS = ("mid_block",)


def selected(prefix: str, layers) -> bool:
    """lavie_unet_set_pag's rule: the transformer's prefix starts with an entry followed by '.' or the end of the name."""
    return any(prefix == e or prefix.startswith(e + ".") for e in layers)


@contextlib.contextmanager
def patched_oracle(layers, batch: int, perturbed: int):
    from oracle import unet_fp32 as O
    orig = O.cross_attention

    def cross_attention(sd, p, x, ctx, heads):
        out = orig(sd, p, x, ctx, heads)
        if ctx is not None or not p.endswith(".attn1.") or perturbed == 0 or not selected(p.split(".transformer_blocks.")[0], layers):
            return out
        n = x.shape[0] // batch * perturbed                   # rows are (b f): the trailing perturbed * f frames
        out = out.clone()
        out[-n:] = F.linear(F.linear(x[-n:], sd[p + "to_v.weight"]), sd[p + "to_out.0.weight"], sd[p + "to_out.0.bias"])
        return out

    O.cross_attention = cross_attention
    try:
        yield
    finally:
        O.cross_attention = orig


def ocfg():
    from oracle import unet_fp32 as O
    return O.UNetConfig(block_out_channels=WIDTHS, cross_attention_dim=128, attn_levels=ATTN)


def base_weights():
    import golden_util as G
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    return G.synth16(spec.param_shapes(UNetConfig(block_out_channels=WIDTHS, cross_attention_dim=128, attn_levels=ATTN)), SEED)


def forward_inputs(name):
    """[neg | prompt | perturbed]: the last two entries are the same latents with the same text, as the pipeline builds them."""
    b, f, h, w, t = FORWARD_CASES[name]
    g = torch.Generator().manual_seed(2000 + f)
    lat = torch.randn(1, 4, f, h, w, generator=g).half()
    neg, pos = torch.randn(1, 77, 128, generator=g).half(), torch.randn(1, 77, 128, generator=g).half()
    return torch.cat([lat] * b).contiguous(), torch.cat([neg] + [pos] * (b - 1)).contiguous(), t


_REFS = {}


def forward_refs(name, layers):
    """(patched oracle output, plain oracle output) for the case, computed once per process and left unchanged."""
    from oracle import unet_fp32 as O
    key = (name, tuple(layers))
    if key not in _REFS:
        sd = _REFS.setdefault("sd", base_weights())
        x, ctx, t = forward_inputs(name)
        if ("plain", name) not in _REFS:
            _REFS["plain", name] = O.unet_forward(sd, x.float(), t, ctx.float(), ocfg())
        with patched_oracle(layers, x.shape[0], 1):
            _REFS[key] = O.unet_forward(sd, x.float(), t, ctx.float(), ocfg())
    return _REFS[key], _REFS["plain", name]


# ------------------------------------------------------------------ 2. the steps
ROUNDINGS = {"five": R.ROUNDINGS["five"] - 1 + 2, "multistep": R.ROUNDINGS["multistep"] - 1 + 2, "history": R.ROUNDINGS["history"] - 1 + 2}
assert ROUNDINGS == {"five": 10, "multistep": 11, "history": 6}          # (guidance_reference counts its multiply by f: the - 1)
U32 = R.U32
GUIDANCE, PAG_SCALE, IN_SCALE = 7.5, 3.0, 0.7312
COEFFS = {"five": (1.0125, 0.1594, 0.0123, 0.9841, 0.0107), "multistep": (1.0125, 0.1594, 0.2113, 0.7894, 0.5)}
LANES, V = 256, 8                                                       # launch geometry of pag_step_kernel's eight-element form
SIZES = {"n8": 8, "n420": 420, "two-workgroups+8": 2 * LANES * V + 8}   # 420: one element per lane, parts at unaligned offsets
FAMILIES, CFGS = ("five", "multistep"), (True, False)


def launch_rule(n):
    """Mirror of launch_pag (sampler_pag.hip): (vector form, workgroups)."""
    vec = n % 8 == 0
    return vec, -(-(n // 8 if vec else n) // LANES)


def step_inputs(name, cfg):
    n = SIZES[name]
    g = torch.Generator().manual_seed(7000 + n + (1 if cfg else 0))
    parts = 3 if cfg else 2
    return dict(eps=torch.randn(parts, n, generator=g).half(), x=torch.randn(n, generator=g) * 1.5,
                aux=torch.randn(n, generator=g))


def pag_eps64(eps, cfg, g, s, swap=False):
    """(eps in float64, its magnitude sum) from the fp16 parts; g, s as the fp32 values the kernel receives.  swap: the injected
    defect, prompt and perturbed parts exchanged."""
    g, s = R.f32s(g), R.f32s(s)
    parts = [p.double() for p in eps]
    eu = parts[0] if cfg else None
    ec, ep = (parts[-1], parts[-2]) if swap else (parts[-2], parts[-1])
    if cfg:
        e, m = eu + g * (ec - eu), eu.abs() + abs(g) * (ec.abs() + eu.abs())
    else:
        e, m = ec, ec.abs()
    return e + s * (ec - ep), m + abs(s) * (ec.abs() + ep.abs())


def step64(family, eps, cfg, x, aux, g, s, swap=False):
    """(x', M, x0, M0) of the whole PAG step in float64."""
    e, m = pag_eps64(eps, cfg, g, s, swap)
    return R.step64(family, e, m, x, aux, COEFFS[family])


def model_input(family, x, scale, parts):
    """[parts, n] the fp16 model input the family's kernel writes from its own fp32 x': every part the same value."""
    h = (R.twice_rounded_f16 if family == "multistep" else R.once_rounded_f16)(x, scale)
    return torch.stack([h.reshape(-1)] * parts)


def pag_scale_at(pag_scale, pag_adaptive_scale, t):
    """diffusers' _get_pag_scale, restated."""
    return max(pag_scale - pag_adaptive_scale * (1000 - t), 0.0)
