"""The cases of the text encoder's checks, shared by tests/test_text_encoder_host.py (CPU: the float64 reference
against transformers, the fp32 models against their own bounds) and tests/test_gpu_text_encoder.py (the kernels and the model).

Bounds are tests/opcheck.py's |got - ref| <= u |ref| + c scale against float64, c from the kernels' rounding points:
  causal attention   n = 2 fp16 roundings (P in front of the PV product, the store) + fp32 accumulation over at most 128 keys and
                     64 dims: round_c(2) + gemm_c(128 + 64)
  activation         n = 1 (the store): round_c(1); scale = the magnitudes added up, |x| / 2 (1 + |erf|) resp. |x| sigmoid, plus
                     fp16's underflow: below 2^-14 a rounding moves a value by up to 2^-25 whatever its size (ACT_TINY)
  embedding          exact: the fp32 sum of two fp16 values, rounded once, is what torch computes: compared bit for bit
Shapes are the smallest that cross the kernel's edges; nothing runs at 12 or 23 layers."""
import functools
import math

import torch

import opcheck as oc

f16, f64 = torch.float16, torch.float64
LOG2E = 1.4426950408889634

ATT_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 77, 128]
ATT_SHAPES = [(1, 1, 64), (3, 4, 32), (2, 12, 64)]           # (NB, heads, dh)
ATT_C = oc.round_c(2) + oc.gemm_c(128 + 64)
ACT_SIZES = [1, 7, 8, 4096 + 3]
ACT_C = oc.round_c(1)
ACT_TINY = 2.0 ** -25 / ACT_C          # added to the scale: c scale then holds half the spacing of fp16's subnormals

TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
MODEL_CONFIGS = {
    "tiny": TINY,
    "dh64-gelu": dict(TINY, num_attention_heads=2, hidden_act="gelu"),
    "vit-l-1layer": dict(TINY, hidden_size=768, intermediate_size=3072, num_hidden_layers=1, num_attention_heads=12),
    "vit-h-1layer": dict(TINY, hidden_size=1024, intermediate_size=4096, num_hidden_layers=1, num_attention_heads=16, hidden_act="gelu"),
}
MODEL_B, MODEL_L = 2, 77


def gen(*seed):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


# ------------------------------------------------------------------ causal attention
def split(t, nb, l, heads, dh):
    return t.reshape(nb, l, heads, dh).permute(0, 2, 1, 3)


def merge(t):
    nb, heads, l, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(nb * l, heads * dh)


def causal_ref(q, k, v, scale):
    """float64: (softmax over j <= i) v and the scale sum_j p_j |v_j|; [nb, heads, l, dh] operands."""
    l = q.shape[-2]
    s = q.to(f64) @ k.to(f64).transpose(-1, -2) * scale
    s = s.masked_fill(torch.ones(l, l, dtype=torch.bool).triu(1), -math.inf)
    p = torch.softmax(s, -1)
    return p @ v.to(f64), p @ v.to(f64).abs()


def causal_model(q, k, v, scale):
    """The kernel's arithmetic in torch fp32: scores in log2 units, the true maximum over the visible keys, exp2, P rounded to fp16,
    the row sum over the rounded P, one rounding at the store."""
    l = q.shape[-2]
    s = (q.float() @ k.float().transpose(-1, -2)) * (scale * LOG2E)
    s = s.masked_fill(torch.ones(l, l, dtype=torch.bool).triu(1), -math.inf)
    p = torch.exp2(s - s.max(-1, keepdim=True).values).half().float()
    return ((p @ v.float()) / p.sum(-1, keepdim=True)).half()


HARD_L = 77


def hard_rows():
    """(far rows: keys 0..63 far below, the matching key at 64..i), (dominant rows: one dominant key at j = i), row 0.  The dominant
    rows lie behind key 63 as well: a dominant key among the first 64 would not be far below the far rows."""
    return [64, 70, 76], [66, 73], [0]


@functools.lru_cache(maxsize=None)
def attention_case(nb, heads, dh, l, pad=0, hard=False):
    """q | k | v packed in rows of 3 heads dh + pad halfs; pad columns are NaN.  hard (l = 77): rows rewritten as hard_rows says,
    every constant exact in fp16."""
    g = gen("causal", nb, heads, dh, l, pad, hard)
    c = heads * dh
    q, k, v = (torch.randn(nb, l, c, generator=g).half() for _ in range(3))
    scale = dh ** -0.5
    if hard:
        assert l == HARD_L
        far, dom, _ = hard_rows()
        u = (torch.randint(0, 2, (c,), generator=g) * 2 - 1).to(f16)
        k[:, :64] = (-1.25 * u.float() + 0.1 * torch.randn(64, c, generator=g)).half()       # q k = -20 dh: -20 sqrt(dh) nats <= -113
        for r in far:
            q[:, r] = 16 * u
            k[:, r] = u                                                                        # the matching key, at 64 .. r
        for r in dom:
            k[:, r] = 3 * q[:, r]                                                              # q k scale = 3 |q|^2 / sqrt(dh) ~ 3 sqrt(dh)
        qh, kh = split(q, nb, l, heads, dh), split(k, nb, l, heads, dh)
        s = qh.to(f64) @ kh.to(f64).transpose(-1, -2) * scale
        assert s[:, :, far, :64].max() < -100, s[:, :, far, :64].max()
        for r in far:
            assert s[:, :, r, r].min() > 0
        for r in dom:
            assert (s[:, :, r, r] - s[:, :, r, :r].max(-1).values).min() > 0, r
    qkv = torch.cat([q, k, v, torch.full((nb, l, pad), math.nan, dtype=f16)], -1).reshape(nb * l, 3 * c + pad)
    heads_of = lambda: tuple(split(t, nb, l, heads, dh) for t in (q, k, v))

    def ref():
        y, sc = causal_ref(*heads_of(), scale)
        return merge(y), merge(sc)

    return dict(qkv=qkv, ref=ref, model=lambda: merge(causal_model(*heads_of(), scale)), nb=nb, heads=heads, dh=dh, l=l, c=c, pad=pad,
                where=oc.loc_heads(heads, dh))


# ------------------------------------------------------------------ activation
def act_input(n):
    """values spanning +-12, with +0 and -0 among them"""
    g = gen("act", n)
    x = (torch.rand(n, generator=g) * 24 - 12).half()
    x[0] = 0.0
    if n > 1:
        x[1] = -0.0
    if n > 4:
        x[2], x[3] = 12.0, -12.0
    return x


def act_ref(x, kind):
    x = x.to(f64)
    if kind == "quick_gelu":
        sg = torch.sigmoid(1.702 * x)
        return x * sg, x.abs() * sg + ACT_TINY
    e = torch.erf(x / math.sqrt(2))
    return 0.5 * x * (1 + e), 0.5 * x.abs() * (1 + e.abs()) + ACT_TINY


def act_model(x, kind):
    x = x.float()
    if kind == "quick_gelu":
        return (x / (1 + torch.exp(-1.702 * x))).half()
    return (0.5 * x * (1 + torch.erf(x * 0.70710678118654752))).half()


# ------------------------------------------------------------------ the model
def synth_state_dict(cfg, seed=0):
    """fp16-rounded random weights under the engine's (classic, `text_model.`-prefixed) keys: N(0, 0.02) matrices as CLIP
    initialises them, scaled up so that attention is not uniform; norms near 1."""
    g = gen("text-sd", tuple(sorted(cfg.items())), seed)
    c, i, v, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["max_position_embeddings"]
    rn = lambda *s, std: (torch.randn(*s, generator=g) * std).half()
    sd = {"text_model.embeddings.token_embedding.weight": rn(v, c, std=0.5),
          "text_model.embeddings.position_embedding.weight": rn(p, c, std=0.2)}
    for n in range(cfg["num_hidden_layers"]):
        pre = f"text_model.encoder.layers.{n}."
        for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[pre + f"self_attn.{proj}.weight"] = rn(c, c, std=1.5 / math.sqrt(c))
            sd[pre + f"self_attn.{proj}.bias"] = rn(c, std=0.1)
        sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"] = rn(i, c, std=1.0 / math.sqrt(c)), rn(i, std=0.1)
        sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"] = rn(c, i, std=1.0 / math.sqrt(i)), rn(c, std=0.1)
        for ln in ("layer_norm1", "layer_norm2"):
            sd[pre + ln + ".weight"], sd[pre + ln + ".bias"] = (1 + 0.1 * torch.randn(c, generator=g)).half(), rn(c, std=0.1)
    sd["text_model.final_layer_norm.weight"] = (1 + 0.1 * torch.randn(c, generator=g)).half()
    sd["text_model.final_layer_norm.bias"] = rn(c, std=0.1)
    return sd


def model_ids(cfg, b=MODEL_B, l=MODEL_L, seed=0):
    return torch.randint(0, cfg["vocab_size"], (b, l), generator=gen("text-ids", b, l, seed))


def reference64(sd, cfg, ids):
    """CLIPTextModel.last_hidden_state in float64, written out: checked against transformers in test_text_encoder_host.py."""
    w = {k[len("text_model."):]: v.to(f64) for k, v in sd.items()}
    c, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    dh = c // heads
    b, l = ids.shape
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (c,), w[p + ".weight"], w[p + ".bias"], cfg["layer_norm_eps"])
    lin = lambda x, p: x @ w[p + ".weight"].t() + w[p + ".bias"]
    x = w["embeddings.token_embedding.weight"][ids] + w["embeddings.position_embedding.weight"][:l]
    mask = torch.ones(l, l, dtype=torch.bool).triu(1)
    for n in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{n}."
        h = ln(x, p + "layer_norm1")
        q, k, v = (lin(h, p + f"self_attn.{t}_proj").reshape(b, l, heads, dh).transpose(1, 2) for t in "qkv")
        s = (q @ k.transpose(-1, -2) * dh ** -0.5).masked_fill(mask, -math.inf)
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b, l, c)
        x = x + lin(a, p + "self_attn.out_proj")
        m = lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")
        m = m * torch.sigmoid(1.702 * m) if cfg["hidden_act"] == "quick_gelu" else 0.5 * m * (1 + torch.erf(m / math.sqrt(2)))
        x = x + lin(m, p + "mlp.fc2")
    return ln(x, "final_layer_norm")


def stock_model(sd, cfg, dtype, device="cpu"):
    """transformers' CLIPTextModel holding `sd` (either spelling of the keys is loaded, whichever this transformers version uses)."""
    from transformers import CLIPTextConfig, CLIPTextModel
    m = CLIPTextModel(CLIPTextConfig(bos_token_id=0, eos_token_id=2, **cfg))
    own = m.state_dict()
    flat = not any(k.startswith("text_model.") for k in own)
    m.load_state_dict({(k[len("text_model."):] if flat else k): v for k, v in sd.items()}, strict=True)
    return m.to(device=device, dtype=dtype).eval()


def errors(got, ref64):
    """(rel-L2, max per-element error) against the float64 result"""
    d = got.detach().cpu().to(f64) - ref64
    return float(d.norm() / ref64.norm()), float(d.abs().max())
