"""The cases of the image-conditioning checks, shared by tests/test_image_encoder_host.py (CPU: the float64
references against transformers and torch.nn, the fp32 models against their own bounds) and tests/test_gpu_image_encoder.py.

Bounds are tests/opcheck.py's |got - ref| <= u |ref| + c scale against float64, c from the kernels' rounding points:
  short attention    n = 2 fp16 roundings (P in front of the PV product, the store) + fp32 accumulation over at most 320 keys and
                     64 dims: round_c(2) + gemm_c(320 + 64)
  patch embedding    n = 2 (a pixel to fp16 -- none for fp16 pixels --, the store) + fp32 accumulation of the 3 P^2 <= 768 products
                     and the position: round_c(2) + gemm_c(768 + 2); the class row is exact (fp32 sum of two fp16 values, rounded once)
  relu               exact: compared bit for bit with torch.relu
Shapes are the smallest that cross the kernels' edges; nothing runs at 24 or 12 layers."""
import functools
import math

import torch

import opcheck as oc
from textcases import LOG2E, errors, gen, merge  # noqa: F401  (errors: re-exported for the model tests)

f16, f64 = torch.float16, torch.float64

ATT_LENGTHS = [(1, 1), (1, 257), (16, 16), (17, 15), (64, 65), (77, 77), (77, 257), (257, 77), (257, 257), (5, 320), (320, 320)]
ATT_SHAPES = [(1, 1, 64), (3, 4, 32), (2, 12, 64)]           # (NB, heads, dh)
ATT_C = oc.round_c(2) + oc.gemm_c(320 + 64)
ACT_SIZES = [1, 7, 8, 4096 + 3]
PATCH_CONFIGS = [(14, 56, 128), (16, 32, 128), (14, 224, 1024)]      # (P, S, C)
PATCH_C = oc.round_c(2) + oc.gemm_c(768 + 2)

TOWER_TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
                  hidden_act="quick_gelu", layer_norm_eps=1e-5)
TOWER_CONFIGS = {
    "tiny": TOWER_TINY,
    "dh32": dict(TOWER_TINY, num_attention_heads=4),
    "patch16-gelu": dict(TOWER_TINY, image_size=32, patch_size=16, hidden_act="gelu"),
    "vit-l-1layer": dict(TOWER_TINY, hidden_size=1024, intermediate_size=4096, num_hidden_layers=1, num_attention_heads=16, image_size=224),
}
MAPPER_TINY = dict(input_dim=128, output_dim=128, num_layers=2, num_heads=2, dim_feedforward=256, seq_len_in=17, seq_len_out=7)
MAPPER_CONFIGS = {
    "tiny": MAPPER_TINY,
    "prod-1layer": dict(input_dim=1024, output_dim=768, num_layers=1, num_heads=12, dim_feedforward=2048, seq_len_in=257, seq_len_out=77),
}
MODEL_B = 2


# ------------------------------------------------------------------ short attention
def split(t, nb, l, heads, dh):
    return t.reshape(nb, l, heads, dh).permute(0, 2, 1, 3)


def attention_ref(q, k, v, scale):
    """float64: softmax(scale q k^T) v and the scale sum_j p_j |v_j|; [nb, heads, l, dh] operands."""
    p = torch.softmax(q.to(f64) @ k.to(f64).transpose(-1, -2) * scale, -1)
    return p @ v.to(f64), p @ v.to(f64).abs()


def attention_model(q, k, v, scale):
    """The kernel's arithmetic in torch fp32: scores in log2 units, the true row maximum, exp2, P rounded to fp16, the row sum over
    the rounded P, one rounding at the store."""
    s = (q.float() @ k.float().transpose(-1, -2)) * (scale * LOG2E)
    p = torch.exp2(s - s.max(-1, keepdim=True).values).half().float()
    return ((p @ v.float()) / p.sum(-1, keepdim=True)).half()


HARD_LQ, HARD_LK = 77, 257


def hard_rows():
    """(query, matching key) of the far rows whose key lies at 64..255, of the far rows whose key is 256 (the single valid key of
    the last key tile), and (query, dominant key) of the dominant-key rows."""
    return [(3, 100), (40, 255)], [(10, 256), (76, 256)], [(5, 70), (60, 200)]


@functools.lru_cache(maxsize=None)
def attention_case(nb, heads, dh, lq, lk, pads=(0, 0, 0), packed=False, hard=False):
    """q [nb lq, c + pads[0]], k [nb lk + 2, c + pads[1]], v [nb lk + 2, c + pads[2]]: the padding columns and the two rows behind the
    last entry's last key are NaN.  packed (lq == lk): the three are column slices of ONE tensor [nb l + 2, 3 c + pads[0]].
    hard ((77, 257)): rows rewritten as hard_rows says, every constant exact in fp16."""
    g = gen("short", nb, heads, dh, lq, lk, pads, packed, hard)
    c = heads * dh
    q = torch.randn(nb, lq, c, generator=g).half()
    k, v = (torch.randn(nb, lk, c, generator=g).half() for _ in range(2))
    scale = dh ** -0.5
    if hard:
        assert (lq, lk) == (HARD_LQ, HARD_LK)
        mid, last, dom = hard_rows()
        u = (torch.randint(0, 2, (c,), generator=g) * 2 - 1).to(f16)
        k[:, :64] = (-1.25 * u.float() + 0.05 * torch.randn(64, c, generator=g)).half()      # q k = -20 dh: -20 sqrt(dh) nats <= -113
        # a far row's query is 16 (u + w) with w = u * (a balanced +-1 pattern per head, orthogonal to the other rows' patterns): u w = 0
        # per head, so the first 64 keys stay at -20 dh; its matching key u + w scores 32 dh, the other rows' matching keys 16 dh
        i = torch.arange(dh)
        walsh = [torch.where(i < dh // 2, 1, -1), torch.where(i % 2 == 0, 1, -1), torch.where(i % 4 < 2, 1, -1)]
        pattern = {m: walsh[n].repeat(heads).to(f16) for n, m in enumerate(sorted({m for _, m in mid + last}))}
        for r, m in mid + last:
            w = u * pattern[m]
            q[:, r] = 16 * (u + w)
            k[:, m] = u + w                                                                    # the matching key
        for n, (r, d) in enumerate(dom):          # a dominant row: q = u * (a further pattern), so that its key 3 q is orthogonal to the far rows
            q[:, r] = u * torch.where(i % (8 << n) < (4 << n), 1, -1).repeat(heads).to(f16)
            k[:, d] = 3 * q[:, r]                                                              # q k scale = 3 dh / sqrt(dh) = 3 sqrt(dh)
        s = split(q, nb, lq, heads, dh).to(f64) @ split(k, nb, lk, heads, dh).to(f64).transpose(-1, -2) * scale
        far = [r for r, _ in mid + last]
        assert s[:, :, far, :64].max() < -100, s[:, :, far, :64].max()
        for r, m in mid + last:                                                                # ONE key carries the row: without it the result changes
            others = torch.cat([s[:, :, r, :m], s[:, :, r, m + 1:]], -1)
            assert s[:, :, r, m].min() > 0 and (s[:, :, r, m] - others.max(-1).values).min() > 50, (r, m)
        for r, d in dom:
            others = torch.cat([s[:, :, r, :d], s[:, :, r, d + 1:]], -1)
            assert (s[:, :, r, d] - others.max(-1).values).min() > 0, r
    nan = lambda rows, cols: torch.full((rows, cols), math.nan, dtype=f16)
    if packed:
        assert lq == lk
        body = torch.cat([q, k, v, nan(nb * lq, pads[0]).reshape(nb, lq, pads[0])], -1).reshape(nb * lq, 3 * c + pads[0])
        tensors = {"qkv": torch.cat([body, nan(2, 3 * c + pads[0])])}
    else:
        wide = lambda t, l, pad, tail: torch.cat([torch.cat([t.reshape(nb * l, c), nan(nb * l, pad)], -1), nan(tail, c + pad)])
        tensors = {"q": wide(q, lq, pads[0], 0), "k": wide(k, lk, pads[1], 2), "v": wide(v, lk, pads[2], 2)}
    heads_of = lambda: (split(q, nb, lq, heads, dh), split(k, nb, lk, heads, dh), split(v, nb, lk, heads, dh))

    def ref():
        y, sc = attention_ref(*heads_of(), scale)
        return merge(y), merge(sc)

    return dict(tensors=tensors, packed=packed, ref=ref, model=lambda: merge(attention_model(*heads_of(), scale)), nb=nb, heads=heads,
                dh=dh, lq=lq, lk=lk, c=c, where=oc.loc_heads(heads, dh))


# ------------------------------------------------------------------ patch embedding
@functools.lru_cache(maxsize=None)
def patch_case(p, s, c, b, dtype):
    """pixels ~ N(0, 1) in `dtype`, weights N(0, 1 / sqrt(3 p^2)), class and positions N(0, 0.3): fp16-rounded parameters."""
    g = gen("patch", p, s, c, b, str(dtype))
    t = 1 + (s // p) ** 2
    return dict(px=torch.randn(b, 3, s, s, generator=g).to(dtype), w=(torch.randn(c, 3, p, p, generator=g) / math.sqrt(3 * p * p)).half(),
                cls=(0.3 * torch.randn(c, generator=g)).half(), pos=(0.3 * torch.randn(t, c, generator=g)).half(), p=p, s=s, c=c, b=b, t=t)


def patch_ref(case, pixels=None):
    """float64 CLIPVisionEmbeddings and the scale (the magnitudes added up into an element); pixels: a rounded copy for the model"""
    px = (case["px"] if pixels is None else pixels).to(f64)
    p, c = case["p"], case["c"]
    cols = torch.nn.functional.unfold(px, kernel_size=p, stride=p).transpose(1, 2)                 # [b, g^2, 3 p^2], (channel, y, x) order
    w = case["w"].to(f64).reshape(c, -1)
    pos, cls = case["pos"].to(f64), case["cls"].to(f64)
    y = torch.cat([(cls + pos[0]).expand(px.shape[0], 1, c), cols @ w.t() + pos[1:]], 1)
    sc = torch.cat([(cls.abs() + pos[0].abs()).expand(px.shape[0], 1, c), cols.abs() @ w.abs().t() + pos[1:].abs()], 1)
    return y, sc


def patch_model(case):
    """the kernels' arithmetic: pixels rounded to fp16, exact products summed (here in float64: the fp32 order is not modelled), the
    position added before the one rounding"""
    return patch_ref(case, case["px"].half())[0].half()


def relu_input(n):
    """values spanning +-12 with +0, -0, the largest and the smallest subnormal among them"""
    x = (torch.rand(n, generator=gen("relu", n)) * 24 - 12).half()
    x[0] = 0.0
    if n > 1:
        x[1] = -0.0
    if n > 4:
        x[2], x[3], x[4] = -6e-8, 6e-8, -65504.0
    return x


# ------------------------------------------------------------------ the vision tower
def rn(g, *s, std):
    return (torch.randn(*s, generator=g) * std).half()


def tower_state_dict(cfg, seed=0):
    """fp16-rounded random weights under the engine's (classic, `vision_model.`-prefixed) keys, post_layernorm included as a full
    CLIPVisionModel state dict has it; matrices scaled up so that attention is not uniform; norms near 1."""
    g = gen("vision-sd", tuple(sorted(cfg.items())), seed)
    c, i, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    t = 1 + (cfg["image_size"] // p) ** 2
    norm = lambda: ((1 + 0.1 * torch.randn(c, generator=g)).half(), rn(g, c, std=0.1))
    v = "vision_model."
    sd = {v + "embeddings.class_embedding": rn(g, c, std=0.5), v + "embeddings.patch_embedding.weight": rn(g, c, 3, p, p, std=1 / math.sqrt(3 * p * p)),
          v + "embeddings.position_embedding.weight": rn(g, t, c, std=0.3)}
    sd[v + "pre_layrnorm.weight"], sd[v + "pre_layrnorm.bias"] = norm()
    for n in range(cfg["num_hidden_layers"]):
        pre = f"{v}encoder.layers.{n}."
        for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[pre + f"self_attn.{proj}.weight"] = rn(g, c, c, std=1.5 / math.sqrt(c))
            sd[pre + f"self_attn.{proj}.bias"] = rn(g, c, std=0.1)
        sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"] = rn(g, i, c, std=1.0 / math.sqrt(c)), rn(g, i, std=0.1)
        sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"] = rn(g, c, i, std=1.0 / math.sqrt(i)), rn(g, c, std=0.1)
        for ln in ("layer_norm1", "layer_norm2"):
            sd[pre + ln + ".weight"], sd[pre + ln + ".bias"] = norm()
    sd[v + "post_layernorm.weight"], sd[v + "post_layernorm.bias"] = norm()
    return sd


def tower_pixels(cfg, b=MODEL_B, seed=0):
    s = cfg["image_size"]
    return torch.randn(b, 3, s, s, generator=gen("vision-px", s, b, seed))


def tower_reference64(sd, cfg, px):
    """CLIPVisionModel.last_hidden_state in float64, written out: checked against transformers in test_image_encoder_host.py."""
    w = {k[len("vision_model."):]: v.to(f64) for k, v in sd.items()}
    c, heads, p = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"]
    dh = c // heads
    b = px.shape[0]
    ln = lambda x, n: torch.nn.functional.layer_norm(x, (c,), w[n + ".weight"], w[n + ".bias"], cfg["layer_norm_eps"])
    lin = lambda x, n: x @ w[n + ".weight"].t() + w[n + ".bias"]
    patches = torch.nn.functional.conv2d(px.to(f64), w["embeddings.patch_embedding.weight"], stride=p).flatten(2).transpose(1, 2)
    x = torch.cat([w["embeddings.class_embedding"].expand(b, 1, c), patches], 1) + w["embeddings.position_embedding.weight"]
    t = x.shape[1]
    x = ln(x, "pre_layrnorm")
    for n in range(cfg["num_hidden_layers"]):
        q = f"encoder.layers.{n}."
        h = ln(x, q + "layer_norm1")
        qq, kk, vv = (lin(h, q + f"self_attn.{m}_proj").reshape(b, t, heads, dh).transpose(1, 2) for m in "qkv")
        a = (torch.softmax(qq @ kk.transpose(-1, -2) * dh ** -0.5, -1) @ vv).transpose(1, 2).reshape(b, t, c)
        x = x + lin(a, q + "self_attn.out_proj")
        m = lin(ln(x, q + "layer_norm2"), q + "mlp.fc1")
        m = m * torch.sigmoid(1.702 * m) if cfg["hidden_act"] == "quick_gelu" else 0.5 * m * (1 + torch.erf(m / math.sqrt(2)))
        x = x + lin(m, q + "mlp.fc2")
    return x                                   # no post_layernorm: it belongs to the pooled output


def stock_tower(sd, cfg, dtype, device="cpu"):
    """transformers' CLIPVisionModel holding `sd` (either spelling of the keys is loaded, whichever this transformers version uses)."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    m = CLIPVisionModel(CLIPVisionConfig(**cfg))
    flat = not any(k.startswith("vision_model.") for k in m.state_dict())
    m.load_state_dict({(k[len("vision_model."):] if flat else k): v for k, v in sd.items()}, strict=True)
    return m.to(device=device, dtype=dtype).eval()


# ------------------------------------------------------------------ the mapper
def mapper_state_dict(cfg, seed=0):
    """fp16-rounded random weights under MappingNetwork's keys (text_proj included, as a saved mapper has it)."""
    g = gen("mapper-sd", tuple(sorted(cfg.items())), seed)
    c, d, ff = cfg["output_dim"], cfg["input_dim"], cfg["dim_feedforward"]
    sd = {"image_pos_embedding": rn(g, 1, cfg["seq_len_in"], c, std=0.3), "text_pos_embedding": rn(g, 1, cfg["seq_len_out"], c, std=0.3),
          "image_proj.weight": rn(g, c, d, std=1 / math.sqrt(d)), "image_proj.bias": rn(g, c, std=0.1),
          "text_proj.weight": rn(g, c, c, std=1 / math.sqrt(c)), "text_proj.bias": rn(g, c, std=0.1)}
    for n in range(cfg["num_layers"]):
        pre = f"transformer_decoder.layers.{n}."
        for att in ("self_attn", "multihead_attn"):
            sd[pre + att + ".in_proj_weight"], sd[pre + att + ".in_proj_bias"] = rn(g, 3 * c, c, std=1.5 / math.sqrt(c)), rn(g, 3 * c, std=0.1)
            sd[pre + att + ".out_proj.weight"], sd[pre + att + ".out_proj.bias"] = rn(g, c, c, std=1 / math.sqrt(c)), rn(g, c, std=0.1)
        sd[pre + "linear1.weight"], sd[pre + "linear1.bias"] = rn(g, ff, c, std=1 / math.sqrt(c)), rn(g, ff, std=0.1)
        sd[pre + "linear2.weight"], sd[pre + "linear2.bias"] = rn(g, c, ff, std=1 / math.sqrt(ff)), rn(g, c, std=0.1)
        for nm in ("norm1", "norm2", "norm3"):
            sd[pre + nm + ".weight"], sd[pre + nm + ".bias"] = (1 + 0.1 * torch.randn(c, generator=g)).half(), rn(g, c, std=0.1)
    return sd


def mapper_inputs(cfg, b=MODEL_B, bi=None, seed=0):
    """(image features [bi, seq_in, input_dim], text embeddings [b, seq_out, output_dim]), fp16-rounded"""
    g = gen("mapper-in", tuple(sorted(cfg.items())), b, seed)
    img = torch.randn(b, cfg["seq_len_in"], cfg["input_dim"], generator=g).half()
    txt = torch.randn(b, cfg["seq_len_out"], cfg["output_dim"], generator=g).half()
    return (img if bi is None else img[:bi]), txt


def mapper_reference64(sd, cfg, img, txt):
    """MappingNetwork.forward in float64, written out (post-norm decoder layers, ReLU, no final norm)."""
    w = {k: v.to(f64) for k, v in sd.items()}
    c, heads = cfg["output_dim"], cfg["num_heads"]
    dh = c // heads
    b = txt.shape[0]
    ln = lambda x, n: torch.nn.functional.layer_norm(x, (c,), w[n + ".weight"], w[n + ".bias"], 1e-5)

    def mha(xq, xkv, n):
        wi, bi_ = w[n + ".in_proj_weight"], w[n + ".in_proj_bias"]
        q = (xq @ wi[:c].t() + bi_[:c]).reshape(b, -1, heads, dh).transpose(1, 2)
        k = (xkv @ wi[c:2 * c].t() + bi_[c:2 * c]).reshape(b, -1, heads, dh).transpose(1, 2)
        v = (xkv @ wi[2 * c:].t() + bi_[2 * c:]).reshape(b, -1, heads, dh).transpose(1, 2)
        a = (torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v).transpose(1, 2).reshape(b, -1, c)
        return a @ w[n + ".out_proj.weight"].t() + w[n + ".out_proj.bias"]

    mem = (img.to(f64) @ w["image_proj.weight"].t() + w["image_proj.bias"] + w["image_pos_embedding"]).expand(b, -1, -1)
    x = txt.to(f64) + w["text_pos_embedding"]
    for n in range(cfg["num_layers"]):
        p = f"transformer_decoder.layers.{n}."
        x = ln(x + mha(x, x, p + "self_attn"), p + "norm1")
        x = ln(x + mha(x, mem, p + "multihead_attn"), p + "norm2")
        x = ln(x + torch.relu(x @ w[p + "linear1.weight"].t() + w[p + "linear1.bias"]) @ w[p + "linear2.weight"].t() + w[p + "linear2.bias"],
               p + "norm3")
    return x


def stock_mapper(sd, cfg, dtype, device="cpu"):
    from lavie_amd.mapping import MappingNetwork
    m = MappingNetwork(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(device=device, dtype=dtype).eval()
