"""NumPy integer model of the CLIP image processor and the float64 references of the feature heads and CLIPSIM.

The resampling is Pillow's 8-bit ImagingResample written out: per axis the bounds and double coefficients of precompute_coeffs, the
int32 coefficients of normalize_coeffs_8bpc, and the two integer passes with a uint8 image between them.  The host tests hold it to
`PIL.Image.resize(BICUBIC)` and to the local `CLIPImageProcessor` bit for bit; the GPU tests hold the kernels to it.  A plain module."""
import math

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22

RESIZE_SIZES = [(320, 512), (37, 53), (224, 224), (240, 224), (1280, 2048), (100, 300), (300, 100), (64, 48), (225, 226)]   # (H, W)
PROCESSOR_SIZES = [(320, 512), (64, 48), (225, 227), (100, 301), (1280, 2048)]
TABLE_PAIRS = [(512, 358), (53, 320), (2048, 358), (48, 224), (226, 224), (224, 224)]                                      # (in, out)


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_table(n_in, n_out):
    """(xmin [out], count [out], coeff int32 [out, ksize]) of one axis; Python floats are the doubles of the C code."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin, count, coeff = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [bicubic((x + lo - center + 0.5) / fs) for x in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            coeff[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        xmin[xx], count[xx] = lo, hi - lo
    return xmin, count, coeff


def _pass(img, table, keep):
    """one pass along axis 1 of img [rows, n_in, ch] uint8 for the outputs `keep` (a range)"""
    xmin, count, coeff = table
    out = np.empty((img.shape[0], len(keep), img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for j, xx in enumerate(keep):
        n = int(count[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin[xx]:xmin[xx] + n, :], coeff[xx, :n].astype(np.int64), axes=([1], [0]))
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31                   # Pillow's accumulator is a signed 32-bit int
        out[:, j, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8(img, out_h, out_w, rows=None, cols=None):
    """img uint8 [H, W, 3] -> rows x cols of the [out_h, out_w, 3] resize: horizontal pass, uint8, vertical pass"""
    h, w, _ = img.shape
    rows = range(out_h) if rows is None else rows
    cols = range(out_w) if cols is None else cols
    mid = _pass(img, axis_table(w, out_w), cols)
    return _pass(mid.transpose(1, 0, 2), axis_table(h, out_h), rows).transpose(1, 0, 2)


def output_size(h, w, size):
    """transformers' shortest-edge rule -> (out_h, out_w)"""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def preprocess(img, size=224, crop=224, mean=CLIP_MEAN, std=CLIP_STD):
    """img uint8 [H, W, 3] -> pixel_values fp32 [3, crop, crop] with the stock processor's bits"""
    h, w, _ = img.shape
    out_h, out_w = output_size(h, w, size)
    assert crop <= min(out_h, out_w)
    y0, x0 = (out_h - crop) // 2, (out_w - crop) // 2
    u = resize_u8(img, out_h, out_w, range(y0, y0 + crop), range(x0, x0 + crop))
    x = u.astype(np.float32) / np.float32(255)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def test_image(h, w, kind="random", seed=0):
    if kind == "rows":                    # alternating 0 / 255 rows: the negative lobes push both ends past the clip
        img = np.zeros((h, w, 3), np.uint8)
        img[1::2] = 255
        return img
    if kind == "columns":
        img = np.zeros((h, w, 3), np.uint8)
        img[:, 1::2] = 255
        return img
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------ the feature heads
def pooled_rows(ids, eos_token_id):
    """CLIPTextTransformer's pooling row per prompt: ids integer [B, L]"""
    ids = torch.as_tensor(ids)
    if eos_token_id == 2:
        return ids.to(torch.int).argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


def embed_reference(x, rows, w, gamma=None, beta=None, eps=1e-5, normalize=True):
    """float64 out [B, D] and the per-element bound's scale (in units of 2^-23) of lavie_clip_embed_f16.

    Bound: |got - ref| <= U32 |ref| + U32 scale.  With T_d = sum_c |W_dc| S_c, S_c = |x_c| without the LayerNorm and
    (|x_c - mu| + mean|x|) rstd |gamma_c| + |beta_c| with it, the projection's error is at most k_y U32 T_d, k_y = C + 8 (the C-term
    fp32 sum) without and 3 C + 32 with the LayerNorm (two more C-term sums, the mean and the variance, and 16 single roundings).
    Normalised: T_d / |y| + |z_d| (|T| / |y|) times k_y, plus |z_d| (D / 2 + 8) for the D-term sum under the square root."""
    x64 = x.double()[torch.arange(x.shape[0]), rows]
    w64 = w.double()
    c, d = x64.shape[1], w64.shape[0]
    if gamma is not None:
        mu = x64.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + eps)
        xn = (x64 - mu) * rstd * gamma.double() + beta.double()
        s = ((x64 - mu).abs() + x64.abs().mean(-1, keepdim=True)) * rstd * gamma.double().abs() + beta.double().abs()
        k_y = 3 * c + 32
    else:
        xn, s, k_y = x64, x64.abs(), c + 8
    y = xn @ w64.T
    t = s @ w64.abs().T
    if not normalize:
        return y, k_y * t
    nrm = y.norm(dim=-1, keepdim=True)
    z = y / nrm
    scale = k_y * (t / nrm + z.abs() * (t.norm(dim=-1, keepdim=True) / nrm)) + z.abs() * (d / 2 + 8)
    return z, scale


def embed_model_fp32(x, rows, w, gamma=None, beta=None, eps=1e-5, normalize=True):
    """the kernel's arithmetic in fp32 on the CPU, sums in index order (the bound must hold for ANY order of an fp32 sum)"""
    xr = x.float()[torch.arange(x.shape[0]), rows]
    if gamma is not None:
        mean = xr.sum(-1, keepdim=True) / xr.shape[1]
        d = xr - mean
        var = (d * d).sum(-1, keepdim=True) / xr.shape[1]
        xr = d * (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))) * gamma.float() + beta.float()
    y = xr @ w.float().T
    if normalize:
        y = y / torch.sqrt((y * y).sum(-1, keepdim=True))
    return y


def similarity_reference(img, txt, frames=0, scale=1.0):
    """float64 result and the sum of |terms| of lavie_clip_similarity_f32"""
    i64, t64 = img.double(), txt.double()
    if frames == 0:
        return scale * (i64 @ t64.T), abs(scale) * (i64.abs() @ t64.abs().T)
    p = t64.shape[0]
    g = i64.view(p, frames, -1)
    return (100.0 / frames) * (g * t64[:, None]).sum((1, 2)), (100.0 / frames) * (g.abs() * t64.abs()[:, None]).sum((1, 2))


def clipsim_from_matrix(dots, frames):
    """the grouped form from the matrix form's diagonal blocks (dots fp32 [P frames, P], scale 1), fp32, in frame order"""
    p = dots.shape[1]
    out = torch.empty(p, dtype=torch.float32)
    k = torch.tensor(100.0, dtype=torch.float32) / torch.tensor(float(frames), dtype=torch.float32)
    for i in range(p):
        s = dots[i * frames, i].clone()
        for f in range(1, frames):
            s = s + dots[i * frames + f, i]
        out[i] = k * s
    return out


# ------------------------------------------------------------------ small random-init CLIPModels
def small_clip_config(patch=32, eos_token_id=2, image_size=None, width=128, proj=128):
    image_size = image_size or (64 if patch == 32 else 56)
    return dict(
        text_config=dict(vocab_size=49408 if eos_token_id == 49407 else 1000, hidden_size=width, intermediate_size=2 * width, num_hidden_layers=2,
                         num_attention_heads=width // 64, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                         eos_token_id=eos_token_id, bos_token_id=0 if eos_token_id == 2 else 49406, pad_token_id=1),
        vision_config=dict(hidden_size=width, intermediate_size=2 * width, num_hidden_layers=2, num_attention_heads=width // 64,
                           image_size=image_size, patch_size=patch, hidden_act="quick_gelu", layer_norm_eps=1e-5),
        projection_dim=proj, logit_scale_init_value=2.6592)


def small_clip_model(cfg, seed=0, dtype=torch.float64, device="cpu"):
    """a transformers CLIPModel with random weights rounded to fp16 (the values every implementation under test holds)"""
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(seed)
    m = CLIPModel(CLIPConfig(text_config=dict(cfg["text_config"]), vision_config=dict(cfg["vision_config"]),
                             projection_dim=cfg["projection_dim"], logit_scale_init_value=cfg["logit_scale_init_value"])).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.mul_(3.0)                  # the default init (std 0.02) leaves the towers near-linear: widen it
            p.copy_(p.half().float())
    return m.to(device=device, dtype=dtype)


def stock_features(m, pixel_values=None, input_ids=None):
    """get_image_features / get_text_features through the parts (the same on every transformers version), L2-normalised"""
    with torch.no_grad():
        if pixel_values is not None:
            f = m.visual_projection(m.vision_model(pixel_values=pixel_values).pooler_output)
        else:
            f = m.text_projection(m.text_model(input_ids=input_ids).pooler_output)
    return f / f.norm(p=2, dim=-1, keepdim=True)


def token_ids(b, l, eos_token_id, vocab, seed=0):
    """prompts of different lengths: bos, words, eos, then padding (pad = eos for the 49407 family, 1 for the legacy one)"""
    g = torch.Generator().manual_seed(seed)
    bos, pad = (0, 1) if eos_token_id == 2 else (49406, eos_token_id)
    ids = torch.full((b, l), pad, dtype=torch.int64)
    for i in range(b):
        n = 3 + (5 * i) % (l - 4)
        hi = vocab - 2 if eos_token_id != 2 else vocab
        ids[i, 0] = bos
        ids[i, 1:1 + n] = torch.randint(3, hi, (n,), generator=g)
        ids[i, 1 + n] = eos_token_id if eos_token_id != 2 else vocab - 1      # legacy rule: the eos is the LARGEST id of the row
    return ids
