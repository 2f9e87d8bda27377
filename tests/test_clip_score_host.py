"""CLIP image processor and CLIPSIM, the parts that need no GPU: the NumPy model against Pillow and the stock
processor bit for bit, the host coefficient tables against the model, the refusals by their texts, the pooling-row rules against
transformers, and that the per-element bound of clip_embed is attainable by fp32 arithmetic."""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_reference as R
import opcheck as oc


def lib():
    from lavie_amd import _lib
    return _lib.load()


def last_error():
    return lib().lavie_last_error().decode()


# ------------------------------------------------------------------ the model against Pillow and the processor
@pytest.mark.parametrize("h,w", R.RESIZE_SIZES)
def test_model_is_pillow_bicubic_bit_for_bit(h, w):
    from PIL import Image
    out_h, out_w = R.output_size(h, w, 224)
    ends = set()
    for kind in ("random", "rows", "columns", "white"):
        img = R.test_image(h, w, kind)
        want = np.asarray(Image.fromarray(img).resize((out_w, out_h), Image.BICUBIC))
        got = R.resize_u8(img, out_h, out_w)
        assert np.array_equal(got, want), (h, w, kind)
        ends |= {int(got.min()), int(got.max())}
    if min(h, w) <= 240:                          # no heavy averaging: the alternating rows overshoot past both clip ends
        assert {0, 255} <= ends


@pytest.fixture(scope="module")
def stock_processor():
    from transformers import CLIPImageProcessor
    return CLIPImageProcessor()


@pytest.mark.parametrize("h,w", R.PROCESSOR_SIZES)
def test_model_is_the_stock_processor_bit_for_bit(h, w, stock_processor):
    from PIL import Image
    img = R.test_image(h, w)
    want = stock_processor(images=Image.fromarray(img), return_tensors="pt").pixel_values[0].numpy()
    got = R.preprocess(img)
    assert want.dtype == np.float32 and want.shape == got.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------ the host tables
@pytest.mark.parametrize("n_in,n_out", R.TABLE_PAIRS)
def test_host_tables_are_the_models(n_in, n_out):
    L = lib()
    ks = L.lavie_clip_resample_table_host(n_in, n_out, None, None, None)
    xmin, count, coeff = R.axis_table(n_in, n_out)
    assert ks == coeff.shape[1]
    a, b, c = (C.c_int * n_out)(), (C.c_int * n_out)(), (C.c_int * (n_out * ks))()
    assert L.lavie_clip_resample_table_host(n_in, n_out, a, b, c) == ks
    assert np.array_equal(np.array(a), xmin) and np.array_equal(np.array(b), count)
    assert np.array_equal(np.array(c).reshape(n_out, ks), coeff)


def test_refusals_hold_to_their_texts():
    L = lib()
    ws = L.lavie_clip_preprocess_workspace_bytes
    for args, word in [((1, 7, 100, 224, 224), "short edge 7 is below 8"), ((1, 300, 300, 8, 8), "is above 32"),
                       ((1, 64, 48, 32, 64), "crop=64 is greater than the resized edge 32"), ((0, 64, 48, 224, 224), "B=0")]:
        assert ws(*args) == -1 and word in last_error(), (args, last_error())
    assert ws(3, 64, 48, 224, 224) > 0
    pre = lambda B=1, H=64, W=48, pitch=144, img=64 * 144, inp=4096, out=4096, dt=1, ws_p=4096, ws_n=1 << 30: L.lavie_clip_preprocess_u8(
        inp, B, H, W, pitch, img, out, dt, None, ws_p, ws_n, None)
    for kw, word in [(dict(B=0), "B=0"), (dict(pitch=143), "row_pitch=143 is below 3 W = 144"), (dict(H=7), "short edge 7 is below 8"),
                     (dict(B=2, img=100), "image_pitch=100"), (dict(dt=2), "out_dtype=2"), (dict(inp=None), "null"),
                     (dict(H=8000, W=8000 * 40, pitch=3 * 8000 * 40), "must be in 1..65535"),
                     (dict(ws_n=ws(1, 64, 48, 224, 224) - 1), "the workspace holds"), (dict(ws_p=None), "the workspace holds 0 bytes")]:
        assert pre(**kw) != 0 and word in last_error(), (kw, last_error())
    from lavie_amd import _lib
    cfg = _lib.ClipPreprocessConfigC()
    cfg.struct_size, cfg.size, cfg.crop = C.sizeof(cfg) + 4, 224, 224
    assert L.lavie_clip_preprocess_u8(4096, 1, 64, 48, 144, 0, 4096, 1, C.byref(cfg), 4096, 1 << 30, None) != 0 and "struct_size" in last_error()
    cfg.struct_size = C.sizeof(cfg)
    cfg.mean[:], cfg.std[:] = [0.5] * 3, [0.5, 0.0, 0.5]
    assert L.lavie_clip_preprocess_u8(4096, 1, 64, 48, 144, 0, 4096, 1, C.byref(cfg), 4096, 1 << 30, None) != 0 and "std[1]" in last_error()
    assert L.lavie_clip_resample_table_host(0, 8, None, None, None) == -1 and "in=0" in last_error()
    assert L.lavie_clip_resample_table_host(330, 10, None, None, None) == -1 and "above 32" in last_error()
    emb = lambda B=1, Lx=77, Cc=128, D=128, row=0, g=None, b=None: L.lavie_clip_embed_f16(4096, B, Lx, Cc, None, 2, row, g, b, 1e-5, 4096, D, 1,
                                                                                         4096, None)
    for kw, word in [(dict(B=0), "B=0"), (dict(Cc=192), "C=192 must be a multiple of 128"), (dict(D=2176), "D=2176"), (dict(row=77), "row=77"),
                     (dict(g=4096), "both ln_weight and ln_bias"), (dict(Lx=0), "L=0")]:
        assert emb(**kw) != 0 and word in last_error(), (kw, last_error())
    sim = lambda N=8, P=2, D=128, F=4: L.lavie_clip_similarity_f32(4096, 4096, 4096, N, P, D, F, 1.0, None)
    for kw, word in [(dict(F=3), "N = P frames"), (dict(P=0), "P=0"), (dict(D=0), "D=0"), (dict(F=-1), "frames=-1")]:
        assert sim(**kw) != 0 and word in last_error(), (kw, last_error())


# ------------------------------------------------------------------ the pooling row
@pytest.mark.parametrize("eos", [2, 49407])
def test_pooling_rows_are_transformers(eos):
    """the row the kernel's rule names = the row whose hidden state transformers returns as pooler_output"""
    cfg = R.small_clip_config(eos_token_id=eos)
    m = R.small_clip_model(cfg, dtype=torch.float32)
    ids = R.token_ids(6, 77, eos, cfg["text_config"]["vocab_size"], seed=3)
    ids[0, 5] = ids[0].max()                              # a repeated maximum (legacy rule: the first one counts)
    if eos != 2:
        assert (ids[1] == eos).sum() > 1                  # eos == pad: every padding position matches, the first one counts
        ids[5] = torch.randint(3, 1000, (77,))            # no eos at all: row 0
    rows = R.pooled_rows(ids, eos)
    if eos != 2:
        assert rows[5] == 0 and rows[1] == (ids[1] == eos).nonzero()[0, 0]
    else:
        assert rows[0] == (ids[0] == ids[0].max()).nonzero()[0, 0] and rows[0] <= 5
    with torch.no_grad():
        out = m.text_model(input_ids=ids)
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(6), rows])


# ------------------------------------------------------------------ the bound is attainable
@pytest.mark.parametrize("c,d", [(128, 128), (1024, 768), (768, 512)])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_fp32_model_of_clip_embed_meets_its_bound(c, d, ln, normalize):
    case = embed_case(c, d, ln)
    ref, scale = R.embed_reference(case["x"], case["rows"], case["w"], case.get("gamma"), case.get("beta"), normalize=normalize)
    got = R.embed_model_fp32(case["x"], case["rows"], case["w"], case.get("gamma"), case.get("beta"), normalize=normalize)
    oc.assert_elementwise(got, ref, scale, oc.U32, where=oc.loc_rows(d), label=f"embed model[{c},{d},{ln},{normalize}]", u=oc.U32)


def embed_case(c, d, ln, b=4, l=77, seed=0):
    """x fp16 [b, l, c] with pooled rows 0, 1, 76 and one row of large magnitude (|x| ~ 200) for the LayerNorm sums"""
    g = torch.Generator().manual_seed(seed + c + d)
    x = torch.randn(b, l, c, generator=g)
    rows = torch.tensor([0, 1, l - 1, 5][:b])
    x[3, 5] = 200.0 + torch.randn(c, generator=g)
    case = dict(x=x.half(), rows=rows, w=(torch.randn(d, c, generator=g) * c ** -0.5).half())
    if ln:
        case["gamma"] = (1.0 + 0.2 * torch.randn(c, generator=g)).half().float()
        case["beta"] = (0.1 * torch.randn(c, generator=g)).half().float()
    return case


def test_an_output_rounded_to_fp16_is_caught():
    """the bound is an fp32 bound: the same values stored through fp16 leave it (at C = 128, where the sum's allowance is smallest)"""
    case = embed_case(128, 128, False)
    ref, scale = R.embed_reference(case["x"], case["rows"], case["w"], normalize=False)
    good = R.embed_model_fp32(case["x"], case["rows"], case["w"], normalize=False)
    with pytest.raises(AssertionError, match="outside the bound"):
        oc.assert_elementwise(good.half().float(), ref, scale, oc.U32, u=oc.U32, label="rounded output")


# ------------------------------------------------------------------ float64 references from transformers
@pytest.mark.parametrize("patch,eos", [(32, 2), (14, 49407)])
def test_float64_references_are_transformers(patch, eos):
    """the helpers the GPU tests call are CLIPModel's own get_*_features, and CLIPSIM of them is the written-out mean"""
    cfg = R.small_clip_config(patch=patch, eos_token_id=eos)
    m = R.small_clip_model(cfg)
    s = cfg["vision_config"]["image_size"]
    px = torch.randn(4, 3, s, s, dtype=torch.float64)
    ids = R.token_ids(2, 77, eos, cfg["text_config"]["vocab_size"])
    img, txt = R.stock_features(m, pixel_values=px), R.stock_features(m, input_ids=ids)
    with torch.no_grad():
        out = m(input_ids=ids, pixel_values=px)
    assert torch.allclose(out.image_embeds / out.image_embeds.norm(dim=-1, keepdim=True), img, rtol=0, atol=1e-12)
    assert torch.allclose(out.text_embeds / out.text_embeds.norm(dim=-1, keepdim=True), txt, rtol=0, atol=1e-12)
    assert torch.allclose(out.logits_per_image, m.logit_scale.exp() * img @ txt.T, rtol=0, atol=1e-9)
    sim, _ = R.similarity_reference(img, txt, frames=2)
    assert torch.allclose(sim, torch.stack([100 * (img[2 * p:2 * p + 2] @ txt[p]).mean() for p in range(2)]), rtol=0, atol=1e-9)


def test_processor_refuses_what_is_not_built():
    from lavie_amd.clip_score import HipCLIPImageProcessor
    from types import SimpleNamespace
    stock = dict(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, image_mean=R.CLIP_MEAN, image_std=R.CLIP_STD, resample=3,
                 do_resize=True, do_center_crop=True, do_rescale=True, do_normalize=True, rescale_factor=1 / 255)
    p = HipCLIPImageProcessor.from_stock(SimpleNamespace(**stock))
    assert (p.size, p.crop_size) == (224, 224)
    for kw, word in [(dict(do_resize=False), "do_resize=False"), (dict(resample=2), "resample"), (dict(do_normalize=False), "do_normalize=False"),
                     (dict(rescale_factor=1.0), "rescale_factor")]:
        with pytest.raises(ValueError, match=word):
            HipCLIPImageProcessor.from_stock(SimpleNamespace(**dict(stock, **kw)))
    with pytest.raises(ValueError, match="mixed sizes"):
        p._pixels([np.zeros((8, 9, 3), np.uint8), np.zeros((9, 8, 3), np.uint8)])
    with pytest.raises(ValueError, match="float32 pixels are not built"):
        p._pixels(torch.zeros(1, 8, 8, 3))
