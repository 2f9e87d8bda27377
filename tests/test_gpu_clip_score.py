"""-m gpu: the CLIP image processor, the feature heads and CLIPSIM on the engine -- the preprocess kernels bit for
bit against the NumPy model of Pillow (tests/clip_reference.py, itself held to Pillow and the stock processor by the host tests),
clip_embed and clip_similarity per element against float64, batch invariance, the scorer against float64 with the stock fp16 CLIPModel
as the yardstick, score / rank, the pipeline's image path and the C ABI from pixels and ids to a score."""
import ctypes

import numpy as np
import pytest
import torch

import clip_reference as R
import imagecases as ic
import opcheck as oc
from test_clip_score_host import embed_case
from test_gpu_image_cond import small  # noqa: F401  (the `small` UNet fixture, as it is)
from test_gpu_image_encoder import c_build

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (225, 227), (64, 48), (100, 301), (500, 260), (320, 512), (640, 1024), (1280, 2048)]      # (H, W)


def sync():
    torch.cuda.synchronize()


def bits32(t):
    return t.contiguous().view(torch.int32)


def packed(imgs, pad=0, gap=0):
    """uint8 [B, H, W, 3] -> (int32 CPU tensor holding the images with `pad` bytes behind every row and `gap` rows behind every image,
    every byte outside the pixels 0xAB; a function that views a device copy of it as the strided uint8 [B, H, W, 3])"""
    b, h, w, _ = imgs.shape
    pitch = 3 * w + pad
    rows = h + gap
    n = (b * rows * pitch + 3) // 4 * 4
    buf = np.full(n, 0xAB, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (b, h, 3 * w), (rows * pitch, pitch, 1))
    view[...] = imgs.reshape(b, h, 3 * w)
    as_images = lambda t: t.view(torch.uint8).as_strided((b, h, w, 3), (rows * pitch, pitch, 3, 1))
    return torch.from_numpy(buf.view(np.int32).copy()), as_images


def run_preprocess(imgs, dtype, pad=0, gap=0, size=224, crop=224):
    from lavie_amd import ops
    data, as_images = packed(imgs, pad, gap)
    fn = lambda i, o: ops.clip_preprocess(as_images(i["px"]), size, crop, dtype=dtype, out=o["y"])
    return oc.run_guarded(fn, {"px": data}, {"y": ((imgs.shape[0], 3, crop, crop), dtype)}, sync=sync)["y"]


def model_pixels(imgs, size=224, crop=224):
    return torch.from_numpy(np.stack([R.preprocess(im, size, crop) for im in imgs]))


# ------------------------------------------------------------------ preprocess
@pytest.mark.parametrize("h,w", SIZES)
def test_preprocess_has_the_models_bits(h, w):
    """fp32: the model's bits (= the stock processor's); fp16: one rounding of them; guarded operands, poisoned outputs, both runs"""
    imgs = R.test_image(h, w)[None]
    want = model_pixels(imgs)
    oc.assert_bits(run_preprocess(imgs, torch.float32), want, where=oc.loc_nchw(3, 224, 224), label=f"preprocess fp32 {h}x{w}")
    oc.assert_bits(run_preprocess(imgs, torch.float16), want.half(), where=oc.loc_nchw(3, 224, 224), label=f"preprocess fp16 {h}x{w}")


@pytest.mark.parametrize("h,w", [(37, 53), (100, 301), (64, 48)])
def test_preprocess_batch_of_three_with_wider_pitches_and_both_clip_ends(h, w):
    imgs = np.stack([R.test_image(h, w), R.test_image(h, w, "rows"), R.test_image(h, w, "white")])
    want = model_pixels(imgs)
    lo, hi = (0 / 255 - R.CLIP_MEAN[0]) / R.CLIP_STD[0], (255 / 255 - R.CLIP_MEAN[0]) / R.CLIP_STD[0]
    assert abs(float(want[1, 0].min()) - lo) < 1e-6 and abs(float(want[1, 0].max()) - hi) < 1e-6          # pixel 0 and pixel 255 occur
    got = run_preprocess(imgs, torch.float32, pad=13, gap=2)
    oc.assert_bits(got, want, where=oc.loc_nchw(3, 224, 224), label=f"preprocess B=3 pitch {h}x{w}")
    for b in range(3):                                       # an image alone, contiguous: the same bits
        oc.assert_bits(run_preprocess(imgs[b:b + 1], torch.float32)[0], want[b], label=f"image {b} alone")


def test_preprocess_other_size_crop_and_constants():
    imgs = R.test_image(80, 96)[None]
    from lavie_amd import ops
    got = ops.clip_preprocess(torch.from_numpy(imgs).cuda(), 56, 48, mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3))
    want = torch.from_numpy(R.preprocess(imgs[0], 56, 48, (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)))[None]
    oc.assert_bits(got, want, label="size 56 crop 48")


def test_preprocess_refusals_leave_the_output_alone():
    from lavie_amd import ops
    y = oc.guarded((1, 3, 224, 224), torch.float32)
    for shape, kw, word in [((1, 7, 100, 3), {}, "short edge 7 is below 8"), ((1, 300, 300, 3), dict(size=8, crop=8), "is above 32"),
                            ((1, 64, 48, 3), dict(size=32, crop=64), "crop=64 is greater than the resized edge 32")]:
        px = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        with pytest.raises(RuntimeError, match=word):
            ops.clip_preprocess(px, **kw, out=y.t if "crop" not in kw else None)
    sync()
    y.check_bands("y (refused call)")
    assert y.unwritten().numel() == y.n


def test_an_image_has_the_same_pixel_values_in_every_batch():
    from lavie_amd import ops
    pool = torch.from_numpy(np.stack([R.test_image(100, 301, seed=s) for s in range(8)])).cuda()
    single = [bits32(ops.clip_preprocess(pool[i:i + 1])[0]) for i in range(8)]
    for n in (1, 3, 8):
        for shift in (0, 5):
            order = [(i + shift) % 8 for i in range(n)]
            got = bits32(ops.clip_preprocess(pool[order]))
            for pos, i in enumerate(order):
                assert torch.equal(got[pos], single[i]), (n, pos, i)


# ------------------------------------------------------------------ clip_embed
def ids_for_rows(rows, l, eos):
    """ids whose pooled row is rows[b]: legacy rule -> the maximum there and once more behind it; eos rule -> eos from there on (eos == pad)"""
    ids = torch.ones(len(rows), l, dtype=torch.int64)
    for b, r in enumerate(rows.tolist()):
        if eos == 2:
            ids[b, r] = 900
            ids[b, min(r + 3, l - 1)] = 900
        else:
            ids[b, r:] = eos
    assert torch.equal(R.pooled_rows(ids, eos), rows)
    return ids


@pytest.mark.parametrize("c,d", [(128, 128), (1024, 768), (768, 512)])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
def test_clip_embed_per_element(c, d, ln, normalize):
    """within the bound of DESIGN.md 7.19 on guarded operands; rows 0, 1, 76 and a row of |x| ~ 200; both row rules"""
    from lavie_amd import ops
    case = embed_case(c, d, ln)
    eos = 2 if normalize else 49407
    ids = ids_for_rows(case["rows"], 77, eos)
    ins = {"x": case["x"], "w": case["w"], "ids": ids.to(torch.int32)}
    if ln:
        ins.update(gamma=case["gamma"], beta=case["beta"])
    fn = lambda i, o: ops.clip_embed(i["x"], i["w"], ids=i["ids"], eos_token_id=eos, ln_weight=i.get("gamma"), ln_bias=i.get("beta"),
                                     normalize=normalize, out=o["y"])
    got = oc.run_guarded(fn, ins, {"y": ((4, d), torch.float32)}, sync=sync)["y"]
    ref, scale = R.embed_reference(case["x"], case["rows"], case["w"], case.get("gamma"), case.get("beta"), normalize=normalize)
    oc.assert_elementwise(got, ref, scale, oc.U32, where=oc.loc_rows(d), label=f"clip_embed[{c},{d},ln{ln},n{normalize}]", u=oc.U32)
    # the fixed row, and an item alone: the same bits
    x, w = case["x"].cuda(), case["w"].cuda()
    kw = dict(ln_weight=case.get("gamma"), ln_bias=case.get("beta"), normalize=normalize)
    for b in range(4):
        alone = ops.clip_embed(x[b:b + 1], w, row=int(case["rows"][b]), **kw)
        oc.assert_bits(alone[0], got[b], label=f"item {b} alone by its fixed row")
    if eos != 2:                                             # no eos among the ids: the rule falls back to row 0, which item 0 pools
        none = torch.ones(1, 77, dtype=torch.int64)
        assert int(R.pooled_rows(none, eos)[0]) == 0
        oc.assert_bits(ops.clip_embed(x[:1], w, ids=none, eos_token_id=eos, **kw)[0], got[0], label="no eos among the ids")
        both = torch.cat([none, ids[3:4]])                   # beside an item that has one
        oc.assert_bits(ops.clip_embed(x[[0, 3]].contiguous(), w, ids=both, eos_token_id=eos, **kw), got[[0, 3]], label="no eos, then an eos at 5")


def test_clip_embed_items_do_not_depend_on_the_batch():
    from lavie_amd import ops
    case = embed_case(768, 512, True, b=4)
    x = case["x"][:, :8].repeat(2, 1, 1).cuda()               # eight items [8, 8, 768]
    w = case["w"].cuda()
    kw = dict(row=5, ln_weight=case["gamma"], ln_bias=case["beta"])
    single = [bits32(ops.clip_embed(x[i:i + 1], w, **kw)[0]) for i in range(8)]
    for n in (1, 3, 8):
        order = [(i + 5) % 8 for i in range(n)]
        got = bits32(ops.clip_embed(x[order].contiguous(), w, **kw))
        for pos, i in enumerate(order):
            assert torch.equal(got[pos], single[i]), (n, pos, i)


# ------------------------------------------------------------------ clip_similarity
@pytest.mark.parametrize("d", [128, 512, 100])
def test_clip_similarity_per_element_and_the_grouped_form(d):
    from lavie_amd import ops
    g = torch.Generator().manual_seed(d)
    p, f = 3, 4
    img = torch.nn.functional.normalize(torch.randn(p * f, d, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(p, d, generator=g), dim=-1)
    c = oc.gemm_c(d)
    run = lambda frames, scale, shape: oc.run_guarded(
        lambda i, o: ops.clip_similarity(i["img"], i["txt"], frames=frames, scale=scale, out=o["y"]), {"img": img, "txt": txt},
        {"y": (shape, torch.float32)}, sync=sync)["y"]
    logits = run(0, 14.285, (p * f, p))
    ref, terms = R.similarity_reference(img, txt, scale=14.285)
    oc.assert_elementwise(logits, ref, terms, c, where=oc.loc_rows(p), label=f"logits[{d}]", u=oc.U32)
    dots = run(0, 1.0, (p * f, p))
    sim = run(f, 1.0, (p,))
    oc.assert_bits(sim, R.clipsim_from_matrix(dots, f), label=f"clipsim[{d}] from the matrix form's diagonal blocks")
    ref, terms = R.similarity_reference(img, txt, frames=f)
    oc.assert_elementwise(sim, ref, terms, c, label=f"clipsim[{d}]", u=oc.U32)


# ------------------------------------------------------------------ the scorer
MODELS = {"patch32-eos2": dict(patch=32, eos_token_id=2), "patch14-eos49407": dict(patch=14, eos_token_id=49407)}


@pytest.fixture(scope="module")
def scorers():
    """name -> (ClipScorer, float64 CLIPModel, config), built once"""
    from lavie_amd.clip_score import ClipScorer
    built = {}

    def get(name):
        if name not in built:
            cfg = R.small_clip_config(**MODELS[name])
            m = R.small_clip_model(cfg)
            built[name] = (ClipScorer.from_state_dict(m.state_dict(), cfg), m, cfg)
        return built[name]
    return get


def within_twice_the_stock_error(name, got, stock, ref):
    e = float((got.double().cpu() - ref).abs().max())
    s = float((stock.double().cpu() - ref).abs().max())
    print(f"{name}: engine max error {e:.3e}; stock fp16 max error {s:.3e}")
    assert e <= 2 * s, (name, e, s)


@pytest.mark.parametrize("name", list(MODELS))
def test_features_and_clipsim_against_float64_within_twice_the_stock_fp16_error(name, scorers):
    """Yardstick: transformers' CLIPModel in float64 on the same fp16-rounded weights; the stock module in fp16 on the device shows
    what fp16 storage costs.  Eight images, eight prompts, four clips of two frames.  Measured pairs: DESIGN.md 7.19."""
    scorer, m64, cfg = scorers(name)
    s = cfg["vision_config"]["image_size"]
    px = torch.randn(8, 3, s, s, generator=torch.Generator().manual_seed(1)).half().float()
    ids = R.token_ids(8, 77, cfg["text_config"]["eos_token_id"], cfg["text_config"]["vocab_size"], seed=1)
    stock = R.small_clip_model(cfg, dtype=torch.float16, device="cuda")
    img64, txt64 = R.stock_features(m64, pixel_values=px.double()), R.stock_features(m64, input_ids=ids)
    img16, txt16 = R.stock_features(stock, pixel_values=px.cuda().half()), R.stock_features(stock, input_ids=ids.cuda())
    img, txt = scorer.get_image_features(px, normalize=True), scorer.get_text_features(ids, normalize=True)
    assert img.dtype == torch.float32 and img.shape == (8, cfg["projection_dim"]) and torch.isfinite(img).all() and torch.isfinite(txt).all()
    within_twice_the_stock_error(f"{name} image features", img, img16, img64)
    within_twice_the_stock_error(f"{name} text features", txt, txt16, txt64)
    from lavie_amd import ops
    sim = ops.clip_similarity(img, txt[:4].contiguous(), frames=2)
    sim16 = 100 * (img16.float().view(4, 2, -1) * txt16[:4].float()[:, None]).sum(-1).mean(-1)
    within_twice_the_stock_error(f"{name} clipsim", sim, sim16, R.similarity_reference(img64, txt64[:4], frames=2)[0])
    # unnormalised = get_*_features as transformers returns them
    raw = scorer.get_text_features(ids)
    assert torch.allclose(torch.nn.functional.normalize(raw, dim=-1), txt, atol=1e-6)


def test_features_do_not_depend_on_the_batch(scorers):
    scorer, _, cfg = scorers("patch32-eos2")
    pool = torch.from_numpy(np.stack([R.test_image(64, 96, seed=s) for s in range(8)])).cuda()
    single = [bits32(scorer._image_features_u8(pool[i:i + 1])[0]) for i in range(8)]
    for n in (1, 3, 8):
        order = [(i + 3) % 8 for i in range(n)]
        got = bits32(scorer._image_features_u8(pool[order]))
        for pos, i in enumerate(order):
            assert torch.equal(got[pos], single[i]), (n, pos, i)


def test_score_and_rank(scorers):
    scorer, m64, cfg = scorers("patch32-eos2")
    g = np.random.default_rng(7)
    # eight candidate clips of smooth random frames for ONE prompt; three with well separated float64 scores are kept
    base = g.integers(0, 256, (8, 1, 4, 6, 3))
    clips = np.clip(np.kron(base, np.ones((1, 4, 16, 16, 1))) + g.integers(-20, 21, (8, 4, 64, 96, 3)), 0, 255).astype(np.uint8)
    ids = R.token_ids(1, 77, 2, cfg["text_config"]["vocab_size"], seed=5)
    px64 = torch.from_numpy(np.stack([R.preprocess(f, 64, 64) for f in clips.reshape(32, 64, 96, 3)])).double()
    s64 = R.similarity_reference(R.stock_features(m64, pixel_values=px64), R.stock_features(m64, input_ids=ids).expand(8, -1).contiguous(),
                                 frames=4)[0]
    order = s64.argsort()
    keep = [int(order[0]), int(order[4]), int(order[7])]
    video = torch.from_numpy(clips[keep]).cuda()
    ids3 = ids.expand(3, -1).contiguous()
    got = scorer.score(video, ids3)
    assert got.dtype == torch.float32 and got.shape == (3,)
    err = float((got.double().cpu() - s64[keep]).abs().max())
    gap = float((s64[keep][1:] - s64[keep][:-1]).abs().min())
    print(f"score: engine max error {err:.3e} against float64, smallest gap of the constructed case {gap:.3e}")
    assert gap > 4 * err
    assert scorer.rank(video, ids3) == [2, 1, 0]
    # two calls agree, and prompt 0 of a pair has its single-call bits
    pair = torch.from_numpy(clips[:2]).cuda()
    assert tuple(pair.shape) == (2, 4, 64, 96, 3)
    ids2 = R.token_ids(2, 77, 2, cfg["text_config"]["vocab_size"], seed=6)
    a, b = scorer.score(pair, ids2), scorer.score(pair, ids2)
    assert torch.equal(bits32(a), bits32(b))
    assert torch.equal(bits32(scorer.score(pair[:1], ids2[:1])), bits32(a[:1]))
    # logits_per_image: the matrix form on the same features
    logits = scorer.logits_per_image(pair.reshape(8, 64, 96, 3), ids2)
    assert logits.shape == (8, 2)
    want = 100.0 / 4 * (logits[:4, 0] / np.exp(scorer.logit_scale)).sum()
    assert abs(float(want) - float(a[0])) < 1e-3


# ------------------------------------------------------------------ the pipeline
PIPE_MAPPER = dict(input_dim=128, output_dim=128, num_layers=2, num_heads=4, dim_feedforward=256, seq_len_in=17, seq_len_out=77)


def test_pipeline_image_path_with_the_engine_processor(small):  # noqa: F811
    """uint8 image_tensor through HipCLIPImageProcessor + engine tower + engine mapper = the model's pixel_values through the tower
    passed as image_embeds, bit for bit; enable_engine_image_encoder(processor=True) wraps a stock processor to the same effect."""
    from transformers import CLIPImageProcessor
    from lavie_amd.clip_score import HipCLIPImageProcessor
    from lavie_amd.image_encoder import HipCLIPVisionModel, HipMappingNetwork
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, _ = small
    cfg = ic.TOWER_CONFIGS["tiny"]
    enc = HipCLIPVisionModel.from_state_dict(ic.tower_state_dict(cfg), cfg)
    mapper = HipMappingNetwork.from_checkpoint(ic.mapper_state_dict(PIPE_MAPPER), num_heads=4)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(1, 77, 128, generator=g).half(), torch.randn(1, 77, 128, generator=g).half()
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    img = R.test_image(80, 96, seed=4)
    image = torch.from_numpy(img).permute(2, 0, 1)[None].contiguous()              # uint8 [1, 3, 80, 96]
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4, num_inference_steps=2,
              guidance_scale=7.5, output_type="latent")
    run = lambda pipe, **more: pipe(generator=torch.Generator().manual_seed(3), **kw, **more).video
    s = cfg["image_size"]
    pipe = VideoGenPipeline(unet=net, clip_model=enc, clip_processor=HipCLIPImageProcessor(size=s, crop_size=s), mapper=mapper).to("cuda")
    a = run(pipe, image_tensor=image)
    feats = enc(pixel_values=torch.from_numpy(R.preprocess(img, s, s))[None]).last_hidden_state
    assert torch.isfinite(a).all() and torch.equal(a, run(pipe, image_embeds=feats))
    stock = CLIPImageProcessor(size={"shortest_edge": s}, crop_size={"height": s, "width": s})
    spipe = VideoGenPipeline(unet=net, clip_model=enc, clip_processor=stock, mapper=mapper).to("cuda")
    spipe.enable_engine_image_encoder()
    assert spipe.clip_processor is stock                                            # the default launches what it launched
    spipe.enable_engine_image_encoder(processor=True)
    assert isinstance(spipe.clip_processor, HipCLIPImageProcessor)
    assert torch.equal(run(spipe, image_tensor=image), a)
    assert spipe.clip_processor._stock is stock


# ------------------------------------------------------------------ the C ABI: pixels and ids in, a score out
def test_c_abi_from_pixels_and_ids_to_clipsim(scorers):
    """every step through ctypes on buffers torch only allocates: preprocess -> vision tower -> embed; text tower -> embed; similarity"""
    from lavie_amd import _lib, image_encoder as E, text_encoder as T
    scorer, m64, cfg = scorers("patch32-eos2")
    sd = m64.state_dict()
    L, hv, fv, held_v = c_build("vision", E.vision_config_c(E.vision_config_dict(cfg["vision_config"])), sd)
    _, ht, ft, held_t = c_build("text", T.config_c(T.config_dict(cfg["text_config"])), sd)
    P, F, H, W, D, C_ = 2, 4, 64, 96, cfg["projection_dim"], 128
    video = torch.from_numpy(np.stack([R.test_image(H, W, seed=s) for s in range(P * F)]).reshape(P, F, H, W, 3)).cuda()
    ids = R.token_ids(P, 77, 2, cfg["text_config"]["vocab_size"], seed=6)
    ids32 = ids.to(torch.int32).cuda()
    want = scorer.score(video, ids)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    f16 = lambda *shape: torch.empty(shape, dtype=torch.float16, device="cuda")
    px, hid_v, hid_t, fi, ft_, out = f32(P * F, 3, 64, 64), f16(P * F, 5, C_), f16(P, 77, C_), f32(P * F, D), f32(P, D), f32(P)
    cfg_c = _lib.ClipPreprocessConfigC()
    cfg_c.struct_size, cfg_c.size, cfg_c.crop = ctypes.sizeof(cfg_c), 64, 64
    cfg_c.mean[:], cfg_c.std[:] = R.CLIP_MEAN, R.CLIP_STD
    try:
        for (f, h, held) in ((fv, hv, held_v), (ft, ht, held_t)):
            for name, t in held:
                assert f("set_param")(h, name, ptr(t), t.numel()) == 0, L.lavie_last_error()
            assert f("finalize")(h, stream) == 0, L.lavie_last_error()
        sync()
        nbytes = L.lavie_clip_preprocess_workspace_bytes(P * F, H, W, 64, 64)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ok = lambda rc: (rc == 0, L.lavie_last_error())
        assert ok(L.lavie_clip_preprocess_u8(ptr(video), P * F, H, W, 3 * W, 3 * W * H, ptr(px), 1, ctypes.byref(cfg_c), ptr(ws), nbytes, stream))[0]
        assert ok(fv("encode")(hv, ptr(px), 1, P * F, ptr(hid_v), stream))[0], L.lavie_last_error()
        assert ok(L.lavie_clip_embed_f16(ptr(hid_v), P * F, 5, C_, None, 2, 0, ptr(scorer.post_ln_weight), ptr(scorer.post_ln_bias), scorer.eps,
                                         ptr(scorer.visual_projection), D, 1, ptr(fi), stream))[0], L.lavie_last_error()
        assert ok(ft("encode")(ht, ptr(ids32), P, 77, ptr(hid_t), stream))[0], L.lavie_last_error()
        assert ok(L.lavie_clip_embed_f16(ptr(hid_t), P, 77, C_, ptr(ids32), 2, 0, None, None, 0.0, ptr(scorer.text_projection), D, 1, ptr(ft_),
                                         stream))[0], L.lavie_last_error()
        assert ok(L.lavie_clip_similarity_f32(ptr(fi), ptr(ft_), ptr(out), P * F, P, D, F, 1.0, stream))[0], L.lavie_last_error()
        sync()
        assert torch.equal(bits32(out), bits32(want))
    finally:
        fv("destroy")(hv)
        ft("destroy")(ht)
