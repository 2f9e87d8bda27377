"""-m gpu: image conditioning on the engine — the new kernels per element on guarded operands, the vision tower
and the mapper against float64 with the stock fp16 modules as the yardstick of what fp16 storage costs, the bit guarantees, the C
ABI without wrapper objects, and the pipeline's image path."""
import ctypes
import json
import os
from types import SimpleNamespace

import pytest
import torch

import imagecases as ic
import opcheck as oc
from test_gpu_image_cond import small  # noqa: F401  (the `small` UNet fixture, as it is)

pytestmark = pytest.mark.gpu

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "image_encoder.json")


def sync():
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------ short attention
def run_attention(case, ldo_pad=0):
    from lavie_amd import ops
    nb, heads, dh, lq, lk, c = (case[k] for k in ("nb", "heads", "dh", "lq", "lk", "c"))

    def fn(i, o):
        if case["packed"]:
            q, k, v = i["qkv"][:, :c], i["qkv"][:, c:2 * c], i["qkv"][:, 2 * c:3 * c]
        else:
            q, k, v = i["q"], i["k"], i["v"]
        ops.short_attention(q, k, v, nb, lq, lk, heads, dh, out=o["y"])

    mask = torch.zeros(nb * lq, c + ldo_pad, dtype=torch.bool)
    mask[:, :c] = True
    out = oc.run_guarded(fn, case["tensors"], {"y": ((nb * lq, c + ldo_pad), torch.float16)}, sync=sync,
                         partial={"y": mask} if ldo_pad else None)
    y = out["y"][:, :c]
    assert torch.isfinite(y).all()
    ref, scale = case["ref"]()
    oc.assert_elementwise(y, ref, scale, ic.ATT_C, where=case["where"], label=f"short[nb{nb},h{heads},dh{dh},lq{lq},lk{lk}]")


@pytest.mark.parametrize("nb,heads,dh", ic.ATT_SHAPES)
@pytest.mark.parametrize("lq,lk", ic.ATT_LENGTHS)
def test_short_attention_per_element(nb, heads, dh, lq, lk):
    run_attention(ic.attention_case(nb, heads, dh, lq, lk))


@pytest.mark.parametrize("nb,heads,dh", ic.ATT_SHAPES)
def test_short_attention_wider_rows_with_distinct_pitches(nb, heads, dh):
    """q, k, v and o each with a pitch of its own, the padding columns NaN (o's keep their poison)"""
    run_attention(ic.attention_case(nb, heads, dh, 77, 257, pads=(8, 16, 24)), ldo_pad=32)


@pytest.mark.parametrize("nb,heads,dh", ic.ATT_SHAPES)
def test_short_attention_on_columns_of_one_packed_tensor(nb, heads, dh):
    run_attention(ic.attention_case(nb, heads, dh, 257, 257, pads=(8, 0, 0), packed=True), ldo_pad=8)


@pytest.mark.parametrize("nb,heads,dh", ic.ATT_SHAPES)
def test_short_attention_hard_logits(nb, heads, dh):
    run_attention(ic.attention_case(nb, heads, dh, ic.HARD_LQ, ic.HARD_LK, hard=True))


@pytest.mark.parametrize("kw,word", [(dict(lq=321), "Lq=321"), (dict(lk=321), "Lk=321"), (dict(lk=0), "Lk=0"), (dict(dh=40), "dh=40"),
                                     (dict(nb=0), "NB=0"), (dict(kpad=4), "ldk=")])
def test_short_attention_refusals_leave_the_output_alone(kw, word):
    from lavie_amd import ops
    a = dict(nb=1, lq=16, lk=16, heads=2, dh=64, kpad=0)
    a.update(kw)
    c = a["heads"] * a["dh"]
    q = torch.zeros(max(a["nb"], 1) * a["lq"], c, dtype=torch.float16, device="cuda")
    k = torch.zeros(max(a["nb"], 1) * max(a["lk"], 1), c + a["kpad"], dtype=torch.float16, device="cuda")
    y = oc.guarded((q.shape[0], c), torch.float16)
    with pytest.raises(RuntimeError, match=word):
        ops.short_attention(q, k, k, a["nb"], a["lq"], a["lk"], a["heads"], a["dh"], out=y.t)
    sync()
    y.check_bands("y (refused call)")
    assert y.unwritten().numel() == y.n                                  # the poison is intact


# ------------------------------------------------------------------ patch embedding
def run_patch(case):
    from lavie_amd import ops
    p, c, b, t = case["p"], case["c"], case["b"], case["t"]
    fn = lambda i, o: ops.patch_embed(i["px"], ops.pack_patch_embed(i["w"]), i["cls"], i["pos"], p, out=o["y"])
    return oc.run_guarded(fn, {k: case[k] for k in ("px", "w", "cls", "pos")}, {"y": ((b, t, c), torch.float16)}, sync=sync)["y"]


@pytest.mark.parametrize("p,s,c", ic.PATCH_CONFIGS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_patch_embed_per_element_and_batch_invariant(p, s, c, dtype):
    """against the float64 convolution + class + position; entry b of B = 3 has the bits of its B = 1 call"""
    three = ic.patch_case(p, s, c, 3, dtype)
    y3 = run_patch(three)
    ref, scale = ic.patch_ref(three)
    oc.assert_elementwise(y3, ref, scale, ic.PATCH_C, where=oc.loc_rows(c), label=f"patch[{p},{s},{c},{dtype}]")
    oc.assert_bits(y3[:, 0], (three["cls"].float() + three["pos"][0].float()).half().expand(3, c), label="class row")
    for b in range(3):
        one = dict(three, px=three["px"][b:b + 1].contiguous(), b=1)
        oc.assert_bits(run_patch(one)[0], y3[b], where=oc.loc_rows(c), label=f"patch entry {b} alone")


# ------------------------------------------------------------------ relu
@pytest.mark.parametrize("n", ic.ACT_SIZES)
def test_relu_is_torch_relu_bit_for_bit(n):
    from lavie_amd import ops
    x = ic.relu_input(n)
    out = oc.run_guarded(lambda i, o: ops.relu(i["x"]), {"x": x}, {"y": ((n,), torch.float16)}, alias={"y": "x"}, sync=sync)
    oc.assert_bits(out["y"], torch.relu(x), label=f"relu[{n}]")


# ------------------------------------------------------------------ the models
@pytest.fixture(scope="module")
def towers():
    """name -> (engine tower, state dict, config), built once"""
    from lavie_amd.image_encoder import HipCLIPVisionModel
    built = {}

    def get(name):
        if name not in built:
            cfg = ic.TOWER_CONFIGS[name]
            sd = ic.tower_state_dict(cfg)
            built[name] = (HipCLIPVisionModel.from_state_dict(sd, cfg), sd, cfg)
        return built[name]
    return get


@pytest.fixture(scope="module")
def mappers():
    from lavie_amd.image_encoder import HipMappingNetwork
    built = {}

    def get(name):
        if name not in built:
            cfg = ic.MAPPER_CONFIGS[name]
            sd = ic.mapper_state_dict(cfg)
            built[name] = (HipMappingNetwork.from_checkpoint(sd, num_heads=cfg["num_heads"]), sd, cfg)
        return built[name]
    return get


def record(name, pair):
    """the measured (engine, stock) error pairs go to profiles/image_encoder.json, beside the timings of tools/bench_image_encoder.py"""
    try:
        with open(PROFILE) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc.setdefault("errors_vs_float64", {})[name] = pair
    try:
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def within_twice_the_stock_error(name, got, stock, ref):
    e_rel, e_max = ic.errors(got, ref)
    s_rel, s_max = ic.errors(stock, ref)
    print(f"{name}: engine rel-L2 {e_rel:.3e} max {e_max:.3e}; stock fp16 rel-L2 {s_rel:.3e} max {s_max:.3e}")
    record(name, {"engine": {"rel_l2": e_rel, "max": e_max}, "stock_fp16": {"rel_l2": s_rel, "max": s_max}})
    assert e_rel <= 2 * s_rel and e_max <= 2 * s_max, (e_rel, s_rel, e_max, s_max)


@pytest.mark.parametrize("name", list(ic.TOWER_CONFIGS))
def test_tower_against_float64_within_twice_the_stock_fp16_error(name, towers):
    """Yardstick: the written-out float64 reference (equal to transformers in float64, test_image_encoder_host.py) on the same
    fp16-rounded weights.  The engine's rel-L2 and max per-element error must not exceed twice those of the stock module in fp16 on
    the device.  Measured on an MI355X: see profiles/image_encoder.json."""
    enc, sd, cfg = towers(name)
    px = ic.tower_pixels(cfg)
    ref = ic.tower_reference64(sd, cfg, px)
    with torch.no_grad():
        stock = ic.stock_tower(sd, cfg, torch.float16, "cuda")(pixel_values=px.cuda().half()).last_hidden_state
    out = enc(pixel_values=px)
    got = out[0]
    assert got is out.last_hidden_state and got.dtype == torch.float16 and got.shape == (ic.MODEL_B, enc.tokens, cfg["hidden_size"])
    assert got.is_cuda and torch.isfinite(got).all()
    within_twice_the_stock_error("tower " + name, got, stock, ref)


@pytest.mark.parametrize("name", list(ic.MAPPER_CONFIGS))
def test_mapper_against_float64_within_twice_the_stock_fp16_error(name, mappers):
    net, sd, cfg = mappers(name)
    img, txt = ic.mapper_inputs(cfg)
    ref = ic.mapper_reference64(sd, cfg, img, txt)
    with torch.no_grad():
        stock = ic.stock_mapper(sd, cfg, torch.float16, "cuda")(img.cuda(), txt.cuda())
    got = net(img, txt)
    assert got.dtype == torch.float16 and got.shape == (ic.MODEL_B, cfg["seq_len_out"], cfg["output_dim"]) and torch.isfinite(got).all()
    within_twice_the_stock_error("mapper " + name, got, stock, ref)


# ------------------------------------------------------------------ bits
def test_two_calls_agree_bit_for_bit(towers, mappers):
    enc, _, cfg = towers("tiny")
    px = ic.tower_pixels(cfg, b=3)
    assert torch.equal(bits(enc(pixel_values=px)[0]), bits(enc(pixel_values=px)[0]))
    net, _, mcfg = mappers("tiny")
    img, txt = ic.mapper_inputs(mcfg, b=3)
    assert torch.equal(bits(net(img, txt)), bits(net(img, txt)))


@pytest.mark.parametrize("name,sizes", [("tiny", tuple(range(1, 17))), ("vit-l-1layer", (1, 3, 16))])
def test_an_image_has_the_same_bits_in_every_batch(name, sizes, towers):
    """every batch size, every position in the batch: pinned GEMMs, per-image patch GEMMs, (entry, head) attention"""
    enc, _, cfg = towers(name)
    pool = ic.tower_pixels(cfg, b=16, seed=5).cuda()
    single = [bits(enc(pixel_values=pool[i:i + 1])[0][0]) for i in range(16)]
    for n in sizes:
        for shift in (0, 7):                                     # two orders: every image meets several positions
            order = [(i + shift) % 16 for i in range(n)]
            got = bits(enc(pixel_values=pool[order])[0])
            for pos, i in enumerate(order):
                assert torch.equal(got[pos], single[i]), (name, n, pos, i)


@pytest.mark.parametrize("name,sizes", [("tiny", tuple(range(1, 17))), ("prod-1layer", (1, 3, 16))])
def test_a_mapper_entry_has_the_same_bits_in_every_batch_and_under_broadcast(name, sizes, mappers):
    net, _, cfg = mappers(name)
    img, txt = (t.cuda() for t in ic.mapper_inputs(cfg, b=16, seed=5))
    single = [bits(net(img[i:i + 1], txt[i:i + 1])[0]) for i in range(16)]
    shared = [bits(net(img[:1], txt[i:i + 1])[0]) for i in range(16)]          # every prompt with image 0
    for n in sizes:
        for shift in (0, 7):
            order = [(i + shift) % 16 for i in range(n)]
            got = bits(net(img[order], txt[order]))
            one_image = bits(net(img[:1], txt[order]))                          # Bi = 1: broadcast inside the engine
            repeated = bits(net(img[:1].expand(n, -1, -1), txt[order]))         # Bi = B with the image repeated
            for pos, i in enumerate(order):
                assert torch.equal(got[pos], single[i]), (name, n, pos, i)
                assert torch.equal(one_image[pos], shared[i]) and torch.equal(repeated[pos], shared[i]), (name, n, pos, i)


def test_mapper_writes_behind_the_text_rows_of_a_context_buffer(mappers):
    """row0 = 77 of a 154-row buffer: rows 0..76 keep their poison bit for bit, rows 77..153 are the plain call's"""
    net, _, cfg = mappers("prod-1layer")
    img, txt = ic.mapper_inputs(cfg, b=3, seed=2)
    plain = net(img[:1], txt)
    ctx = oc.guarded((3, 154, cfg["output_dim"]), torch.float16)
    assert net(img[:1], txt, out=ctx.t, row0=77) is ctx.t
    sync()
    ctx.check_bands("context buffer")
    mask = torch.zeros(3, 154, cfg["output_dim"], dtype=torch.bool)
    mask[:, 77:] = True
    ctx.check_written("context buffer", mask=mask)
    assert torch.equal(bits(ctx.t[:, 77:]), bits(plain))
    with pytest.raises(RuntimeError, match="row0=78"):
        net(img[:1], txt, out=ctx.t, row0=78)


# ------------------------------------------------------------------ the C ABI with no wrapper objects
def c_build(prefix, cfg_c, sd, normalize=lambda k: k):
    """create -> set_param for every listed name -> finalize, through ctypes alone; returns (library, handle, held tensors)"""
    from lavie_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    f = lambda n: getattr(L, f"lavie_{prefix}_{n}")
    assert f("create")(ctypes.byref(cfg_c), ctypes.byref(h)) == 0, L.lavie_last_error()
    held, name_p, numel = [], ctypes.c_char_p(), ctypes.c_longlong()
    for i in range(f("num_params")(h)):
        assert f("param_info")(h, i, ctypes.byref(name_p), ctypes.byref(numel)) == 0
        t = sd[normalize(name_p.value.decode())].cuda().half().contiguous()
        assert t.numel() == numel.value
        held.append((name_p.value, t))
    return L, h, f, held


def test_vision_c_abi_matches_the_python_class(towers):
    from lavie_amd import image_encoder as E
    enc, sd, cfg = towers("tiny")
    c = E.vision_config_c(E.vision_config_dict(cfg))
    L, h, f, held = c_build("vision", c, sd)
    px = ic.tower_pixels(cfg, b=2, seed=3).cuda()
    out = torch.zeros(2, 17, 128, dtype=torch.float16, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        bad = E.vision_config_c(E.vision_config_dict(cfg))
        bad.struct_size += 4
        assert L.lavie_vision_create(ctypes.byref(bad), ctypes.byref(ctypes.c_void_p())) != 0 and b"struct_size" in L.lavie_last_error()
        for name, t in held[1:]:
            assert f("set_param")(h, name, ctypes.c_void_p(t.data_ptr()), t.numel()) == 0
        assert f("finalize")(h, stream) != 0 and held[0][0] in L.lavie_last_error()                # the missing parameter is named
        assert f("encode")(h, ctypes.c_void_p(px.data_ptr()), 1, 2, ctypes.c_void_p(out.data_ptr()), stream) != 0
        assert b"not finalized" in L.lavie_last_error()
        assert f("set_param")(h, held[0][0], ctypes.c_void_p(held[0][1].data_ptr()), held[0][1].numel()) == 0
        assert f("finalize")(h, stream) == 0, L.lavie_last_error()
        sync()
        assert f("workspace_bytes")(h, 17) == -1 and f("workspace_bytes")(h, 2) > 0
        assert f("encode")(h, ctypes.c_void_p(px.data_ptr()), 1, 2, ctypes.c_void_p(out.data_ptr()), stream) == 0, L.lavie_last_error()
        sync()
        assert torch.equal(bits(out), bits(enc(pixel_values=px)[0]))
    finally:
        f("destroy")(h)


def test_mapper_c_abi_matches_the_python_class(mappers):
    from lavie_amd import image_encoder as E
    net, sd, cfg = mappers("tiny")
    c = E.mapper_config_c(E.mapper_config_from_state_dict(sd, cfg["num_heads"]))
    L, h, f, held = c_build("mapper", c, sd)
    img, txt = (t.cuda() for t in ic.mapper_inputs(cfg, b=2, seed=3))
    out = torch.zeros(2, 7, 128, dtype=torch.float16, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    enc_args = lambda: (h, ctypes.c_void_p(img.data_ptr()), 2, ctypes.c_void_p(txt.data_ptr()), 2, ctypes.c_void_p(out.data_ptr()), 7, 0, stream)
    try:
        bad = E.mapper_config_c(E.mapper_config_from_state_dict(sd, cfg["num_heads"]))
        bad.struct_size -= 4
        assert L.lavie_mapper_create(ctypes.byref(bad), ctypes.byref(ctypes.c_void_p())) != 0 and b"struct_size" in L.lavie_last_error()
        for name, t in held[:-1]:
            assert f("set_param")(h, name, ctypes.c_void_p(t.data_ptr()), t.numel()) == 0
        assert f("finalize")(h, stream) != 0 and held[-1][0] in L.lavie_last_error()
        assert f("encode")(*enc_args()) != 0 and b"not finalized" in L.lavie_last_error()
        assert f("set_param")(h, held[-1][0], ctypes.c_void_p(held[-1][1].data_ptr()), held[-1][1].numel()) == 0
        assert f("finalize")(h, stream) == 0, L.lavie_last_error()
        sync()
        assert f("workspace_bytes")(h, 17) == -1 and f("workspace_bytes")(h, 2) > 0
        assert f("encode")(*enc_args()) == 0, L.lavie_last_error()
        sync()
        assert torch.equal(bits(out), bits(net(img, txt)))
    finally:
        f("destroy")(h)


# ------------------------------------------------------------------ the pipeline
class Proc:                      # stand-in for CLIPImageProcessor (resize + normalise), the caller's part as the tokenizer is
    def __call__(self, images=None, return_tensors="pt"):
        x = torch.nn.functional.interpolate(images.float(), size=(56, 56), mode="bilinear", align_corners=False)
        return SimpleNamespace(pixel_values=(x - 0.45) / 0.27)


PIPE_MAPPER = dict(input_dim=128, output_dim=128, num_layers=2, num_heads=4, dim_feedforward=256, seq_len_in=17, seq_len_out=77)


def test_pipeline_image_path_on_the_engine(small, towers):  # noqa: F811
    """image_tensor through engine tower + engine mapper = passing the engine tower's output as image_embeds, bit for bit; within
    rel-L2 1e-2 of the stock tower + stock mapper in fp16; enable / disable swap the stock objects; no image: nothing changes."""
    from lavie_amd.image_encoder import HipCLIPVisionModel, HipMappingNetwork
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, _ = small
    enc, sd, cfg = towers("tiny")
    msd = ic.mapper_state_dict(PIPE_MAPPER)
    mapper = HipMappingNetwork.from_checkpoint(msd, num_heads=4)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(1, 77, 128, generator=g).half(), torch.randn(1, 77, 128, generator=g).half()
    image = torch.rand(1, 3, 80, 96, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4, num_inference_steps=2,
              guidance_scale=7.5, output_type="latent")
    run = lambda pipe, **more: pipe(generator=torch.Generator().manual_seed(3), **kw, **more).video
    pipe = VideoGenPipeline(unet=net, clip_model=enc, clip_processor=Proc(), mapper=mapper)
    assert pipe.to("cuda") is pipe
    a = run(pipe, image_tensor=image)
    feats = enc(pixel_values=Proc()(images=image).pixel_values).last_hidden_state
    b = run(pipe, image_embeds=feats)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # the stock pair in fp16, wrapped and unwrapped
    stock_tower, stock_mapper = ic.stock_tower(sd, cfg, torch.float16, "cuda"), ic.stock_mapper(msd, PIPE_MAPPER, torch.float16, "cuda")
    spipe = VideoGenPipeline(unet=net, clip_model=stock_tower, clip_processor=Proc(), mapper=stock_mapper)
    ref = run(spipe, image_tensor=image)
    rel = float((a.float() - ref.float()).norm() / ref.float().norm())
    print(f"pipeline latents, engine image path against the stock fp16 pair: rel-L2 {rel:.3e}")
    assert rel < 1e-2
    spipe.enable_engine_image_encoder()
    assert isinstance(spipe.clip_model, HipCLIPVisionModel) and isinstance(spipe.mapper, HipMappingNetwork)
    assert torch.equal(run(spipe, image_tensor=image), a)
    spipe.disable_engine_image_encoder()
    assert spipe.clip_model is stock_tower and spipe.mapper is stock_mapper
    loaded = VideoGenPipeline(unet=net).load_mapper(msd, num_heads=4, engine=True)
    assert isinstance(loaded, HipMappingNetwork) and torch.equal(bits(loaded(feats, pe)), bits(mapper(feats, pe)))
    # a call without an image: the parts are not consulted, the latents are those of a pipeline without them
    assert torch.equal(run(pipe), run(VideoGenPipeline(unet=net)))
