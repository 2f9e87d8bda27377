"""CPU: the host side of image conditioning on the engine — the state-dict key maps and config mirrors against
transformers, torch.nn and the library, the refusals of the new C entries and Python objects, and the yardsticks of
tests/imagecases.py themselves."""
import ctypes

import pytest
import torch

import imagecases as ic
import opcheck as oc

transformers = pytest.importorskip("transformers")


def lib():
    from lavie_amd import _lib
    return _lib.load(), _lib


def last_error():
    return lib()[0].lavie_last_error().decode()


def vision_cfg(**over):
    from lavie_amd import image_encoder as E
    return E.vision_config_c(E.vision_config_dict(dict(ic.TOWER_TINY, **over)))


def mapper_cfg(**over):
    from lavie_amd import image_encoder as E
    base = dict(input_dim=128, output_dim=128, layers=2, heads=2, dim_feedforward=256, seq_in=17, seq_out=7, eps=1e-5)
    return E.mapper_config_c(dict(base, **over))


# ------------------------------------------------------------------ the contracts with transformers and torch.nn
@pytest.mark.parametrize("name", list(ic.TOWER_CONFIGS))
def test_vision_state_dict_keys_match_transformers(name):
    from transformers import CLIPVisionConfig, CLIPVisionModel
    from lavie_amd import image_encoder as E
    with torch.device("meta"):
        stock = CLIPVisionModel(CLIPVisionConfig(**ic.TOWER_CONFIGS[name]))
    full = stock.state_dict()
    sd = E.normalize_vision_keys(full)
    want = E.vision_state_dict_keys(E.vision_config_dict(stock.config))
    assert sorted(sd) == sorted(want) and len(full) - len(sd) == 2            # post_layernorm.weight / .bias left out, nothing else
    L, _ = lib()
    h = ctypes.c_void_p()
    c = E.vision_config_c(E.vision_config_dict(stock.config))
    assert L.lavie_vision_create(ctypes.byref(c), ctypes.byref(h)) == 0, last_error()
    try:
        assert L.lavie_vision_num_params(h) == len(want)
        name_p, numel = ctypes.c_char_p(), ctypes.c_longlong()
        for i, k in enumerate(want):                     # the engine lists them in the same order, with the module's sizes
            assert L.lavie_vision_param_info(h, i, ctypes.byref(name_p), ctypes.byref(numel)) == 0
            assert name_p.value.decode() == k and numel.value == sd[k].numel(), (i, k)
        buf = (ctypes.c_char * 16)()
        for k in full:                                   # every key of the full state dict is known, in the spelling of this version
            rc = L.lavie_vision_set_param(h, k.encode(), buf, 1)
            assert rc == 0 or "expected" in last_error(), (k, last_error())
    finally:
        L.lavie_vision_destroy(h)


@pytest.mark.parametrize("name", list(ic.MAPPER_CONFIGS))
def test_mapper_state_dict_keys_match_the_module(name):
    from lavie_amd import image_encoder as E
    from lavie_amd.mapping import MappingNetwork
    cfg = ic.MAPPER_CONFIGS[name]
    with torch.device("meta"):
        stock = MappingNetwork(**cfg)
    full = stock.state_dict()
    want = E.mapper_state_dict_keys(cfg["num_layers"])
    assert sorted(want) == sorted(k for k in full if k not in E.MAPPER_IGNORED) and len(full) - len(want) == 2
    derived = E.mapper_config_from_state_dict(full, cfg["num_heads"])
    assert derived == dict(input_dim=cfg["input_dim"], output_dim=cfg["output_dim"], layers=cfg["num_layers"], heads=cfg["num_heads"],
                           dim_feedforward=cfg["dim_feedforward"], seq_in=cfg["seq_len_in"], seq_out=cfg["seq_len_out"], eps=1e-5)
    L, _ = lib()
    h = ctypes.c_void_p()
    c = E.mapper_config_c(derived)
    assert L.lavie_mapper_create(ctypes.byref(c), ctypes.byref(h)) == 0, last_error()
    try:
        assert L.lavie_mapper_num_params(h) == len(want)
        name_p, numel = ctypes.c_char_p(), ctypes.c_longlong()
        for i, k in enumerate(want):
            assert L.lavie_mapper_param_info(h, i, ctypes.byref(name_p), ctypes.byref(numel)) == 0
            assert name_p.value.decode() == k and numel.value == full[k].numel(), (i, k)
        buf = (ctypes.c_char * 16)()
        assert L.lavie_mapper_set_param(h, b"text_proj.weight", buf, 1) == 0 and L.lavie_mapper_set_param(h, b"text_proj.bias", buf, 1) == 0
    finally:
        L.lavie_mapper_destroy(h)


def test_mapping_network_default_is_unchanged_and_feedforward_is_read_off_a_checkpoint():
    from lavie_amd.mapping import MappingNetwork
    assert MappingNetwork(128, 128, 1, 2, 5, 3).state_dict()["transformer_decoder.layers.0.linear1.weight"].shape == (2048, 128)
    sd = ic.mapper_state_dict(ic.MAPPER_TINY)
    net = MappingNetwork.from_checkpoint(sd, num_heads=2)
    assert net.transformer_decoder.layers[0].linear1.out_features == 256


def test_config_mirrors_have_the_librarys_size():
    L, _lib = lib()
    assert ctypes.sizeof(_lib.VisionConfigC) == L.lavie_vision_config_size()
    assert ctypes.sizeof(_lib.MapperConfigC) == L.lavie_mapper_config_size()
    assert [f[0] for f in _lib.VisionConfigC._fields_] == ["struct_size", "hidden", "intermediate", "layers", "heads", "image_size",
                                                           "patch_size", "act", "eps"]
    assert [f[0] for f in _lib.MapperConfigC._fields_] == ["struct_size", "input_dim", "output_dim", "layers", "heads", "dim_feedforward",
                                                           "seq_in", "seq_out", "eps"]
    assert L.lavie_abi_version() == 8                                      # additive entries: the generation stays


def test_classic_flat_and_clip_model_keys_are_all_taken():
    from lavie_amd import image_encoder as E
    flat = {"embeddings.class_embedding": 1, "embeddings.position_ids": 2, "post_layernorm.weight": 3}
    classic = {"vision_model.embeddings.class_embedding": 1, "vision_model.embeddings.position_ids": 2, "vision_model.post_layernorm.weight": 3,
               "text_model.embeddings.token_embedding.weight": 4, "visual_projection.weight": 5, "logit_scale": 6}
    assert E.normalize_vision_keys(flat) == E.normalize_vision_keys(classic) == {"vision_model.embeddings.class_embedding": 1}


# ------------------------------------------------------------------ refusals of the C entries (no GPU: every check precedes the first HIP call)
def test_create_refusals_name_the_argument():
    L, _ = lib()
    h = ctypes.c_void_p()
    c = vision_cfg()
    c.struct_size -= 4
    assert L.lavie_vision_create(ctypes.byref(c), ctypes.byref(h)) != 0 and "struct_size" in last_error()
    assert L.lavie_vision_create(None, ctypes.byref(h)) != 0 and "null" in last_error()
    for field, value, word in (("hidden", 96, "hidden"), ("hidden", 4096, "hidden"), ("intermediate", 200, "intermediate"),
                               ("layers", 0, "layers"), ("heads", 3, "heads"), ("heads", 1, "heads"), ("image_size", 57, "image_size"),
                               ("image_size", 336, "577 tokens"), ("patch_size", 0, "patch_size"), ("act", 2, "act"), ("eps", 0.0, "eps")):
        c = vision_cfg()
        setattr(c, field, value)
        assert L.lavie_vision_create(ctypes.byref(c), ctypes.byref(h)) != 0, (field, value)
        assert word in last_error(), (field, last_error())
    m = mapper_cfg()
    m.struct_size += 4
    assert L.lavie_mapper_create(ctypes.byref(m), ctypes.byref(h)) != 0 and "struct_size" in last_error()
    for field, value, word in (("input_dim", 100, "input_dim"), ("output_dim", 96, "output_dim"), ("layers", 0, "layers"),
                               ("heads", 3, "heads"), ("dim_feedforward", 200, "dim_feedforward"), ("seq_in", 321, "seq_in"),
                               ("seq_out", 321, "seq_out"), ("seq_out", 0, "seq_out"), ("eps", 0.0, "eps")):
        m = mapper_cfg(**{field: value})
        assert L.lavie_mapper_create(ctypes.byref(m), ctypes.byref(h)) != 0, (field, value)
        assert word in last_error(), (field, last_error())


def test_handle_refusals():
    L, _ = lib()
    buf = (ctypes.c_char * 16)()
    h = ctypes.c_void_p()
    c = vision_cfg()
    assert L.lavie_vision_create(ctypes.byref(c), ctypes.byref(h)) == 0
    try:
        assert L.lavie_vision_set_param(h, b"vision_model.nope", buf, 8) != 0 and "unknown state-dict key" in last_error()
        assert L.lavie_vision_set_param(h, b"pre_layrnorm.bias", buf, 8) != 0 and "expected 128" in last_error()
        assert L.lavie_vision_set_param(h, b"vision_model.pre_layrnorm.bias", None, 128) != 0 and "null data" in last_error()
        assert L.lavie_vision_finalize(h, None) != 0 and "was never set" in last_error() and "class_embedding" in last_error()
        assert L.lavie_vision_encode(h, buf, 1, 1, buf, None) != 0 and "not finalized" in last_error()
        assert L.lavie_vision_param_info(h, 999, None, None) != 0 and "out of range" in last_error()
        for b, word in ((0, "B=0"), (17, "B=17")):
            assert L.lavie_vision_workspace_bytes(h, b) == -1 and word in last_error()
        m = 2 * 17
        assert L.lavie_vision_workspace_bytes(h, 2) == 2 * m * 128 * 2 + m * 3 * 128 * 2 + 2 * 16 * 640 * 2      # x | h | wide | patches
    finally:
        L.lavie_vision_destroy(h)
    assert L.lavie_vision_encode(None, None, 0, 1, None, None) != 0 and "null handle" in last_error()
    assert L.lavie_vision_workspace_bytes(None, 1) == -1 and L.lavie_vision_num_params(None) == -1
    m = mapper_cfg()
    assert L.lavie_mapper_create(ctypes.byref(m), ctypes.byref(h)) == 0
    try:
        assert L.lavie_mapper_set_param(h, b"nope", buf, 8) != 0 and "unknown state-dict key" in last_error()
        assert L.lavie_mapper_set_param(h, b"image_proj.bias", buf, 8) != 0 and "expected 128" in last_error()
        assert L.lavie_mapper_finalize(h, None) != 0 and "was never set" in last_error() and "image_pos_embedding" in last_error()
        assert L.lavie_mapper_encode(h, buf, 1, buf, 1, buf, 7, 0, None) != 0 and "not finalized" in last_error()
        for b, word in ((0, "B=0"), (17, "B=17")):
            assert L.lavie_mapper_workspace_bytes(h, b) == -1 and word in last_error()
    finally:
        L.lavie_mapper_destroy(h)
    assert L.lavie_mapper_encode(None, None, 1, None, 1, None, 7, 0, None) != 0 and "null handle" in last_error()


def test_operator_refusals_launch_nothing():
    """every check of the launchers precedes the launch: on a machine without a device a refusal is all that can come back"""
    L, _ = lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    base = dict(q=p, ldq=64, k=p, ldk=64, v=p, ldv=64, o=p, ldo=64, NB=1, Lq=16, Lk=16, heads=1, dh=64, scale=0.125, stream=None)
    att = lambda **k: L.lavie_short_attention_f16(*{**base, **k}.values())
    for kw, word in ((dict(Lq=321), "Lq=321"), (dict(Lk=321), "Lk=321"), (dict(Lk=0), "Lk=0"), (dict(Lq=0), "Lq=0"), (dict(dh=40), "dh=40"),
                     (dict(NB=0), "NB=0"), (dict(ldq=68), "ldq=68"), (dict(ldk=56), "ldk=56"), (dict(ldv=66), "ldv=66"), (dict(ldo=60), "ldo=60"),
                     (dict(k=None), "null"), (dict(scale=float("nan")), "scale"), (dict(v=ctypes.c_void_p(p.value + 2)), "aligned")):
        assert att(**kw) != 0 and word in last_error(), (kw, last_error())
    pe = lambda px=p, dt=1, B=1, S=56, P=14, C=128: L.lavie_patch_embed_f16(px, dt, p, p, p, p, p, B, S, P, C, None)
    for kw, word in ((dict(dt=2), "x_dtype=2"), (dict(B=0), "B=0"), (dict(S=57), "S=57"), (dict(P=0), "P=0"), (dict(C=96), "C=96"),
                     (dict(px=None), "null")):
        assert pe(**kw) != 0 and word in last_error(), (kw, last_error())
    assert L.lavie_patch_embed_k(14) == 640 and L.lavie_patch_embed_k(16) == 768 and L.lavie_patch_embed_k(65) == -1
    assert L.lavie_patch_embed_workspace_bytes(3, 224, 14) == 3 * 256 * 640 * 2 and L.lavie_patch_embed_workspace_bytes(1, 30, 14) == -1
    for args, word in (((p, 0), "n=0"), ((None, 8), "null")):
        assert L.lavie_relu_f16(*args, None) != 0 and word in last_error(), (args, last_error())
    assert L.lavie_act_f16(p, 8, 2, None) != 0 and "kind=2" in last_error()      # relu is an entry of its own; this one is unchanged


# ------------------------------------------------------------------ refusals of the Python objects
def test_python_refusals():
    from lavie_amd import image_encoder as E
    with pytest.raises(ValueError, match="hidden_act"):
        E.vision_config_c(E.vision_config_dict(dict(ic.TOWER_TINY, hidden_act="gelu_new")))
    with pytest.raises(ValueError, match="lacks"):
        E.vision_config_dict({"hidden_size": 10})
    enc = E.HipCLIPVisionModel.__new__(E.HipCLIPVisionModel)          # the argument checks of __call__ precede any device work
    enc._cfg, enc._h = E.vision_config_dict(ic.TOWER_TINY), None
    px = torch.zeros(1, 3, 56, 56)
    for kw, word in ((dict(output_hidden_states=True), "output_hidden_states"), (dict(output_attentions=True), "output_attentions"),
                     (dict(interpolate_pos_encoding=True), "interpolate_pos_encoding")):
        with pytest.raises(NotImplementedError, match=word):
            enc(pixel_values=px, **kw)
    with pytest.raises(ValueError, match="image size"):
        enc(pixel_values=torch.zeros(1, 3, 42, 42))
    with pytest.raises(ValueError, match=r"\[B, 3, S, S\]"):
        enc(pixel_values=torch.zeros(1, 1, 56, 56))
    assert enc.vision_model is enc and enc.tokens == 17
    out = E.VisionEncoderOutput(px)
    assert out[0] is px and out.last_hidden_state is px
    with pytest.raises(NotImplementedError, match="pooler_output"):
        out.pooler_output
    with pytest.raises(ValueError, match="missing key"):
        E.HipMappingNetwork({"image_proj.weight": torch.zeros(8, 8)})
    net = E.HipMappingNetwork.__new__(E.HipMappingNetwork)
    net._cfg, net._h = E.mapper_config_from_state_dict(ic.mapper_state_dict(ic.MAPPER_TINY), 2), None
    with pytest.raises(ValueError, match="image_embeds"):
        net(torch.zeros(1, 16, 128), torch.zeros(1, 7, 128))
    with pytest.raises(ValueError, match="text_embeds"):
        net(torch.zeros(1, 17, 128), torch.zeros(1, 8, 128))
    with pytest.raises(ValueError, match="2 images for 3 prompts"):
        net(torch.zeros(2, 17, 128), torch.zeros(3, 7, 128))


def test_pipeline_switch_needs_the_parts():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline(unet=object())
    with pytest.raises(ValueError, match="no clip_model or mapper"):
        pipe.enable_engine_image_encoder()
    pipe.disable_engine_image_encoder()                             # nothing wrapped: nothing to do


# ------------------------------------------------------------------ the yardsticks themselves
@pytest.mark.parametrize("name", ["tiny", "dh32", "patch16-gelu"])
def test_tower_reference64_is_transformers_in_float64(name):
    """pins the pre-norm order, pre_layrnorm, and that last_hidden_state carries no post_layernorm"""
    cfg = ic.TOWER_CONFIGS[name]
    sd, px = ic.tower_state_dict(cfg), ic.tower_pixels(cfg)
    with torch.no_grad():
        want = ic.stock_tower(sd, cfg, torch.float64)(pixel_values=px.double()).last_hidden_state
    got = ic.tower_reference64(sd, cfg, px)
    assert got.dtype == torch.float64 and (got - want).abs().max() <= 1e-10 * want.abs().max(), name


@pytest.mark.parametrize("name", ["tiny"])
def test_mapper_reference64_is_the_module_in_float64(name):
    """pins the post-norm order, the q | k | v split of in_proj_weight, ReLU, and that there is no final norm"""
    cfg = ic.MAPPER_CONFIGS[name]
    sd = ic.mapper_state_dict(cfg)
    for bi in (None, 1):
        img, txt = ic.mapper_inputs(cfg, bi=bi)
        with torch.no_grad():
            want = ic.stock_mapper(sd, cfg, torch.float64)(img.double().expand(txt.shape[0], -1, -1), txt.double())
        got = ic.mapper_reference64(sd, cfg, img, txt)
        assert got.dtype == torch.float64 and (got - want).abs().max() <= 1e-10 * want.abs().max(), (name, bi)


@pytest.mark.parametrize("nb,heads,dh", ic.ATT_SHAPES)
def test_attention_model_meets_its_bound(nb, heads, dh):
    """the fp32 model of the kernel, with fp16 roundings at the counted points, against float64: the bound is reachable"""
    for lq, lk, hard in [(1, 1, False), (17, 15, False), (77, 257, False), (320, 320, False), (ic.HARD_LQ, ic.HARD_LK, True)]:
        case = ic.attention_case(nb, heads, dh, lq, lk, hard=hard)
        ref, scale = case["ref"]()
        got = case["model"]()
        assert torch.isfinite(got).all()
        oc.assert_elementwise(got, ref, scale, ic.ATT_C, where=case["where"], label=f"model:short[{nb},{heads},{dh},{lq},{lk},{hard}]")


def test_hard_rows_are_hard():
    mid, last, dom = ic.hard_rows()
    assert all(64 <= m < 256 for _, m in mid) and all(m == ic.HARD_LK - 1 == 256 for _, m in last) and all(d >= 64 for _, d in dom)
    rows = [r for r, _ in mid + last + dom]
    assert len(set(rows)) == len(rows) and all(0 <= r < ic.HARD_LQ for r in rows)
    case = ic.attention_case(1, 1, 64, ic.HARD_LQ, ic.HARD_LK, hard=True)       # the construction asserts its own premises
    assert torch.isnan(case["tensors"]["k"][ic.HARD_LK:]).all()                   # a read past the last key meets NaN


@pytest.mark.parametrize("p,s,c", ic.PATCH_CONFIGS[:2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_patch_model_meets_its_bound(p, s, c, dtype):
    case = ic.patch_case(p, s, c, 1, dtype)
    ref, scale = ic.patch_ref(case)
    oc.assert_elementwise(ic.patch_model(case), ref, scale, ic.PATCH_C, where=oc.loc_rows(c), label=f"model:patch[{p},{s},{c}]")
    w = torch.nn.functional.conv2d(case["px"].double(), case["w"].double(), stride=p).flatten(2).transpose(1, 2)
    assert (ref[:, 1:] - (w + case["pos"][1:].double())).abs().max() < 1e-12    # the unfold order is the conv weight's flattening


def test_relu_input_has_the_edge_values():
    x = ic.relu_input(4099)
    bits = x.view(torch.int16)
    assert bits[0] == 0 and bits[1] == -32768 and x[2] < 0 and x[3] > 0 and x.abs().max() == 65504
    assert torch.relu(x).view(torch.int16)[1] == -32768                         # torch keeps -0
