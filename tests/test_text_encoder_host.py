"""CPU: the text encoder's host side — the state-dict key map and the config mirror against transformers and the
library, every refusal of the new C entries and of the Python object, and the yardsticks of tests/textcases.py themselves."""
import ctypes

import pytest
import torch

import opcheck as oc
import textcases as tc

transformers = pytest.importorskip("transformers")


def lib():
    from lavie_amd import _lib
    return _lib.load(), _lib


def last_error():
    return lib()[0].lavie_last_error().decode()


def make_cfg(**over):
    from lavie_amd import text_encoder as T
    return T.config_c(T.config_dict(dict(tc.TINY, **over)))


# ------------------------------------------------------------------ the contract with transformers
@pytest.mark.parametrize("name", list(tc.MODEL_CONFIGS))
def test_state_dict_keys_match_transformers(name):
    from transformers import CLIPTextConfig, CLIPTextModel
    from lavie_amd import text_encoder as T
    cfg = dict(tc.MODEL_CONFIGS[name], vocab_size=64)
    with torch.device("meta"):
        stock = CLIPTextModel(CLIPTextConfig(bos_token_id=0, eos_token_id=2, **cfg))
    sd = T.normalize_keys(stock.state_dict())
    want = T.state_dict_keys(T.config_dict(stock.config))
    assert sorted(sd) == sorted(want)
    L, _ = lib()
    h = ctypes.c_void_p()
    c = T.config_c(T.config_dict(stock.config))
    assert L.lavie_text_create(ctypes.byref(c), ctypes.byref(h)) == 0, last_error()
    try:
        assert L.lavie_text_num_params(h) == len(want)
        name_p, numel = ctypes.c_char_p(), ctypes.c_longlong()
        for i, k in enumerate(want):                     # the engine lists them in the same order, with the module's sizes
            assert L.lavie_text_param_info(h, i, ctypes.byref(name_p), ctypes.byref(numel)) == 0
            assert name_p.value.decode() == k and numel.value == sd[k].numel(), (i, k)
    finally:
        L.lavie_text_destroy(h)


def test_config_mirror_has_the_librarys_size():
    L, _lib = lib()
    assert ctypes.sizeof(_lib.TextConfigC) == L.lavie_text_config_size()
    assert [f[0] for f in _lib.TextConfigC._fields_] == ["struct_size", "vocab_size", "hidden", "intermediate", "layers", "heads",
                                                         "max_positions", "act", "eps"]


def test_classic_and_flat_keys_are_both_taken():
    from lavie_amd import text_encoder as T
    flat = {"embeddings.token_embedding.weight": 1, "embeddings.position_ids": 2}
    classic = {"text_model.embeddings.token_embedding.weight": 1, "text_model.embeddings.position_ids": 2}
    assert T.normalize_keys(flat) == T.normalize_keys(classic) == {"text_model.embeddings.token_embedding.weight": 1}


# ------------------------------------------------------------------ refusals of the C entries (no GPU: every check precedes the first HIP call)
def test_create_refusals_name_the_argument():
    L, _ = lib()
    h = ctypes.c_void_p()
    c = make_cfg()
    c.struct_size -= 4
    assert L.lavie_text_create(ctypes.byref(c), ctypes.byref(h)) != 0 and "struct_size" in last_error()
    assert L.lavie_text_create(None, ctypes.byref(h)) != 0 and "null" in last_error()
    for field, value, word in (("vocab_size", 0, "vocab_size"), ("hidden", 96, "hidden"), ("hidden", 4096, "hidden"),
                               ("intermediate", 200, "intermediate"), ("layers", 0, "layers"), ("heads", 3, "heads"),
                               ("heads", 1, "heads"), ("max_positions", 129, "max_positions"), ("max_positions", 0, "max_positions"),
                               ("act", 2, "act"), ("eps", 0.0, "eps")):
        c = make_cfg()
        setattr(c, field, value)
        assert L.lavie_text_create(ctypes.byref(c), ctypes.byref(h)) != 0, (field, value)
        assert word in last_error(), (field, last_error())


def test_handle_refusals():
    L, _ = lib()
    h = ctypes.c_void_p()
    c = make_cfg()
    assert L.lavie_text_create(ctypes.byref(c), ctypes.byref(h)) == 0
    try:
        buf = (ctypes.c_char * 16)()
        assert L.lavie_text_set_param(h, b"text_model.nope", buf, 8) != 0 and "unknown state-dict key" in last_error()
        assert L.lavie_text_set_param(h, b"text_model.final_layer_norm.bias", buf, 8) != 0 and "expected 128" in last_error()
        assert L.lavie_text_set_param(h, b"text_model.final_layer_norm.bias", None, 128) != 0 and "null data" in last_error()
        assert L.lavie_text_finalize(h, None) != 0 and "was never set" in last_error()
        assert L.lavie_text_encode(h, buf, 1, 77, buf, None) != 0 and "not finalized" in last_error()
        assert L.lavie_text_param_info(h, 999, None, None) != 0 and "out of range" in last_error()
        for b, l, word in ((0, 77, "B=0"), (17, 77, "B=17"), (1, 0, "L=0"), (1, 78, "L=78")):
            assert L.lavie_text_workspace_bytes(h, b, l) == -1 and word in last_error(), (b, l, last_error())
        c_, i_, m = 128, 256, 2 * 77
        assert L.lavie_text_workspace_bytes(h, 2, 77) == 2 * m * c_ * 2 + m * 3 * c_ * 2      # x | h | max(3 C, I) wide, 256-byte pieces
    finally:
        L.lavie_text_destroy(h)
    assert L.lavie_text_encode(None, None, 1, 1, None, None) != 0 and "null handle" in last_error()
    assert L.lavie_text_workspace_bytes(None, 1, 1) == -1 and L.lavie_text_num_params(None) == -1


def test_operator_refusals_launch_nothing():
    """every check of the three launchers precedes the launch: on a machine without a device a refusal is all that can come back"""
    L, _ = lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    base = dict(qkv=p, ld=192, o=p, ldo=64, NB=1, L=16, heads=1, dh=64, scale=0.125, stream=None)
    att = lambda **k: L.lavie_causal_attention_f16(*{**base, **k}.values())
    for kw, word in ((dict(L=129), "L=129"), (dict(L=0), "L=0"), (dict(dh=40), "dh=40"), (dict(NB=0), "NB=0"), (dict(ld=191), "ld=191"),
                     (dict(ld=184), "ld=184"), (dict(ldo=56), "ldo=56"), (dict(qkv=None), "null"), (dict(scale=float("inf")), "scale"),
                     (dict(o=ctypes.c_void_p(p.value + 2)), "aligned")):
        assert att(**kw) != 0 and word in last_error(), (kw, last_error())
    emb = lambda ids=p, tok=p, pos=p, out=p, B=1, L_=4, C=128, V=10: L.lavie_token_embed_f16(ids, tok, pos, out, B, L_, C, V, None)
    for kw, word in ((dict(C=100), "C=100"), (dict(V=0), "V=0"), (dict(B=0), "B=0"), (dict(L_=0), "L=0"), (dict(ids=None), "null")):
        assert emb(**kw) != 0 and word in last_error(), (kw, last_error())
    for args, word in (((p, 0, 0), "n=0"), ((p, 8, 2), "kind=2"), ((None, 8, 0), "null")):
        assert L.lavie_act_f16(*args, None) != 0 and word in last_error(), (args, last_error())


# ------------------------------------------------------------------ refusals of the Python object
def test_python_refusals():
    from lavie_amd import ops, text_encoder as T
    with pytest.raises(ValueError, match="hidden_act"):
        T.config_c(T.config_dict(dict(tc.TINY, hidden_act="gelu_new")))
    with pytest.raises(ValueError, match="hidden_act"):
        T.HipCLIPTextModel({}, dict(tc.TINY, hidden_act="relu"))
    with pytest.raises(ValueError, match="lacks"):
        T.config_dict({"vocab_size": 10})
    enc = T.HipCLIPTextModel.__new__(T.HipCLIPTextModel)          # the argument checks of __call__ precede any device work
    enc._cfg, enc._h = T.config_dict(tc.TINY), None
    ids = torch.zeros(1, 77, dtype=torch.long)
    for kw, word in ((dict(attention_mask=torch.ones(1, 77)), "attention_mask"), (dict(position_ids=torch.arange(77)[None]), "position_ids"),
                     (dict(output_hidden_states=True), "output_hidden_states"), (dict(output_attentions=True), "output_attentions")):
        with pytest.raises(NotImplementedError, match=word):
            enc(ids, **kw)
    with pytest.raises(ValueError, match=r"\[0, 1000\)"):
        enc(torch.full((1, 77), 1000))
    with pytest.raises(ValueError, match=r"\[0, 1000\)"):
        enc(torch.full((1, 77), -1))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        enc(torch.zeros(1, 78, dtype=torch.long))
    with pytest.raises(ValueError, match="act: kind"):
        ops.act(torch.zeros(8, dtype=torch.float16), "relu")


def test_pipeline_switch_needs_an_encoder():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline(unet=object())
    with pytest.raises(ValueError, match="no text_encoder"):
        pipe.enable_engine_text_encoder()
    pipe.disable_engine_text_encoder()                             # nothing wrapped: nothing to do


# ------------------------------------------------------------------ the yardsticks themselves
def test_reference64_is_transformers_in_float64():
    for name in ("tiny", "dh64-gelu"):
        cfg = tc.MODEL_CONFIGS[name]
        sd, ids = tc.synth_state_dict(cfg), tc.model_ids(cfg)
        with torch.no_grad():
            want = tc.stock_model(sd, cfg, torch.float64)(ids)[0]
        got = tc.reference64(sd, cfg, ids)
        assert got.dtype == torch.float64 and (got - want).abs().max() < 1e-11, name


@pytest.mark.parametrize("nb,heads,dh", tc.ATT_SHAPES)
def test_attention_model_meets_its_bound(nb, heads, dh):
    """the fp32 model of the kernel, with fp16 roundings at the counted points, against float64: the bound is reachable"""
    for l, pad, hard in [(l, 0, False) for l in (1, 17, 77, 128)] + [(77, 0, True)]:
        case = tc.attention_case(nb, heads, dh, l, pad, hard)
        ref, scale = case["ref"]()
        oc.assert_elementwise(case["model"](), ref, scale, tc.ATT_C, where=case["where"], label=f"model:causal[{nb},{heads},{dh},{l},{hard}]")


def test_hard_rows_are_hard():
    far, dom, first = tc.hard_rows()
    assert all(64 <= r < tc.HARD_L for r in far) and all(0 < r < tc.HARD_L for r in dom) and first == [0]
    assert not set(far) & set(dom)


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu"])
def test_act_model_meets_its_bound(kind):
    for n in tc.ACT_SIZES:
        x = tc.act_input(n)
        assert x.abs().max() <= 12 and (n < 5 or (x.max() == 12 and x.min() == -12))
        ref, scale = tc.act_ref(x, kind)
        oc.assert_elementwise(tc.act_model(x, kind), ref, scale, tc.ACT_C, label=f"model:act[{kind},{n}]")
