"""-m gpu: the text encoder on the engine — its three kernels per element on guarded operands, the model against
transformers in float64 with the stock fp16 module as the yardstick of what fp16 storage costs, and the four guarantees."""
import json
import os

import pytest
import torch

import opcheck as oc
import textcases as tc
from test_gpu_engine import small  # noqa: F401  (the `small` UNet fixture, as it is)

pytestmark = pytest.mark.gpu

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "text_encoder.json")


def sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ causal attention
def run_attention(case, ldo_pad=0):
    from lavie_amd import ops
    nb, heads, dh, l, c = case["nb"], case["heads"], case["dh"], case["l"], case["c"]
    mask = torch.zeros(nb * l, c + ldo_pad, dtype=torch.bool)
    mask[:, :c] = True
    out = oc.run_guarded(lambda i, o: ops.causal_attention(i["qkv"], nb, l, heads, dh, out=o["y"]), {"qkv": case["qkv"]},
                         {"y": ((nb * l, c + ldo_pad), torch.float16)}, sync=sync, partial={"y": mask} if ldo_pad else None)
    y = out["y"][:, :c]
    assert torch.isfinite(y).all()
    ref, scale = case["ref"]()
    oc.assert_elementwise(y, ref, scale, tc.ATT_C, where=case["where"], label=f"causal[nb{nb},h{heads},dh{dh},l{l},pad{case['pad']}]")


@pytest.mark.parametrize("nb,heads,dh", tc.ATT_SHAPES)
@pytest.mark.parametrize("l", tc.ATT_LENGTHS)
def test_causal_attention_per_element(nb, heads, dh, l):
    run_attention(tc.attention_case(nb, heads, dh, l))


@pytest.mark.parametrize("nb,heads,dh", tc.ATT_SHAPES)
def test_causal_attention_wider_rows_with_poisoned_padding(nb, heads, dh):
    """ld > 3 heads dh (the padding columns NaN) and ldo > heads dh (the padding columns keep their poison)"""
    run_attention(tc.attention_case(nb, heads, dh, 77, pad=16), ldo_pad=8)


@pytest.mark.parametrize("nb,heads,dh", tc.ATT_SHAPES)
def test_causal_attention_hard_logits(nb, heads, dh):
    run_attention(tc.attention_case(nb, heads, dh, tc.HARD_L, hard=True))


@pytest.mark.parametrize("kw,word", [(dict(l=129), "L=129"), (dict(dh=40), "dh=40"), (dict(nb=0), "NB=0")])
def test_causal_attention_refusals_leave_the_output_alone(kw, word):
    from lavie_amd import ops
    a = dict(nb=1, l=16, heads=2, dh=64)
    a.update(kw)
    rows = max(a["nb"], 1) * a["l"]
    qkv = torch.zeros(rows, 3 * a["heads"] * a["dh"], dtype=torch.float16)
    with pytest.raises(RuntimeError, match=word):
        oc.run_guarded(lambda i, o: ops.causal_attention(i["qkv"], a["nb"], a["l"], a["heads"], a["dh"], out=o["y"]), {"qkv": qkv},
                       {"y": ((rows, a["heads"] * a["dh"]), torch.float16)}, sync=sync)
    y = oc.guarded((rows, a["heads"] * a["dh"]), torch.float16)
    with pytest.raises(RuntimeError, match=word):
        ops.causal_attention(qkv.cuda(), a["nb"], a["l"], a["heads"], a["dh"], out=y.t)
    sync()
    assert y.unwritten().numel() == y.n                                  # the poison is intact


# ------------------------------------------------------------------ embedding gather
@pytest.mark.parametrize("b,l,c,v", [(3, 7, 128, 50), (2, 77, 768, 1000), (1, 1, 8, 1)])
def test_token_embed_is_exact(b, l, c, v):
    """bit-equal to (tok[id].float() + pos[i].float()).half(); ids include 0 and V - 1; 3 x 7 rows of 16 lanes do not fill a workgroup's 16 rows"""
    from lavie_amd import ops
    g = tc.gen("embed", b, l, c, v)
    tok, pos = torch.randn(v, c, generator=g).half(), torch.randn(l + 3, c, generator=g).half()
    ids = torch.randint(0, v, (b, l), generator=g)
    ids.view(-1)[0], ids.view(-1)[-1] = 0, v - 1
    out = oc.run_guarded(lambda i, o: ops.token_embed(ids, i["tok"], i["pos"], out=o["y"]), {"tok": tok, "pos": pos},
                         {"y": ((b * l, c), torch.float16)}, sync=sync)
    want = (tok[ids].float() + pos[:l].float()).half().reshape(b * l, c)
    oc.assert_bits(out["y"], want, where=oc.loc_rows(c), label=f"token_embed[{b},{l},{c},{v}]")


def test_token_embed_validates_ids_on_the_host():
    from lavie_amd import ops
    tok, pos = torch.zeros(10, 8, dtype=torch.float16, device="cuda"), torch.zeros(4, 8, dtype=torch.float16, device="cuda")
    for bad in (torch.tensor([[0, 10]]), torch.tensor([[-1, 3]])):
        with pytest.raises(ValueError, match=r"\[0, 10\)"):
            ops.token_embed(bad, tok, pos)
    with pytest.raises(ValueError, match="position table"):
        ops.token_embed(torch.zeros(1, 5, dtype=torch.long), tok, pos)


# ------------------------------------------------------------------ activation
@pytest.mark.parametrize("kind", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("n", tc.ACT_SIZES)
def test_act_per_element(kind, n):
    from lavie_amd import ops
    x = tc.act_input(n)
    out = oc.run_guarded(lambda i, o: ops.act(i["x"], kind), {"x": x}, {"y": ((n,), torch.float16)}, alias={"y": "x"}, sync=sync)
    ref, scale = tc.act_ref(x, kind)
    oc.assert_elementwise(out["y"], ref, scale, tc.ACT_C, label=f"act[{kind},{n}]")


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def models():
    """name -> (engine encoder, state dict, config), built once"""
    from lavie_amd.text_encoder import HipCLIPTextModel
    built = {}

    def get(name):
        if name not in built:
            cfg = tc.MODEL_CONFIGS[name]
            sd = tc.synth_state_dict(cfg)
            built[name] = (HipCLIPTextModel.from_state_dict(sd, cfg), sd, cfg)
        return built[name]
    return get


def record(name, pair):
    """the measured (engine, stock) error pairs go to profiles/text_encoder.json, beside the timings of tools/bench_text_encoder.py"""
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


@pytest.mark.parametrize("name", list(tc.MODEL_CONFIGS))
def test_model_against_float64_within_twice_the_stock_fp16_error(name, models):
    """Yardstick: transformers in float64 on the CPU with the same fp16-rounded weights.  The engine's rel-L2 and max per-element
    error must not exceed twice those of the stock module in fp16 on the device, measured here against the same result: both keep
    fp16 tensors between operators but round at different points.  Measured on an MI355X (engine / stock, rel-L2 then max):
    see profiles/text_encoder.json."""
    enc, sd, cfg = models(name)
    ids = tc.model_ids(cfg)
    with torch.no_grad():
        ref = tc.stock_model(sd, cfg, torch.float64)(ids)[0]
        stock = tc.stock_model(sd, cfg, torch.float16, "cuda")(ids.cuda())[0]
    out = enc(ids)
    got = out[0]
    assert got is out.last_hidden_state and got.dtype == torch.float16 and got.shape == (tc.MODEL_B, tc.MODEL_L, cfg["hidden_size"])
    assert got.is_cuda and torch.isfinite(got).all()
    e_rel, e_max = tc.errors(got, ref)
    s_rel, s_max = tc.errors(stock, ref)
    print(f"text model {name}: engine rel-L2 {e_rel:.3e} max {e_max:.3e}; stock fp16 rel-L2 {s_rel:.3e} max {s_max:.3e}")
    record(name, {"engine": {"rel_l2": e_rel, "max": e_max}, "stock_fp16": {"rel_l2": s_rel, "max": s_max}})
    assert e_rel <= 2 * s_rel and e_max <= 2 * s_max, (e_rel, s_rel, e_max, s_max)


# ------------------------------------------------------------------ guarantees
def bits(t):
    return t.contiguous().view(torch.int16)


def test_two_calls_agree_bit_for_bit(models):
    enc, _, cfg = models("tiny")
    ids = tc.model_ids(cfg, b=3)
    a, b = enc(ids)[0], enc(ids)[0]
    assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("name,sizes", [("tiny", tuple(range(1, 17))), ("vit-l-1layer", (1, 3, 16))])
def test_a_prompt_has_the_same_bits_in_every_batch(name, sizes, models):
    """every batch size, every position in the batch: the GEMMs are pinned to one tile geometry without split-K"""
    enc, _, cfg = models(name)
    pool = tc.model_ids(cfg, b=16, seed=5)
    single = [bits(enc(pool[i:i + 1])[0][0]) for i in range(16)]
    for n in sizes:
        for shift in (0, 7):                                     # two orders: every prompt meets several positions
            order = [(i + shift) % 16 for i in range(n)]
            got = bits(enc(pool[order])[0])
            for pos, i in enumerate(order):
                assert torch.equal(got[pos], single[i]), (name, n, pos, i)


def test_rows_do_not_depend_on_later_tokens(models):
    enc, _, cfg = models("tiny")
    ids = tc.model_ids(cfg, b=2, seed=9)
    base = bits(enc(ids)[0])
    for i in (0, 15, 16, 40, 75):
        other = ids.clone()
        other[:, i + 1:] = (other[:, i + 1:] + 17) % cfg["vocab_size"]
        got = bits(enc(other)[0])
        assert torch.equal(got[:, :i + 1], base[:, :i + 1]), i
        assert not torch.equal(got[:, i + 1:], base[:, i + 1:]), i


class Tok:                       # stand-in for CLIPTokenizer (its vocabulary files are not in the image), as in test_gpu_engine.py
    model_max_length = 77

    def __call__(self, text, padding=None, max_length=77, truncation=True, return_tensors="pt"):
        from types import SimpleNamespace
        text = [text] if isinstance(text, str) else text
        ids = torch.full((len(text), max_length), 2, dtype=torch.long)
        for i, s in enumerate(text):
            toks = [1 + (sum(map(ord, w)) % 900) for w in s.split()][: max_length - 1]
            ids[i, : len(toks)] = torch.tensor(toks, dtype=torch.long)
        return SimpleNamespace(input_ids=ids)


def test_pipeline_prompt_path_with_engine_text_encoder(small, models):  # noqa: F811
    """test_pipeline_prompt_path_with_stock_text_encoder for the engine's object: `prompt=` gives the latents of passing the
    engine's own embeddings as prompt_embeds, bit for bit; and prompt=[a, b] gives `a` the latents of prompt=a."""
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, _ = small
    enc, _, _ = models("tiny")
    pipe = VideoGenPipeline(unet=net, text_encoder=enc, tokenizer=Tok())
    lat = torch.randn(1, 4, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    kw = dict(height=64, width=64, video_length=4, num_inference_steps=2, guidance_scale=7.5, output_type="latent")
    pa, pb, neg = "a corgi walking in the park", "a teddy bear skating", "blurry"
    a = pipe(prompt=pa, negative_prompt=neg, latents=lat, generator=torch.Generator().manual_seed(3), **kw).video
    pe, ne = enc(Tok()(pa).input_ids)[0], enc(Tok()(neg).input_ids)[0]
    b = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, generator=torch.Generator().manual_seed(3), **kw).video
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # a batch of two prompts: the encoder gives `a` the embeddings of its single call
    both = enc(Tok()([pa, pb]).input_ids)[0]
    assert torch.equal(bits(both[0]), bits(pe[0]))
    two = pipe(prompt=[pa, pb], negative_prompt=[neg, neg], latents=torch.cat([lat, lat]), generator=torch.Generator().manual_seed(3), **kw).video
    ref2 = pipe(prompt_embeds=both, negative_prompt_embeds=torch.cat([ne, ne]), latents=torch.cat([lat, lat]),
                generator=torch.Generator().manual_seed(3), **kw).video
    assert torch.equal(two, ref2)


def test_pipeline_wraps_and_unwraps_a_stock_encoder(small):  # noqa: F811
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.text_encoder import HipCLIPTextModel
    net, _ = small
    cfg = tc.TINY
    stock = tc.stock_model(tc.synth_state_dict(cfg), cfg, torch.float16, "cuda")
    pipe = VideoGenPipeline(unet=net, text_encoder=stock, tokenizer=Tok())
    pipe.enable_engine_text_encoder()
    assert isinstance(pipe.text_encoder, HipCLIPTextModel) and pipe.to("cuda") is pipe
    ids = Tok()("a corgi").input_ids
    got = pipe.text_encoder(ids)[0]
    with torch.no_grad():
        ref = stock(ids.cuda())[0]
    assert (got.float() - ref.float()).norm() / ref.float().norm() < 1e-2
    pipe.disable_engine_text_encoder()
    assert pipe.text_encoder is stock
    p2, _, _ = VideoGenPipeline.from_sample_yaml({"sample_method": "ddim"}, net, text_encoder=HipCLIPTextModel.from_stock(stock), tokenizer=Tok())
    assert isinstance(p2.text_encoder, HipCLIPTextModel)
