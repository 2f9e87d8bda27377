"""-m gpu: several named LoRA adapters blended in one fixed-order merge (lavie_lora_merge_multi_f16, lavie_unet_lora_*_slot*): the
multi-term kernel against fp64 and its three bit-exact properties (one term = the single merge, a dead term is invisible, two runs
agree), the per-element check with poisoned outputs and guard bands, the engine's blend equal to a fresh build of the merged
weights and within tolerance of the fp32 oracle, exact round trips, fuse_lora, the pipeline surface and the refusals."""
import functools

import pytest
import torch

import opcases as C
import opcheck as oc
import test_gpu_lora as L
from gpu_util import TOL_UNET, rel_l2
from test_gpu_ops_local import check

pytestmark = pytest.mark.gpu

SCALES = [0.7, -0.4, 1.3, 0.25, 0.9, -1.1, 0.5, 0.6]
KERNEL_CASES = [((33, 72), (1, 33, 128)),            # row tail, the 64 + 8 column tail, rank-chunk boundaries
                ((320, 320), (4, 16, 40)),           # a level-0 projection
                ((1280, 768), (16,) * 8),            # all eight terms
                ((640, 2560), (64, 128))]            # the widest projection


@pytest.fixture(scope="module")
def small():
    sd = L.synth(11, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    return L.build(sd, **L.SMALL_KW), sd


@pytest.fixture(scope="module")
def wide():
    sd = L.synth(12, block_out_channels=(320, 640), cross_attention_dim=768, attn_levels=(True, False))
    return L.build(sd, **L.WIDE_KW), sd


def kernel_inputs(shape, ranks):
    n, k = shape
    g = torch.Generator().manual_seed(n * 7 + k + sum(ranks))
    w0 = (torch.randn(n, k, generator=g) * 0.05).half()
    terms = [(torch.randn(r, k, generator=g), torch.randn(n, r, generator=g) * 1e-3, SCALES[i]) for i, r in enumerate(ranks)]
    return w0, terms


def on_gpu(terms):
    return [(a.cuda(), b.cuda(), s) for a, b, s in terms]


def same_bits(x, y):
    """torch.equal takes -0.0 for +0.0; this does not."""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16))


# ------------------------------------------------------------------ 1. the multi-term kernel
@pytest.mark.parametrize("shape,ranks", KERNEL_CASES, ids=lambda v: "x".join(map(str, v)))
def test_multi_merge_kernel_vs_fp64(shape, ranks):
    """<= 1 fp16 ulp from fp16(W0 + sum s_i B_i A_i) in fp64, >= 99.9 % exact (an fp32 model of the sum alone gives >= 0.9997),
    in place = out of place, two runs equal."""
    from lavie_amd import ops
    w0, terms = kernel_inputs(shape, ranks)
    ref = w0.double()
    for a, b, s in terms:
        ref = ref + s * (b.double() @ a.double())
    ref = ref.to(torch.float16)
    dev = on_gpu(terms)
    got = ops.lora_merge_multi(w0.cuda(), dev)
    again = ops.lora_merge_multi(w0.cuda(), dev)
    w = w0.cuda()
    ops.lora_merge_multi(w, dev, out=w)                   # in place
    ulps = (L.ordered16(got.cpu()) - L.ordered16(ref)).abs()
    exact = (ulps == 0).double().mean().item()
    print(f"multi merge {shape} ranks {ranks}: max {int(ulps.max())} ulp, exact share {exact:.6f}")
    assert same_bits(got, again)
    assert same_bits(w, got)
    assert int(ulps.max()) <= 1, int(ulps.max())
    assert exact >= 0.999, exact
    assert not torch.equal(got.cpu(), w0)


@pytest.mark.parametrize("r", [1, 32, 33, 128])
def test_one_term_gives_the_bits_of_the_single_merge(r):
    """By construction (one live term is handed to the single kernel), so for any compiler; zero-scale terms around it included."""
    from lavie_amd import ops
    for shape in ((33, 72), (320, 768)):
        w0, terms = kernel_inputs(shape, (r,))
        (a, b, s), = on_gpu(terms)
        want = ops.lora_merge(w0.cuda(), a, b, s)
        assert same_bits(ops.lora_merge_multi(w0.cuda(), [(a, b, s)]), want)
        assert same_bits(ops.lora_merge_multi(w0.cuda(), [(a, b, 0.0), (a, b, s), (a, b, -0.0)]), want)
        w = w0.cuda()
        ops.lora_merge_multi(w, [(a, b, s)], out=w)
        assert same_bits(w, want)
    # W0 = -0.0 with a term that adds nothing there and a negative factor: the single kernel keeps -0.0
    w0 = torch.full((8, 16), -0.0).half()
    a0, b0 = torch.zeros(r, 16).cuda(), torch.randn(8, r).cuda()
    assert same_bits(ops.lora_merge_multi(w0.cuda(), [(a0, b0, -0.4)]), ops.lora_merge(w0.cuda(), a0, b0, -0.4))


@pytest.mark.parametrize("shape", [(33, 72), (320, 768)])
def test_a_dead_term_changes_no_bit(shape):
    """Among two or more live terms a term with A = 0 or with scale 0 changes no bit, wherever it stands; zero-scale terms change
    none next to one live term either (they are dropped: the single merge) and alone give W0.  A term with A = 0 and a non-zero
    scale next to exactly ONE live term makes a two-term sum, rounded fp32 -> fp16, while the single merge's own last step may be
    fused by the compiler (one rounding): at most 1 ulp apart and only at double-rounding ties, >= 99.9 % exact."""
    from lavie_amd import ops
    w0, terms = kernel_inputs(shape, (5, 33))
    dev = on_gpu(terms)
    want = ops.lora_merge_multi(w0.cuda(), dev)
    assert not torch.equal(want.cpu(), w0)
    a2, b2, _ = on_gpu(kernel_inputs(shape, (40,))[1])[0]
    zero_a = (torch.zeros_like(a2), b2, 1.3)
    zero_b = (a2, torch.zeros_like(b2), -1.1)
    zero_s = (a2, b2, 0.0)
    for where in range(3):                                # in front, between, behind
        for dead in (zero_a, zero_b, zero_s):
            ts = dev[:where] + [dead] + dev[where:]
            assert same_bits(ops.lora_merge_multi(w0.cuda(), ts), want), where
    assert same_bits(ops.lora_merge_multi(w0.cuda(), dev + [zero_a, zero_s, zero_s]), want)
    single = ops.lora_merge(w0.cuda(), dev[1][0], dev[1][1], dev[1][2])
    assert same_bits(ops.lora_merge_multi(w0.cuda(), [dev[1], zero_s]), single)
    ulps = (L.ordered16(ops.lora_merge_multi(w0.cuda(), [dev[1], zero_a]).cpu()) - L.ordered16(single.cpu())).abs()
    assert int(ulps.max()) <= 1 and (ulps == 0).double().mean().item() >= 0.999
    # zero-scale terms only: the base, out of place and in place
    assert same_bits(ops.lora_merge_multi(w0.cuda(), [zero_s, (dev[0][0], dev[0][1], 0.0)]).cpu(), w0)
    w = w0.cuda()
    ops.lora_merge_multi(w, [zero_s], out=w)
    assert same_bits(w.cpu(), w0)
    # a live term's -0.0 factor is a zero factor too
    assert same_bits(ops.lora_merge_multi(w0.cuda(), [(a2, b2, -0.0)]).cpu(), w0)


# ------------------------------------------------------------------ 2. per element, poisoned outputs, guard bands
@functools.lru_cache(maxsize=None)
def multi_case(N, K, ranks, in_place):
    """Bound: the GEMM family's with K_terms = sum r_i + T + 1 (r_i fmas per term, one fma per term into the running sum, the fp32
    conversion of W0) on the sum of the absolute terms; one fp16 rounding (U16 |ref|)."""
    g = C.gen("lora_multi", N, K, ranks)
    w0 = C.rnd(g, N, K)
    ab = [(C.rnd(g, r, K, dtype=C.f32t), C.rnd(g, N, r, dtype=C.f32t, s=0.1)) for r in ranks]
    scales = SCALES[:len(ranks)]
    ins = {"w0": w0}
    for t, (a, b) in enumerate(ab):
        ins[f"a{t}"], ins[f"b{t}"] = a, b

    def run(ops, i, o):
        ops.lora_merge_multi(i["w0"], [(i[f"a{t}"], i[f"b{t}"], scales[t]) for t in range(len(ranks))], out=o["y"])

    def terms(cv, p, ps):
        y = p(cv(w0))
        for (a, b), s in zip(ab, scales):
            y = y + ps(s) * (p(cv(b)) @ p(cv(a)))
        return y

    ident, ab_ = (lambda t: t), (lambda t: t.abs())
    return C.Case(f"lora_merge_multi[{N}x{K},r{ranks},inplace{int(in_place)}]", ins, {"y": ((N, K), C.f16)}, run,
                  lambda: {"y": (terms(C.d, ident, ident), terms(C.d, ab_, abs))}, oc.gemm_c(sum(ranks) + len(ranks) + 1),
                  lambda: {"y": terms(lambda t: t.float(), ident, ident).half()}, oc.loc_rows(K),
                  alias={"y": "w0"} if in_place else None)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("N,K,ranks", [(3, 24, (2, 1)), (33, 72, (1, 33, 128))])
def test_multi_merge_per_element(N, K, ranks, in_place):
    from lavie_amd import ops
    case = multi_case(N, K, ranks, in_place)
    case.check(case.model(), label="model ")              # the fp32 model of the kernel meets the bound it is held to
    check(ops, case)


# ------------------------------------------------------------------ 3. the engine's blend
def partial(ad):
    """The adapter on the attn2 and attn_temp targets only."""
    return {k: v for k, v in ad.items() if ".attn2." in k or ".attn_temp." in k}


def norm(ad):
    from lavie_amd import lora
    t = lora.normalize_lora_state_dict(ad)
    return t, lora.target_scales(t)


def blend_f16(sd, blend, gscale):
    """The engine's merged weights by the standalone operator: blend = [(adapter state dict, weight)] in slot order; the factor
    of a term is the engine's fp32 product.  A state dict for a fresh build."""
    from lavie_amd import lora, ops
    out = {k: v.to(torch.float16) for k, v in sd.items()}
    parts = [(norm(ad), w) for ad, w in blend]
    for name in sd:
        terms = [(t[name][0].cuda(), t[name][1].cuda(), lora.blend_factor(gscale, w, s[name])) for (t, s), w in parts if name in t]
        if terms:
            out[name] = ops.lora_merge_multi(out[name].cuda(), terms).cpu()
    return out


def blend_fp32(sd, blend, gscale):
    """fp32 W0 + sum gscale * weight * (alpha / r) B A (the oracle's weights)."""
    out = dict(sd)
    for ad, w in blend:
        t, s = norm(ad)
        for name, (a, b, _) in t.items():
            out[name] = out[name].float() + gscale * w * s[name] * (b.double() @ a.double()).float()
    return out


def fresh_forward(sd, blend, gscale, kw, x, t, ctx, cached=False):
    net = L.build({k: v.float() for k, v in blend_f16(sd, blend, gscale).items()}, **kw)
    try:
        if cached:
            net.prepare(x.shape[0], x.shape[2], x.shape[3], x.shape[4], ctx.shape[1])
            return L._counts(net, x, t, net.cache_context(ctx))
        return L._counts(net, x, t, ctx)
    finally:
        del net


@pytest.mark.parametrize("which", ["small", "wide"])
def test_blend_equals_fresh_build_and_matches_the_oracle(which, request):
    from oracle import unet_fp32 as O
    net, sd = request.getfixturevalue(which)
    wide_ = which == "wide"
    cdim = 768 if wide_ else 128
    kw = L.WIDE_KW if wide_ else L.SMALL_KW
    x, ctx = L.inputs(31, cdim=cdim)
    ad_a, ad_b = L.adapter(sd, 16, 41, alpha=8), partial(L.adapter(sd, 8, 42))
    assert 0 < len(ad_b) < len(ad_a)
    blend, gscale = [(ad_a, 0.8), (ad_b, -0.5)], 1.5
    try:
        if wide_:                                            # cached context: the text K / V images are re-derived by the apply
            net.prepare(2, 4, 8, 8, 77)
            cc = net.cache_context(ctx)
        else:
            cc = ctx
        base, n_base = L._counts(net, x, 400, cc)
        net.load_lora(ad_a, adapter_name="a")
        net.load_lora(ad_b, adapter_name="b")
        net.set_adapters(["a", "b"], [0.8, -0.5])
        net.set_lora_scale(gscale)
        got, n_got = L._counts(net, x, 400, cc)
    finally:
        net.cache_context(None)
        net.unload_lora()
    want, n_want = fresh_forward(sd, blend, gscale, kw, x, 400, ctx, cached=wide_)
    assert torch.equal(got, want)
    assert n_got == n_base == n_want, (n_got, n_base, n_want)
    ocfg = O.UNetConfig(block_out_channels=net.cfg.block_out_channels, cross_attention_dim=cdim, attn_levels=(True, False))
    with torch.no_grad():
        ref = O.unet_forward(blend_fp32(sd, blend, gscale), x.float().cpu(), 400, ctx.float().cpu(), ocfg)
    assert rel_l2(got, base) > 1e-2                          # a no-op blend fails here
    assert rel_l2(got, ref) < TOL_UNET, rel_l2(got, ref)


# ------------------------------------------------------------------ 4. exact round trips
def test_round_trips_bit_for_bit(small):
    net, sd = small
    x, ctx = L.inputs(33)
    ad_a, ad_b = L.adapter(sd, 16, 43), partial(L.adapter(sd, 8, 44))
    fwd = lambda: net(x, 250, encoder_hidden_states=ctx).sample.clone()       # noqa: E731
    try:
        base = fwd()
        net.load_lora(ad_a, adapter_name="a")
        only_a = fwd()
        net.load_lora(ad_b, adapter_name="b")
        both = fwd()
        assert not torch.equal(both, only_a) and not torch.equal(only_a, base)
        net.set_adapters(["a"])                              # b resident, contributes nothing
        assert net.get_list_adapters() == ["a", "b"] and net.get_active_adapters() == ["a"]
        assert torch.equal(fwd(), only_a)
        net.set_adapters(["a", "b"])
        assert torch.equal(fwd(), both)
        net.set_adapters(["a", "b"], [0.0, 0.0])
        assert torch.equal(fwd(), base)
        net.set_adapters(["a", "b"])
        net.set_adapters([])
        assert torch.equal(fwd(), base)
        net.set_adapters(["b", "a"])                         # the order of the names does not matter: slots do
        assert torch.equal(fwd(), both)
        net.refresh_engine()                                 # a rebuild registers every adapter again, slot and weight
        assert torch.equal(fwd(), both)
        net.delete_adapters(["a", "b"])
        assert net.get_list_adapters() == [] and net._lora == {}
        assert torch.equal(fwd(), base)
        net.load_lora(ad_a, adapter_name="a")
        net.load_lora(ad_b, adapter_name="b")
        assert torch.equal(fwd(), both)
        net.delete_adapters("a")
        net.load_lora(ad_a, adapter_name="a")                # back in the slot it left
        assert torch.equal(fwd(), both)
        net.unload_lora()
        assert torch.equal(fwd(), base)
        net.load_lora(ad_a)                                  # no name: one adapter, as ever
        assert net.get_list_adapters() == ["default"]
        assert torch.equal(fwd(), only_a)
    finally:
        net.unload_lora()
    assert torch.equal(fwd(), base)


def test_each_of_five_changes_equals_its_fresh_build(small):
    net, sd = small
    x, ctx = L.inputs(35)
    ad_a, ad_b, ad_c = L.adapter(sd, 16, 45), partial(L.adapter(sd, 8, 46)), L.adapter(sd, 4, 47, alpha=2)
    ad_b2 = partial(L.adapter(sd, 12, 48))
    steps = [
        (lambda: (net.load_lora(ad_a, adapter_name="a"), net.load_lora(ad_b, adapter_name="b"),
                  net.set_adapters(["a", "b"], [0.8, -0.5])), [(ad_a, 0.8), (ad_b, -0.5)], 1.0),
        (lambda: net.set_lora_scale(0.5), [(ad_a, 0.8), (ad_b, -0.5)], 0.5),
        (lambda: net.load_lora(ad_c, scale=1.25, adapter_name="c"), [(ad_a, 0.8), (ad_b, -0.5), (ad_c, 1.25)], 0.5),
        (lambda: net.delete_adapters("a"), [(ad_b, -0.5), (ad_c, 1.25)], 0.5),
        (lambda: net.load_lora(ad_b2, scale=0.3, adapter_name="b"), [(ad_b2, 0.3), (ad_c, 1.25)], 0.5),     # another rank in b's slot
    ]
    seen = []
    try:
        for i, (change, blend, gscale) in enumerate(steps):
            change()
            got = net(x, 250, encoder_hidden_states=ctx).sample.clone()
            want, _ = fresh_forward(sd, blend, gscale, L.SMALL_KW, x, 250, ctx)
            assert torch.equal(got, want), i
            assert all(not torch.equal(got, y) for y in seen), i
            seen.append(got)
    finally:
        net.unload_lora()


def test_graph_and_cached_context_follow_a_reweight(small):
    net, sd = small
    x, ctx = L.inputs(37)
    plain_ctx = ctx.clone()                                  # another tensor: never served from the cache
    try:
        net.prepare(2, 4, 8, 8, 77)
        cc = net.cache_context(ctx)
        net.load_lora(L.adapter(sd, 16, 49), adapter_name="a")
        net.load_lora(partial(L.adapter(sd, 8, 50)), adapter_name="b")
        changes = (lambda: None, lambda: net.set_adapters(["a", "b"], [0.8, -0.5]), lambda: net.set_adapters(["b"], [2.0]),
                   lambda: net.set_adapters(["a", "b"]))
        wants = []
        for change in changes:                               # eager, uncached: what each state must give
            change()
            wants.append(net(x, 500, encoder_hidden_states=plain_ctx).sample.clone())
        assert torch.equal(wants[0], wants[3]) and not torch.equal(wants[0], wants[1]) and not torch.equal(wants[1], wants[2])
        net.enable_graph(True)                               # the same walk from the same state: one capture, then replays
        for step, change in enumerate(changes):
            change()
            for call in range(3):
                assert torch.equal(net(x, 500, encoder_hidden_states=cc).sample, wants[step]), (step, call)
    finally:
        net.enable_graph(False)
        net.cache_context(None)
        net.unload_lora()


# ------------------------------------------------------------------ 5. fuse_lora
def test_fuse_lora_writes_the_served_blend(small):
    _, sd = small
    x, ctx = L.inputs(39)
    ad_a, ad_b = L.adapter(sd, 8, 51), partial(L.adapter(sd, 4, 52, alpha=2))
    clone = L.build(sd, **L.SMALL_KW)
    clone.load_lora(ad_a, adapter_name="a")
    clone.load_lora(ad_b, adapter_name="b")
    clone.load_lora(L.adapter(sd, 4, 53), adapter_name="off")
    clone.set_adapters(["a", "b"], [0.8, -0.5])              # "off" stays resident, contributes nothing
    clone.set_lora_scale(0.6)
    y = clone(x, 100, encoder_hidden_states=ctx).sample.clone()
    clone.fuse_lora()
    assert clone._lora == {} and clone.get_list_adapters() == [] and clone.lora_scale == 1.0
    assert torch.equal(clone(x, 100, encoder_hidden_states=ctx).sample, y)
    want = blend_f16(sd, [(ad_a, 0.8), (ad_b, -0.5)], 0.6)
    got = {k: v.cpu() for k, v in clone.state_dict().items()}
    assert all(torch.equal(got[k], want[k]) for k in want)
    del clone


# ------------------------------------------------------------------ 6. pipeline
def test_pipeline_adapters_reach_the_unet(small):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, sd = small
    pipe = VideoGenPipeline(unet=net)
    g = torch.Generator().manual_seed(21)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    ad_a, ad_b = L.adapter(sd, 16, 54), partial(L.adapter(sd, 8, 55))

    def call(**kw):
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4,
                    num_inference_steps=3, guidance_scale=7.5, generator=torch.Generator().manual_seed(3),
                    output_type="latent", **kw).video.float().cpu()

    try:
        base = call()
        net.load_lora(ad_a, adapter_name="a")                 # the blend set on the UNet directly ...
        net.load_lora(ad_b, adapter_name="b")
        net.set_adapters(["a", "b"], [0.8, -0.5])
        want = call()
        net.unload_lora()
        pipe.load_lora_weights(ad_a, adapter_name="a")        # ... and through the pipeline
        pipe.load_lora_weights(ad_b, adapter_name="b")
        pipe.set_adapters(["a", "b"], [0.8, -0.5])
        assert pipe.get_list_adapters() == {"unet": ["a", "b"]} and pipe.get_active_adapters() == ["a", "b"]
        assert net._lora_slots() == [("a", 0, 0.8), ("b", 1, -0.5)]
        full = call()
        assert torch.equal(full, want) and not torch.equal(full, base)
        half = call(cross_attention_kwargs={"scale": 0.5})    # scales the whole blend for one call
        assert net.lora_scale == 1.0 and torch.equal(call(), full)
        net.set_lora_scale(0.5)
        assert torch.equal(call(), half) and not torch.equal(half, full) and not torch.equal(half, base)

        def boom(i, t, x):
            raise KeyError("callback")
        with pytest.raises(KeyError):
            call(cross_attention_kwargs={"scale": 0.0}, callback=boom)
        assert net.lora_scale == 0.5                          # restored on the exception too
        assert torch.equal(call(), half)
        pipe.delete_adapters("b")
        assert pipe.get_list_adapters() == {"unet": ["a"]}
        pipe.unload_lora_weights()                            # removes all
        assert net.get_list_adapters() == [] and torch.equal(call(), base)
    finally:
        net.unload_lora()


# ------------------------------------------------------------------ 7. refusals leave the served weights alone
def test_refusals_with_a_built_engine(small):
    from lavie_amd.vsr import UNet3DVSRModel
    net, sd = small
    x, ctx = L.inputs(41)
    one = {k: v for k, v in L.adapter(sd, 2, 56).items() if "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q." in k}
    assert len(one) == 2
    fwd = lambda: net(x, 250, encoder_hidden_states=ctx).sample.clone()       # noqa: E731
    try:
        for i in range(8):
            net.load_lora(one, scale=0.5 + i, adapter_name=f"n{i}")
        y = fwd()
        with pytest.raises(ValueError, match="8 adapters"):
            net.load_lora(one, adapter_name="ninth")
        with pytest.raises(ValueError, match="nope"):
            net.set_adapters(["n0", "nope"])
        with pytest.raises(ValueError, match="nope"):
            net.delete_adapters("nope")
        with pytest.raises(ValueError, match="not finite"):
            net.set_adapters(["n0", "n1"], [1.0, float("nan")])
        assert len(net.get_list_adapters()) == len(net.get_active_adapters()) == 8
        assert torch.equal(fwd(), y)
        # all eight slots on one target: the eight-term merge, equal to its fresh build
        want, _ = fresh_forward(sd, [(one, 0.5 + i) for i in range(8)], 1.0, L.SMALL_KW, x, 250, ctx)
        assert torch.equal(y, want)
    finally:
        net.unload_lora()
    vsr = UNet3DVSRModel(init_weights=False, sample_size=8, block_out_channels=(256,), cross_attention_dim=1024,
                         layers_per_block=1, down_block_types=("CrossAttnDownBlock3D",), up_block_types=("CrossAttnUpBlock3D",),
                         only_cross_attention=(True,), num_class_embeds=None, down_temporal_idx=(), mid_temporal=False,
                         up_temporal_idx=())
    with pytest.raises(NotImplementedError):
        vsr.load_lora({"unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_q.lora_A.weight": torch.zeros(4, 256),
                       "unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_q.lora_B.weight": torch.zeros(256, 4)},
                      adapter_name="a")
