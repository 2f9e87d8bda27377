"""-m gpu: LoRA adapters served merged by the engine (lavie_lora_merge_f16, lavie_unet_lora_*): the merge kernel against fp64,
parity with the fp32 oracle on merged weights, in-place re-derivation equal to a fresh build, exact round trips to the base
model, cached-context / graph consistency, the pipeline's cross_attention_kwargs scale, and the interpolation / VSR variants."""
import numpy as np
import pytest
import torch

import golden_util as G
from gpu_util import TOL_UNET, rel_l2

pytestmark = pytest.mark.gpu

SMALL_KW = dict(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
                down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
# level 0 at C = 320: the row-resident kernels (GroupNorm -> q|k|v, text cross-attention, temporal sub-block, feed-forward) and
# their weight images are built, as in the production model
WIDE_KW = dict(sample_size=8, block_out_channels=(320, 640), cross_attention_dim=768,
               down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))


def build(sd, cls=None, **kw):
    if cls is None:
        from lavie_amd.unet import UNet3DConditionModel as cls
    net = cls(init_weights=False, **kw)
    net.load_state_dict({k: v.to(torch.float16) for k, v in sd.items()})
    return net.to("cuda", torch.float16)


def synth(seed, **cfg):
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    return G.synth16(spec.param_shapes(UNetConfig(**cfg)), seed)


@pytest.fixture(scope="module")
def small():
    sd = synth(11, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))
    return build(sd, **SMALL_KW), sd


@pytest.fixture(scope="module")
def wide():
    sd = synth(12, block_out_channels=(320, 640), cross_attention_dim=768, attn_levels=(True, False))
    return build(sd, **WIDE_KW), sd


def adapter(sd, r, seed, alpha=None):
    """A non-trivial adapter on every target, in the fork's saved spelling (`unet.<module>.lora_A.weight`); |B A| ~ 0.3 |W0|."""
    from lavie_amd import lora
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(sd):
        if not lora.is_target(name):
            continue
        n, k = sd[name].shape
        m = "unet." + name[: -len(".weight")]
        out[m + ".lora_A.weight"] = torch.randn(r, k, generator=g) / k ** 0.5
        out[m + ".lora_B.weight"] = torch.randn(n, r, generator=g) * (0.3 / r ** 0.5)
        if alpha is not None:
            out[m + ".alpha"] = torch.tensor(float(alpha))
    return out


def merged_fp32(sd, ad, scale):
    """fp32 W0 + scale * (alpha / r) B A on every target (the oracle's weights)."""
    from lavie_amd import lora
    t = lora.normalize_lora_state_dict(ad)
    s = lora.target_scales(t)
    out = dict(sd)
    for name, (a, b, _) in t.items():
        out[name] = sd[name].float() + scale * s[name] * (b.double() @ a.double()).float()
    return out


def merged_f16(net, sd, ad, scale):
    """The engine's merged weights, computed by the standalone operator: a state dict for a fresh build."""
    from lavie_amd import lora, ops
    t = lora.normalize_lora_state_dict(ad)
    s = lora.target_scales(t)
    out = {k: v.to(torch.float16) for k, v in sd.items()}
    for name, (a, b, _) in t.items():
        eff = float(np.float32(scale) * np.float32(s[name]))
        out[name] = ops.lora_merge(out[name].cuda(), a.cuda(), b.cuda(), eff).cpu()
    return out


def inputs(seed, b=2, f=4, h=8, w=8, cdim=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 4, f, h, w, generator=g).half().cuda(), torch.randn(b, 77, cdim, generator=g).half().cuda()


def ordered16(t):
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


# ------------------------------------------------------------------ 1. the merge kernel
@pytest.mark.parametrize("shape", [(320, 320), (1280, 768), (640, 2560)])
@pytest.mark.parametrize("r", [1, 16, 64])
def test_merge_kernel_vs_fp64(shape, r):
    from lavie_amd import ops
    n, k = shape
    g = torch.Generator().manual_seed(n * 7 + k + r)
    w0 = (torch.randn(n, k, generator=g) * 0.05).half()
    a = torch.randn(r, k, generator=g)
    b = torch.randn(n, r, generator=g) * 1e-3           # trained lora_B values are small: they must survive in fp32
    scale = 0.7
    ref = (w0.double() + scale * (b.double() @ a.double())).to(torch.float16)
    got = ops.lora_merge(w0.cuda(), a.cuda(), b.cuda(), scale)
    again = ops.lora_merge(w0.cuda(), a.cuda(), b.cuda(), scale)
    assert torch.equal(got, again)
    ulps = (ordered16(got.cpu()) - ordered16(ref)).abs()
    assert int(ulps.max()) <= 1, int(ulps.max())
    assert (ulps == 0).double().mean().item() >= 0.999
    assert not torch.equal(got.cpu(), w0)
    # in place (out = W0) gives the same bits; scale 0 is the base exactly
    w = w0.cuda()
    ops.lora_merge(w, a.cuda(), b.cuda(), scale, out=w)
    assert torch.equal(w, got)
    assert torch.equal(ops.lora_merge(w0.cuda(), a.cuda(), b.cuda(), 0.0).cpu(), w0)


# ------------------------------------------------------------------ 2. parity with the oracle
@pytest.mark.parametrize("which", ["small", "wide"])
def test_lora_unet_vs_oracle_on_merged_weights(which, request):
    from oracle import unet_fp32 as O
    net, sd = request.getfixturevalue(which)
    wide_ = which == "wide"
    cdim = 768 if wide_ else 128
    ocfg = O.UNetConfig(block_out_channels=net.cfg.block_out_channels, cross_attention_dim=cdim, attn_levels=(True, False))
    x, ctx = inputs(3, f=16 if wide_ else 4, cdim=cdim)
    ad = adapter(sd, 16, 5, alpha=8)                   # per-target factor 8 / 16
    try:
        base = net(x, 400, encoder_hidden_states=ctx).sample.clone()
        net.load_lora(ad, scale=1.5)
        got = net(x, 400, encoder_hidden_states=ctx).sample.clone()
        cc = net.cache_context(ctx)                     # and the way the denoise loop runs it (fused text kernel at C = 320)
        got_c = net(x, 400, encoder_hidden_states=cc).sample.clone()
        net.cache_context(None)
    finally:
        net.cache_context(None)
        net.unload_lora()
    with torch.no_grad():
        ref = O.unet_forward(merged_fp32(sd, ad, 1.5), x.float().cpu(), 400, ctx.float().cpu(), ocfg)
        ref_base = O.unet_forward(sd, x.float().cpu(), 400, ctx.float().cpu(), ocfg)
    assert rel_l2(ref, ref_base) > 1e-2
    assert rel_l2(got, base) > 1e-2                      # a no-op adapter fails here
    assert rel_l2(got, ref) < TOL_UNET, rel_l2(got, ref)
    assert rel_l2(got_c, ref) < TOL_UNET, rel_l2(got_c, ref)


# ------------------------------------------------------------------ 3. in-place re-derivation == fresh build
def _counts(net, x, t, cc):
    import bench
    from lavie_amd import _lib
    lib = _lib.load()
    bench.profile_begin(lib, (1 << 11) - 1, 2048)        # every class counted
    y = net(x, t, encoder_hidden_states=cc).sample.clone()
    rows = bench.profile_end(lib)
    return y, [r["launches"] for r in rows]


def test_in_place_rederivation_equals_fresh_build(wide):
    net, sd = wide
    ad = adapter(sd, 16, 7)
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(1, 4, 16, 8, 8, generator=g).half()
    x = torch.cat([lat, lat]).cuda()                     # CFG batch: both halves the same latents (shared prefix on)
    ctx = torch.randn(2, 77, 768, generator=g).half().cuda()
    y_net = build({k: v.float() for k, v in merged_f16(net, sd, ad, 0.75).items()}, **WIDE_KW)
    outs = {}
    try:
        for name, m in (("base", net), ("fresh", y_net), ("lora", net)):
            if name == "lora":
                m.load_lora(ad, scale=0.75)
            m.prepare(2, 16, 8, 8, 77)
            cc = m.cache_context(ctx)
            m.set_cfg_shared_input(True)
            outs[name] = _counts(m, x, 300, cc)
            m.set_cfg_shared_input(False)
            m.cache_context(None)
    finally:
        net.set_cfg_shared_input(False)
        net.cache_context(None)
        net.unload_lora()
    (yb, cb), (yf, cf), (yl, cl) = outs["base"], outs["fresh"], outs["lora"]
    assert torch.equal(yl, yf)
    assert not torch.equal(yl, yb)
    assert cl == cb == cf, (cl, cb, cf)
    assert cl[8] > 0 and cl[9] > 0 and cl[10] > 0, cl    # the fused level-0 sub-blocks ran
    del y_net


# ------------------------------------------------------------------ 4. exact round trips
def test_round_trips_to_the_base_and_rescale(small):
    net, sd = small
    x, ctx = inputs(13)
    ad = adapter(sd, 16, 9)
    try:
        base = net(x, 250, encoder_hidden_states=ctx).sample.clone()
        net.load_lora(ad)
        y1 = net(x, 250, encoder_hidden_states=ctx).sample.clone()
        assert rel_l2(y1, base) > 1e-2
        net.set_lora_scale(0.0)
        assert torch.equal(net(x, 250, encoder_hidden_states=ctx).sample, base)
        net.set_lora_scale(0.5)
        y_half = net(x, 250, encoder_hidden_states=ctx).sample.clone()
        assert not torch.equal(y_half, y1) and not torch.equal(y_half, base)
        net.unload_lora()
        assert torch.equal(net(x, 250, encoder_hidden_states=ctx).sample, base)
        net.load_lora(ad, scale=0.5)                        # loading at a scale == rescaling to it
        assert torch.equal(net(x, 250, encoder_hidden_states=ctx).sample, y_half)
        net.refresh_engine()                                # a rebuild registers the adapter again
        assert torch.equal(net(x, 250, encoder_hidden_states=ctx).sample, y_half)
        net.set_lora_scale(1.0)
        assert torch.equal(net(x, 250, encoder_hidden_states=ctx).sample, y1)
        # the parameters stay the base weights until fuse_lora()
        name = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight"
        assert torch.equal(dict(net.named_parameters())[name].cpu(), sd[name].half())
    finally:
        net.unload_lora()
    assert torch.equal(net(x, 250, encoder_hidden_states=ctx).sample, base)


def test_fuse_lora_writes_the_served_weights(small):
    from lavie_amd.unet import UNet3DConditionModel
    net, sd = small
    x, ctx = inputs(15)
    ad = adapter(sd, 8, 10)
    clone = build(sd, **SMALL_KW)
    clone.load_lora(ad, scale=0.6)
    y = clone(x, 100, encoder_hidden_states=ctx).sample.clone()
    clone.fuse_lora()
    assert clone._lora == {}
    assert torch.equal(clone(x, 100, encoder_hidden_states=ctx).sample, y)
    want = merged_f16(clone, sd, ad, 0.6)
    got = {k: v.cpu() for k, v in clone.state_dict().items()}
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert isinstance(clone, UNet3DConditionModel)
    del clone


# ------------------------------------------------------------------ 5. cached context and graph replay follow the adapter
def test_cached_context_and_graph_follow_adapter_changes(small, wide):
    # small: no fused text kernel, so the cached forward is bit-equal to the plain one
    net, sd = small
    x, ctx = inputs(17)
    ad = adapter(sd, 16, 11)
    plain_ctx = ctx.clone()                                 # another tensor: never served from the cache
    try:
        net.prepare(2, 4, 8, 8, 77)
        cc = net.cache_context(ctx)
        for step, change in enumerate((lambda: net.load_lora(ad), lambda: net.set_lora_scale(0.3),
                                       lambda: net.set_lora_scale(0.0), lambda: net.set_lora_scale(2.0),
                                       lambda: net.unload_lora())):
            change()
            want = net(x, 500, encoder_hidden_states=plain_ctx).sample.clone()       # eager, uncached
            assert torch.equal(net(x, 500, encoder_hidden_states=cc).sample, want), step
            net.enable_graph(True)
            for call in range(3):                                                    # eager, capture, replay
                assert torch.equal(net(x, 500, encoder_hidden_states=cc).sample, want), (step, call)
            net.enable_graph(False)
    finally:
        net.enable_graph(False)
        net.cache_context(None)
        net.unload_lora()
    # wide: the fused text cross-attention reads the per-video images bound from the cached K / V; compared with a fresh build of
    # the merged weights that cached the same context
    net, sd = wide
    x, ctx = inputs(19, f=16, cdim=768)
    ad = adapter(sd, 16, 12)
    fresh = build({k: v.float() for k, v in merged_f16(net, sd, ad, 1.0).items()}, **WIDE_KW)
    try:
        fresh.prepare(2, 16, 8, 8, 77)
        want = fresh(x, 700, encoder_hidden_states=fresh.cache_context(ctx)).sample.clone()
        fresh.cache_context(None)
        net.prepare(2, 16, 8, 8, 77)
        cc = net.cache_context(ctx)
        base = net(x, 700, encoder_hidden_states=cc).sample.clone()
        net.load_lora(ad)
        assert torch.equal(net(x, 700, encoder_hidden_states=cc).sample, want)
        net.enable_graph(True)
        for _ in range(3):
            assert torch.equal(net(x, 700, encoder_hidden_states=cc).sample, want)
        net.unload_lora()
        for _ in range(3):
            assert torch.equal(net(x, 700, encoder_hidden_states=cc).sample, base)
    finally:
        net.enable_graph(False)
        net.cache_context(None)
        net.unload_lora()
    del fresh


# ------------------------------------------------------------------ 6. pipeline
def test_pipeline_cross_attention_kwargs_scale(small):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    net, sd = small
    pipe = VideoGenPipeline(unet=net)
    g = torch.Generator().manual_seed(21)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)

    def call(**kw):
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4,
                    num_inference_steps=3, guidance_scale=7.5, generator=torch.Generator().manual_seed(3),
                    output_type="latent", **kw).video.float().cpu()

    try:
        base = call()
        pipe.load_lora_weights(adapter(sd, 16, 13))
        full = call()
        half = call(cross_attention_kwargs={"scale": 0.5})
        assert net.lora_scale == 1.0
        assert torch.equal(call(), full)
        net.set_lora_scale(0.5)
        assert torch.equal(call(), half)
        assert not torch.equal(half, full) and not torch.equal(half, base)

        def boom(i, t, x):
            raise KeyError("callback")
        with pytest.raises(KeyError):
            call(cross_attention_kwargs={"scale": 0.0}, callback=boom)
        assert net.lora_scale == 0.5                        # restored on the exception too
        pipe.unload_lora_weights()
        assert torch.equal(call(), base)
    finally:
        net.unload_lora()


# ------------------------------------------------------------------ 7. interpolation / VSR variants
def test_interpolation_unet_lora_vs_oracle():
    from lavie_amd.interpolation import UNet3DConditionModel as InterpUNet
    from oracle import unet_fp32 as O
    cfg = dict(in_channels=8, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False),
               sparse_causal_attn1=True, temporal_plain=True, ff_before_temporal=True)
    sd = synth(21, **cfg)
    net = build(sd, cls=InterpUNet, sample_size=8, in_channels=8, block_out_channels=(256, 512), cross_attention_dim=128,
                use_first_frame=True, down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
                up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 8, 4, 8, 8, generator=g).half()
    ctx = torch.randn(2, 77, 128, generator=g).half()
    ad = adapter(sd, 16, 14)
    base = net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample.clone()
    net.load_lora(ad)
    got = net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample
    ref = O.unet_forward(merged_fp32(sd, ad, 1.0), x.float(), 300, ctx.float(), O.UNetConfig(**cfg))
    assert rel_l2(got, base) > 1e-2
    assert rel_l2(got, ref) < TOL_UNET, rel_l2(got, ref)
    net.unload_lora()
    assert torch.equal(net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample, base)


def test_vsr_unet_refuses_lora():
    from lavie_amd.vsr import UNet3DVSRModel
    net = UNet3DVSRModel(init_weights=False, sample_size=8, block_out_channels=(256,), cross_attention_dim=1024,
                         layers_per_block=1, down_block_types=("CrossAttnDownBlock3D",), up_block_types=("CrossAttnUpBlock3D",),
                         only_cross_attention=(True,), num_class_embeds=None, down_temporal_idx=(), mid_temporal=False,
                         up_temporal_idx=())
    with pytest.raises(NotImplementedError):
        net.load_lora({"unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_q.lora_A.weight": torch.zeros(4, 256),
                       "unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_q.lora_B.weight": torch.zeros(256, 4)})
