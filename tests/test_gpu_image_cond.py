"""-m gpu: image-conditioned sampling (a 77-token text context widened by 77 mapped image tokens): the long variant of the fused
level-0 text cross-attention (81..160 keys) against an fp32 restatement, the production UNet at a 154-token context against the
oracle (eager, cached context, shared CFG prefix), LoRA re-derivation of the long images, and the guided pipeline with a mapper
against the oracle loop."""
import math

import pytest
import torch
import torch.nn.functional as F

import golden_util as G
from gpu_util import TOL_OP, TOL_UNET, f32, h16, q16, rel_l2

pytestmark = pytest.mark.gpu

SMALL_KW = dict(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
                down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
WIDE_KW = dict(sample_size=8, block_out_channels=(320, 640), cross_attention_dim=768,
               down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
KC_FUSED_CROSS = 10


def build(sd, **kw):
    from lavie_amd.unet import UNet3DConditionModel
    net = UNet3DConditionModel(init_weights=False, **kw)
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
def full():
    from lavie_amd import spec
    sd = G.synth16(spec.param_shapes(), 0)
    return build(sd, sample_size=64, cross_attention_dim=768), sd


def counted(net, x, t, ctx, mask=(1 << 11) - 1, events=2048):
    """One forward with the kernel classes of `mask` counted -> (output, launches per class)."""
    import bench
    from lavie_amd import _lib
    lib = _lib.load()
    bench.profile_begin(lib, mask, events)
    y = net(x, t, encoder_hidden_states=ctx).sample.clone()
    rows = bench.profile_end(lib)
    return y, [r["launches"] for r in rows]


# ------------------------------------------------------------------ 1. the long kernel
# (videos, rows per video, keys): one pass; two videos with ragged passes (163 tiles per video on 256 workgroups); the production
# level-0 shape (40960 rows per video) at 154 keys; the first and last lengths of the variant
@pytest.mark.parametrize("B,P,L", [(1, 128, 81), (2, 2608, 128), (2, 40960, 154), (2, 512, 160), (3, 48, 100)])
def test_cross_block_long_fused(B, P, L):
    """The sub-block of attention.py:513-534 (attn1.to_out + residual, norm2, attn2 over the cached text K / V, to_out + residual)
    at 81..160 keys, against an fp32 restatement."""
    from lavie_amd import ops
    C, heads = 320, 8
    dh = C // heads
    M = B * P
    g = torch.Generator().manual_seed(B * 100000 + P * 10 + L)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = q16(rnd(M, C) * 1.5 + 0.3 * rnd(1, C))
    att = q16(rnd(M, C))
    wo1, wq2, wo2 = [q16(rnd(C, C) / math.sqrt(C)) for _ in range(3)]
    bo1, bo2 = rnd(C) * 0.2, rnd(C) * 0.2
    gamma, beta = 1.0 + 0.2 * rnd(C), 0.1 * rnd(C)
    kv = q16(rnd(B * L, 2 * C) * torch.cat([torch.full((C,), 1.5), torch.ones(C)]))
    scale = dh ** -0.5
    x1 = x + att @ wo1.t() + bo1
    q = (F.layer_norm(x1, (C,), gamma, beta, 1e-5) @ wq2.t()).reshape(B, P, heads, dh).permute(0, 2, 1, 3)
    k = kv[:, :C].reshape(B, L, heads, dh).permute(0, 2, 1, 3)
    v = kv[:, C:].reshape(B, L, heads, dh).permute(0, 2, 1, 3)
    o = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v
    ref = x1 + o.permute(0, 2, 1, 3).reshape(M, C) @ wo2.t() + bo2
    tmpl = ops.pack_cross_block_long(h16(wo1), h16(wq2), h16(wo2))
    img = ops.bind_cross_block_long(tmpl, h16(kv), B, L)
    xd, ad = h16(x), h16(att)
    args = (img, f32(bo1), f32(gamma), f32(beta), f32(bo2), P, L, heads, scale)
    got = ops.cross_block_long(ad, xd, *args)
    assert rel_l2(got, ref) < TOL_OP
    assert rel_l2(got.float().cpu() - x, ref - x) < 4e-3          # the residual must not hide an error in the products
    assert torch.equal(got, ops.cross_block_long(ad, xd, *args))   # bit-reproducible
    ops.cross_block_long(ad, xd, *args, out=xd)                    # in place, as the engine runs it
    assert torch.equal(xd, got)


def test_cross_block_long_refuses_other_lengths():
    from lavie_amd import ops
    z = torch.zeros(320, 320, dtype=torch.float16, device="cuda")
    tmpl = ops.pack_cross_block_long(z, z, z)
    assert tmpl.numel() * 2 == 840 * 1024
    for L in (161, 80):                                            # above the variant; and the short kernel's range
        with pytest.raises(RuntimeError):
            ops.bind_cross_block_long(tmpl, torch.zeros(L, 640, dtype=torch.float16, device="cuda"), 1, L)
    x = torch.zeros(128, 320, dtype=torch.float16, device="cuda")
    v = torch.zeros(320, dtype=torch.float32, device="cuda")
    img = torch.zeros(tmpl.numel(), dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.cross_block_long(x, x, img, v, v, v, v, 128, 161, 8, 0.1)


# ------------------------------------------------------------------ 2. the production UNet at a 154-token context
def test_full_size_forward_154_tokens_vs_oracle(full):
    """909 M parameters, CFG batch 2, F = 16, latent 40x64, each half's context = 77 text + 77 image tokens: eager (unfused text
    cross-attention at every level), with the context cached (the five level-0 blocks take the long fused kernel: counted, so a
    silent fallback fails) and with the shared CFG prefix, against oracle.unet_fp32.unet_forward per CFG half."""
    import bench
    from oracle import unet_fp32 as O
    net, sd = full
    pe, ne, lat = bench.synth_inputs(0, "cpu")
    g = torch.Generator().manual_seed(77)
    img_tok = torch.randn(2, 77, 768, generator=g)
    ctx = torch.cat([torch.cat([ne, img_tok[:1]], 1), torch.cat([pe, img_tok[1:]], 1)]).half()
    assert ctx.shape == (2, 154, 768)
    x = torch.cat([lat, lat]).half()
    torch.set_num_threads(bench.host_cores())
    t = 500
    with torch.no_grad():
        ref = O.unet_forward(sd, x.float(), t, ctx.float())
    got, n_eager = counted(net, x.cuda(), t, ctx.cuda(), 1 << KC_FUSED_CROSS, 64)
    assert n_eager[KC_FUSED_CROSS] == 0
    assert rel_l2(got[0], ref[0]) < TOL_UNET and rel_l2(got[1], ref[1]) < TOL_UNET
    try:
        cc = net.cache_context(ctx.cuda())
        got_c, n_cached = counted(net, x.cuda(), t, cc, 1 << KC_FUSED_CROSS, 64)
        assert n_cached[KC_FUSED_CROSS] == 5, n_cached                 # down 0 (x2), up 3 (x3)
        assert rel_l2(got_c[0], ref[0]) < TOL_UNET and rel_l2(got_c[1], ref[1]) < TOL_UNET
        net.set_cfg_shared_input(True)
        got_s, n_shared = counted(net, x.cuda(), t, cc, 1 << KC_FUSED_CROSS, 64)
        assert n_shared[KC_FUSED_CROSS] == 5, n_shared
        assert rel_l2(got_s[0], ref[0]) < TOL_UNET and rel_l2(got_s[1], ref[1]) < TOL_UNET
    finally:
        net.set_cfg_shared_input(False)
        net.cache_context(None)
    # back to a 77-token context on the same engine: the short kernel again, unchanged
    try:
        cc = net.cache_context(torch.cat([ne, pe]).half().cuda())
        _, n77 = counted(net, x.cuda(), t, cc, 1 << KC_FUSED_CROSS, 64)
        assert n77[KC_FUSED_CROSS] == 5
    finally:
        net.cache_context(None)


# ------------------------------------------------------------------ 3. LoRA with a cached long context
@pytest.fixture(scope="module")
def wide():
    sd = synth(12, block_out_channels=(320, 640), cross_attention_dim=768, attn_levels=(True, False))
    return build(sd, **WIDE_KW), sd


def test_lora_apply_with_cached_154_token_context_equals_fresh_build(wide):
    """lavie_unet_lora_apply re-derives the long templates and re-binds the cached context's images in place: the forward that
    follows equals a fresh build of the merged weights that cached the same context, bit for bit."""
    import numpy as np
    from lavie_amd import lora, ops
    net, sd = wide
    g = torch.Generator().manual_seed(41)
    ad = {}
    for name in sorted(sd):
        if lora.is_target(name):
            n, k = sd[name].shape
            m = "unet." + name[: -len(".weight")]
            ad[m + ".lora_A.weight"] = torch.randn(16, k, generator=g) / k ** 0.5
            ad[m + ".lora_B.weight"] = torch.randn(n, 16, generator=g) * (0.3 / 4.0)
    t = lora.normalize_lora_state_dict(ad)
    s = lora.target_scales(t)
    merged = {k: v.to(torch.float16) for k, v in sd.items()}
    for name, (a, b, _) in t.items():
        merged[name] = ops.lora_merge(merged[name].cuda(), a.cuda(), b.cuda(), float(np.float32(s[name]))).cpu()
    lat = torch.randn(1, 4, 16, 8, 8, generator=g).half()
    x = torch.cat([lat, lat]).cuda()
    ctx = torch.randn(2, 154, 768, generator=g).half().cuda()
    fresh = build({k: v.float() for k, v in merged.items()}, **WIDE_KW)
    try:
        fresh.prepare(2, 16, 8, 8, 154)
        want, n_fresh = counted(fresh, x, 600, fresh.cache_context(ctx))
        fresh.cache_context(None)
        net.prepare(2, 16, 8, 8, 154)
        cc = net.cache_context(ctx)
        base, _ = counted(net, x, 600, cc)
        net.load_lora(ad)
        got, n_lora = counted(net, x, 600, cc)
        assert torch.equal(got, want)
        assert not torch.equal(got, base)
        assert n_lora == n_fresh and n_lora[KC_FUSED_CROSS] == 5, n_lora      # down 0 (x2), up 1 (x3)
    finally:
        net.cache_context(None)
        net.unload_lora()
    del fresh


def test_one_engine_serves_77_154_77_tokens_like_fresh_engines(wide):
    """One engine handle serving context lengths 77 -> 154 -> 77 in turn, each turn cache_context then one forward: the short
    images, the long templates built by the first long context, then the short layout in the front of the larger images.  Every
    output equals, bit for bit, that of a fresh engine that only ever saw that length, and the fused text kernel ran each time."""
    _, sd = wide
    g = torch.Generator().manual_seed(53)
    lat = torch.randn(1, 4, 16, 8, 8, generator=g).half()
    x = torch.cat([lat, lat]).cuda()
    ctxs = {L: torch.randn(2, L, 768, generator=g).half().cuda() for L in (77, 154)}

    def turn(net, L):
        net.prepare(2, 16, 8, 8, L)
        try:
            y, n = counted(net, x, 600, net.cache_context(ctxs[L]), 1 << KC_FUSED_CROSS, 64)
        finally:
            net.cache_context(None)
        assert n[KC_FUSED_CROSS] == 5, n          # down 0 (x2), up 1 (x3): no silent GEMM route
        return y

    want = {}
    for L in (77, 154):
        fresh = build(sd, **WIDE_KW)
        want[L] = turn(fresh, L)
        del fresh
    net = build(sd, **WIDE_KW)
    for L in (77, 154, 77):
        assert torch.equal(turn(net, L), want[L]), L


# ------------------------------------------------------------------ 4. the guided pipeline with a mapper
def test_guided_pipeline_with_mapper_vs_oracle_loop(small):
    """Three guided DDPM steps on the small model with a small random mapper and precomputed image features: the context the
    pipeline builds ([negative + mapped | prompt + mapped], 154 tokens) driven through oracle.ddpm.cfg_denoise_loop."""
    from lavie_amd.mapping import MappingNetwork
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from oracle import unet_fp32 as O
    from oracle.ddpm import cfg_denoise_loop
    net, sd = small
    torch.manual_seed(3)
    mapper = MappingNetwork(input_dim=64, output_dim=128, num_layers=2, num_heads=4, seq_len_in=17, seq_len_out=77)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    img = torch.randn(1, 17, 64, generator=g)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    pipe = VideoGenPipeline(unet=net, mapper=mapper)
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, image_embeds=img, latents=lat, height=64, width=64, video_length=4,
               num_inference_steps=3, guidance_scale=7.5, generator=torch.Generator().manual_seed(3),
               output_type="latent").video.float().cpu()
    with torch.no_grad():
        cond = torch.cat([pe, mapper(img, pe)], 1).half().float()
        uncond = torch.cat([ne, mapper(img, ne)], 1).half().float()
    gen = torch.Generator().manual_seed(3)
    noises = [torch.randn(lat.shape, generator=gen) for _ in range(2)] + [None]
    fn = lambda x, t, c: O.unet_forward(sd, x, t, c, O.UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128,
                                                                  attn_levels=(True, False)))
    ref = cfg_denoise_loop(fn, lat, cond, uncond, noises, num_steps=3, guidance_scale=7.5)
    assert rel_l2(out, ref) < 3e-2
    # the image matters: without the mapper the same call is the text-only trajectory
    plain = VideoGenPipeline(unet=net)(prompt_embeds=pe, negative_prompt_embeds=ne, image_embeds=img, latents=lat, height=64,
                                       width=64, video_length=4, num_inference_steps=3, guidance_scale=7.5,
                                       generator=torch.Generator().manual_seed(3), output_type="latent").video.float().cpu()
    assert rel_l2(plain, out) > 1e-3
