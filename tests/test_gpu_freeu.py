"""-m gpu: FreeU inside the engine's forward (lavie_unet_set_freeu) against the oracle's walk with FreeU inserted in
torch.fft form, and the properties of the setting: off is the plain forward bit for bit, reproducible, inside the planned workspace,
through a captured graph, through the pipelines.

The base model is the base structure (four levels, attention on the first three) at reduced width, 256 / 256 / 512 / 512: at a 16 x 16
latent up blocks 0 and 1 see 2 x 2 and 4 x 4 images, at 24 x 40 they see 3 x 5 and 6 x 10, with C_h != C2 at the block boundary."""
import pytest
import torch

import golden_util as G
from gpu_util import TOL_UNET, rel_l2

pytestmark = pytest.mark.gpu

FREEU = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
WIDTHS, ATTN = (256, 256, 512, 512), (True, True, True, False)
BASE_KW = dict(sample_size=16, block_out_channels=WIDTHS, cross_attention_dim=128)
CASES = {"F4-16x16": (2, 4, 16, 16, 500), "F3-24x40": (1, 3, 24, 40, 321)}


# ------------------------------------------------------------------ the reference: oracle.unet_fp32.unet_forward's walk with FreeU
def fourier_filter(x, s):
    """diffusers' fourier_filter(x, threshold=1, scale=s) on [n, c, h, w], in float64"""
    H, W = x.shape[-2:]
    X = torch.fft.fftshift(torch.fft.fftn(x.double(), dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(X.shape, dtype=torch.float64)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(X * mask, dim=(-2, -1)), dim=(-2, -1)).real.to(x.dtype)


def apply_freeu(i, x, skip, s1, s2, b1, b2):
    """diffusers' apply_freeu on video tensors [b, c, f, h, w]: every frame is an image"""
    if i > 1:
        return x, skip
    b, s = (b1, s1) if i == 0 else (b2, s2)
    x = x.clone()
    x[:, :x.shape[1] // 2] = x[:, :x.shape[1] // 2] * b
    bs, c, f, h, w = skip.shape
    flat = skip.permute(0, 2, 1, 3, 4).reshape(bs * f, c, h, w)
    return x, fourier_filter(flat, s).reshape(bs, f, c, h, w).permute(0, 2, 1, 3, 4)


def unet_forward_freeu(sd, sample, timesteps, ctx, cfg, freeu=None):
    """oracle.unet_fp32.unet_forward, restated from its piece functions, with apply_freeu in front of every resnet of the up walk"""
    from oracle import unet_fp32 as O
    sample = sample.float()
    t = torch.as_tensor(timesteps).reshape(-1).expand(sample.shape[0])
    emb = O.time_embedding(sd, t, cfg)
    ctx = ctx.float()
    nlev = len(cfg.block_out_channels)
    x = O.conv_frames(sample, sd["conv_in.weight"], sd["conv_in.bias"])
    skips = [x]
    for lvl in range(nlev):
        for j in range(cfg.layers_per_block):
            x = O.resnet_block(sd, f"down_blocks.{lvl}.resnets.{j}.", x, emb, cfg)
            if cfg.attn_levels[lvl]:
                x = O.transformer3d(sd, f"down_blocks.{lvl}.attentions.{j}.", x, ctx, cfg)
            skips.append(x)
        if lvl != nlev - 1:
            x = O.downsample(sd, f"down_blocks.{lvl}.downsamplers.0.", x)
            skips.append(x)
    x = O.resnet_block(sd, "mid_block.resnets.0.", x, emb, cfg)
    x = O.transformer3d(sd, "mid_block.attentions.0.", x, ctx, cfg)
    x = O.resnet_block(sd, "mid_block.resnets.1.", x, emb, cfg)
    for i in range(nlev):
        lvl = nlev - 1 - i
        for j in range(cfg.layers_per_block + 1):
            skip = skips.pop()
            if freeu:
                x, skip = apply_freeu(i, x, skip, **freeu)
            x = O.resnet_block(sd, f"up_blocks.{i}.resnets.{j}.", torch.cat([x, skip], dim=1), emb, cfg)
            if cfg.attn_levels[lvl]:
                x = O.transformer3d(sd, f"up_blocks.{i}.attentions.{j}.", x, ctx, cfg)
        if i != nlev - 1:
            x = O.upsample(sd, f"up_blocks.{i}.upsamplers.0.", x)
    x = torch.nn.functional.silu(O.group_norm_video(x, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], cfg.norm_groups, cfg.norm_eps))
    return O.conv_frames(x, sd["conv_out.weight"], sd["conv_out.bias"])


def ocfg():
    from oracle import unet_fp32 as O
    return O.UNetConfig(block_out_channels=WIDTHS, cross_attention_dim=128, attn_levels=ATTN)


@pytest.fixture(scope="module")
def base():
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    from lavie_amd.unet import UNet3DConditionModel
    sd = G.synth16(spec.param_shapes(UNetConfig(block_out_channels=WIDTHS, cross_attention_dim=128, attn_levels=ATTN)), 11)
    net = UNet3DConditionModel(init_weights=False, **BASE_KW)
    net.load_state_dict({k: v.to(torch.float16) for k, v in sd.items()})
    yield net.to("cuda", torch.float16), sd
    net.disable_freeu()


def inputs(name):
    b, f, h, w, t = CASES[name]
    g = torch.Generator().manual_seed(1000 + f)
    return torch.randn(b, 4, f, h, w, generator=g).half(), torch.randn(b, 77, 128, generator=g).half(), t


@pytest.fixture(scope="module")
def refs(base):
    """name -> (ref with FreeU, plain ref): computed once, on the CPU"""
    _, sd = base
    out = {}
    for name in CASES:
        x, ctx, t = inputs(name)
        out[name] = (unet_forward_freeu(sd, x.float(), t, ctx.float(), ocfg(), FREEU), unet_forward_freeu(sd, x.float(), t, ctx.float(), ocfg()))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_restated_walk_is_the_oracles_and_freeu_moves_it(base, refs, name):
    """CPU only: without FreeU the restated walk is oracle.unet_forward bit for bit; with the chosen factors the reference moves by
    more than 3 TOL_UNET, so a forward that ignores FreeU cannot pass the comparison below"""
    from oracle import unet_fp32 as O
    _, sd = base
    x, ctx, t = inputs(name)
    ref_on, ref_off = refs[name]
    assert torch.equal(ref_off, O.unet_forward(sd, x.float(), t, ctx.float(), ocfg()))
    d = rel_l2(ref_on, ref_off)
    print(f"{name}: rel_l2(ref_on, ref_off) = {d:.4f}")
    assert d > 3 * TOL_UNET


@pytest.mark.parametrize("name", list(CASES))
def test_forward_with_freeu_vs_reference(base, refs, name):
    net, _ = base
    x, ctx, t = inputs(name)
    ref_on, ref_off = refs[name]
    plain = net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()
    assert rel_l2(plain, ref_off) <= TOL_UNET
    net.enable_freeu(**FREEU)
    try:
        got = net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()
        again = net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()
    finally:
        net.disable_freeu()
    d = rel_l2(got, ref_on)
    print(f"{name}: rel_l2(got, ref_on) = {d:.3e}, rel_l2(plain, ref_off) = {rel_l2(plain, ref_off):.3e}")
    assert d <= TOL_UNET
    assert torch.equal(got, again)                                               # two runs are bit-equal
    assert torch.equal(net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample, plain)      # enable then disable: the plain bits
    net.enable_freeu(1, 1, 1, 1)
    assert torch.equal(net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample, plain)
    # one factor per stage: b1 and s2 alone
    net.enable_freeu(1.0, FREEU["s2"], FREEU["b1"], 1.0)
    try:
        part = net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()
    finally:
        net.disable_freeu()
    assert rel_l2(part, plain) > 1e-2 and rel_l2(part, got) > 1e-2
    _, sd = base
    assert rel_l2(part, unet_forward_freeu(sd, x.float(), t, ctx.float(), ocfg(), dict(s1=1.0, s2=FREEU["s2"], b1=FREEU["b1"], b2=1.0))) <= TOL_UNET


def test_identical_cfg_halves_give_identical_halves(base):
    net, _ = base
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, 4, 4, 16, 16, generator=g).half().cuda()
    x = torch.cat([lat, lat]).contiguous()
    c1 = torch.randn(1, 77, 128, generator=g).half().cuda()
    ctx = torch.cat([c1, c1]).contiguous()
    net.enable_freeu(**FREEU)
    try:
        y = net(x, 400, encoder_hidden_states=ctx).sample.clone()
        assert torch.equal(y[0], y[1])
        net.set_cfg_shared_input(True)
        ys = net(x, 400, encoder_hidden_states=ctx).sample.clone()
        assert torch.equal(ys[0], ys[1]) and rel_l2(ys, y) < 2e-3
    finally:
        net.set_cfg_shared_input(False)
        net.disable_freeu()


def test_enabling_after_prepare_needs_no_new_workspace():
    """a fresh model: prepare() for the shape, then enable_freeu, then forward: the planned workspace serves it"""
    from lavie_amd import _lib, spec
    from lavie_amd.config import UNetConfig
    from lavie_amd.unet import UNet3DConditionModel
    sd = G.synth16(spec.param_shapes(UNetConfig(block_out_channels=WIDTHS, cross_attention_dim=128, attn_levels=ATTN)), 11)
    net = UNet3DConditionModel(init_weights=False, **BASE_KW)
    net.load_state_dict({k: v.to(torch.float16) for k, v in sd.items()})
    net = net.to("cuda", torch.float16)
    x, ctx, t = inputs("F3-24x40")
    net.prepare(1, 3, 24, 40, 77)
    lib, handle = _lib.load(), net.engine_handle()
    before = lib.lavie_unet_workspace_bytes(handle)
    plain = net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()
    net.enable_freeu(**FREEU)
    on = net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()
    assert lib.lavie_unet_workspace_bytes(handle) == before
    assert rel_l2(on, plain) > 3 * TOL_UNET


def test_graph_replay_follows_the_setting(base):
    net, _ = base
    x, ctx, t = inputs("F4-16x16")
    x, ctx = x.cuda(), ctx.cuda()
    eager = {}
    for key, vals in (("off", (1, 1, 1, 1)), ("on", tuple(FREEU[k] for k in ("s1", "s2", "b1", "b2")))):
        net.enable_freeu(*vals)
        eager[key] = net(x, t, encoder_hidden_states=ctx).sample.clone()
    net.disable_freeu()
    assert not torch.equal(eager["on"], eager["off"])
    try:
        net.enable_graph(True)
        for key, vals in (("off", (1, 1, 1, 1)), ("on", tuple(FREEU[k] for k in ("s1", "s2", "b1", "b2"))), ("off", (1, 1, 1, 1))):
            net.enable_freeu(*vals)
            for i in range(3):                                   # eager, capture, replay
                assert torch.equal(net(x, t, encoder_hidden_states=ctx).sample, eager[key]), (key, i)
    finally:
        net.enable_graph(False)
        net.disable_freeu()


# ------------------------------------------------------------------ interpolation and VSR (reduced configurations of their own tests)
def test_interpolation_model_with_freeu():
    """the interpolation model shares the walk: compared with the same helper (the oracle has its piece functions)"""
    import test_gpu_interpolation as TI
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    cfg = UNetConfig(in_channels=8, block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False),
                     sparse_causal_attn1=True, temporal_plain=True, ff_before_temporal=True)
    sd = G.synth16(spec.param_shapes(cfg), 21)
    net = TI.build(sd, **TI.SMALL_KW)
    g = torch.Generator().manual_seed(77)
    x, ctx = torch.randn(2, 8, 5, 8, 8, generator=g).half(), torch.randn(2, 77, 128, generator=g).half()
    plain = net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample.clone()
    net.enable_freeu(**FREEU)
    on = net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample.clone()
    assert torch.equal(on, net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample)
    ref_on = unet_forward_freeu(sd, x.float(), 300, ctx.float(), TI.ocfg_small(), FREEU)
    ref_off = unet_forward_freeu(sd, x.float(), 300, ctx.float(), TI.ocfg_small())
    print(f"interpolation: on vs ref {rel_l2(on, ref_on):.3e}, ref_on vs ref_off {rel_l2(ref_on, ref_off):.4f}")
    assert rel_l2(ref_on, ref_off) > 3 * TOL_UNET and rel_l2(on, ref_on) <= TOL_UNET
    net.disable_freeu()
    assert torch.equal(net(x.cuda(), 300, encoder_hidden_states=ctx.cuda()).sample, plain)


def test_vsr_model_with_freeu():
    """the VSR walk has temporal modules behind the resnets; the oracle offers its forward whole (vsr_blocks.vsr_unet_forward), not as
    a walk to restate: on != off, reproducible, and off again is the plain forward"""
    import test_gpu_vsr as TV
    net, _ = TV.build_small_vsr()
    g = torch.Generator().manual_seed(205)
    x, low = torch.randn(2, 4, 5, 8, 8, generator=g).half().cuda(), torch.randn(2, 3, 5, 8, 8, generator=g).half().cuda()
    ctx = torch.randn(2, 77, 128, generator=g).half().cuda()
    t, labels = torch.tensor([41.0, 82.0]).cuda(), torch.tensor([20, 250])
    fwd = lambda: net(x, t, low, encoder_hidden_states=ctx, class_labels=labels).sample.clone()
    plain = fwd()
    net.enable_freeu(**FREEU)
    on = fwd()
    assert torch.equal(on, fwd()) and torch.isfinite(on).all()
    assert rel_l2(on, plain) > 1e-2
    net.disable_freeu()
    assert torch.equal(fwd(), plain)


# ------------------------------------------------------------------ pipelines
def test_pipeline_steps_with_freeu_are_the_models(base):
    """two guided DDPM steps through VideoGenPipeline after enable_freeu: the oracle's guided loop driven by hand on the same model
    gives the same latents, and the plain call differs"""
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from oracle.ddpm import cfg_denoise_loop
    net, _ = base
    pipe = VideoGenPipeline(unet=net)
    g = torch.Generator().manual_seed(9)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    lat = torch.randn(1, 4, 4, 16, 16, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=128, width=128, video_length=4, num_inference_steps=2,
              guidance_scale=7.5, output_type="latent")
    plain = pipe(generator=torch.Generator().manual_seed(3), **kw).video.float().cpu()
    pipe.enable_freeu(**FREEU)
    try:
        assert net.freeu == tuple(FREEU[k] for k in ("s1", "s2", "b1", "b2"))
        on = pipe(generator=torch.Generator().manual_seed(3), **kw).video.float().cpu()
        gen = torch.Generator().manual_seed(3)
        noises = [torch.randn(lat.shape, generator=gen), None]
        fn = lambda x, t, c: net(x.half().cuda(), int(t), encoder_hidden_states=c.half().cuda()).sample.float().cpu()
        hand = cfg_denoise_loop(fn, lat, pe.half().float(), ne.half().float(), noises, num_steps=2, guidance_scale=7.5)
    finally:
        pipe.disable_freeu()
    print(f"pipeline: on vs hand loop {rel_l2(on, hand):.3e}, on vs plain {rel_l2(on, plain):.3e}")
    assert rel_l2(on, hand) < 5e-3 and rel_l2(on, plain) > 2e-2
    assert net.freeu == (1.0, 1.0, 1.0, 1.0)


def test_cascade_restores_the_setting(monkeypatch):
    """text_to_video_cascade(base_freeu=, vsr_freeu=): set for the call, seen by the stages, and the models' own settings afterwards"""
    from lavie_amd import cascade

    class Unet:
        freeu = (1.0, 1.0, 1.0, 1.0)

        def enable_freeu(self, s1, s2, b1, b2):
            self.freeu = (s1, s2, b1, b2)

    class Pipe:
        def __init__(self):
            self.unet, self.scheduler = Unet(), None

    base_pipe, vsr_pipe = Pipe(), Pipe()
    vsr_pipe.unet.freeu = (0.8, 0.8, 1.1, 1.1)
    seen = []
    monkeypatch.setattr(cascade, "_cascade", lambda *a, **k: seen.append((base_pipe.unet.freeu, vsr_pipe.unet.freeu)) or "ran")
    args = [base_pipe, None, None, vsr_pipe] + [None] * 8
    assert cascade.text_to_video_cascade(*args, base_freeu=FREEU) == "ran"
    assert seen == [((0.9, 0.2, 1.5, 1.6), (0.8, 0.8, 1.1, 1.1))]
    assert base_pipe.unet.freeu == (1.0, 1.0, 1.0, 1.0) and vsr_pipe.unet.freeu == (0.8, 0.8, 1.1, 1.1)
    cascade.text_to_video_cascade(*args, vsr_freeu=dict(s1=0.5, s2=0.5, b1=1.2, b2=1.2))
    assert seen[1] == ((1.0, 1.0, 1.0, 1.0), (0.5, 0.5, 1.2, 1.2)) and vsr_pipe.unet.freeu == (0.8, 0.8, 1.1, 1.1)

    def boom(*a, **k):
        raise KeyError("stage failed")
    monkeypatch.setattr(cascade, "_cascade", boom)
    with pytest.raises(KeyError):
        cascade.text_to_video_cascade(*args, base_freeu=FREEU, vsr_freeu=FREEU)
    assert base_pipe.unet.freeu == (1.0, 1.0, 1.0, 1.0) and vsr_pipe.unet.freeu == (0.8, 0.8, 1.1, 1.1)
