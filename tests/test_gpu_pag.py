"""-m gpu: perturbed-attention guidance.  The four fused steps per element against the float64 restatement of
tests/pagcases.py; the identity attn1 through the transformer seam and the whole forward against the patched oracle, on the kernel
routes the engine has; the properties of the setting (off is the plain forward bit for bit, reproducible, inside the planned workspace,
followed by a captured graph); the pipeline against a hand loop.

The forward model is the reduced base structure of tests/test_gpu_freeu.py (256 / 256 / 512 / 512, attention on the first three
levels, synth16 weights); the layer sets are fixed by tests/test_pag_host.py."""
import pytest
import torch

import golden_util as G
import opcheck as oc
import pagcases as P
from gpu_util import TOL_BLOCK, TOL_UNET, h16, rel_l2

pytestmark = pytest.mark.gpu
f16, f32t = torch.float16, torch.float32


def sync():
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ops():
    from lavie_amd import ops as o
    return o


# ------------------------------------------------------------------ 1. the steps
def plain_name(family, cfg):
    return {("five", True): "cfg_ddpm_step", ("five", False): "sampler_step", ("multistep", True): "cfg_multistep_step",
            ("multistep", False): "multistep_step"}[family, cfg]


def pag_name(family, cfg):
    return ("cfg_" if cfg else "") + "pag_" + ("multistep_step" if family == "multistep" else "sampler_step")


def run_step(ops, family, cfg, d, pag_scale, plain=False):
    """The PAG step (or, plain=True, the plain namesake on the leading parts) on guarded operands; returns x, aux, model_in."""
    eps = d["eps"][:-1] if plain else d["eps"]
    ins = {"eps": eps.contiguous(), "x": d["x"], "aux": d["aux"]}
    outs = {"model_in": (tuple(eps.shape), f16), "x": (tuple(d["x"].shape), f32t), "aux": (tuple(d["x"].shape), f32t)}
    alias = {"x": "x", "aux": "aux"}
    if family == "five":
        outs.pop("aux")
        alias.pop("aux")
    g = (P.GUIDANCE,) if cfg else ()

    def run(i, o):
        if plain:
            getattr(ops, plain_name(family, cfg))(i["eps"], i["x"], i["aux"], o["model_in"], *g, P.COEFFS[family], P.IN_SCALE)
        else:
            getattr(ops, pag_name(family, cfg))(i["eps"], i["x"], i["aux"], o["model_in"], *g, pag_scale, P.COEFFS[family], P.IN_SCALE)

    return oc.run_guarded(run, ins, outs, alias=alias, sync=sync)


STEP_CASES = [(n, fam, cfg) for n in P.SIZES for fam in P.FAMILIES for cfg in P.CFGS]
STEP_IDS = [f"{n}-{fam}-{'cfg' if cfg else 'nocfg'}" for n, fam, cfg in STEP_CASES]


@pytest.mark.parametrize("name,family,cfg", STEP_CASES, ids=STEP_IDS)
def test_step_per_element_vs_float64(ops, name, family, cfg):
    """x (and x0_prev) inside the derived bound everywhere; the parts of model_in bit-equal to each other and to the family's
    rounding of the written x; run_guarded holds the guard bands and that two runs agree bit for bit."""
    d = P.step_inputs(name, cfg)
    parts = 3 if cfg else 2
    res = run_step(ops, family, cfg, d, P.PAG_SCALE)
    xn, m, x0, m0 = P.step64(family, d["eps"], cfg, d["x"], d["aux"], P.GUIDANCE, P.PAG_SCALE)
    oc.assert_elementwise(res["x"], xn, m, 2 * P.ROUNDINGS[family] * P.U32, label=f"{name} {family} cfg={cfg} x", u=0.0)
    if family == "multistep":
        oc.assert_elementwise(res["aux"], x0, m0, 2 * P.ROUNDINGS["history"] * P.U32, label=f"{name} {family} cfg={cfg} x0_prev", u=0.0)
    print(f"{name} {family} cfg={cfg}: worst |err| / bound = {oc.WORST.get(f'{name} {family} cfg={cfg} x', 0.0):.3f}")
    mi = res["model_in"].reshape(parts, -1)
    for k in range(1, parts):
        oc.assert_bits(mi[k], mi[0], label=f"model_in part {k} vs part 0")
    oc.assert_bits(mi, P.model_input(family, res["x"], P.IN_SCALE, parts), label="model_in vs the family's rounding")
    if family == "five":          # the bits lavie_latents_to_scaled_model_input1 gives for that x
        want = torch.empty(res["x"].numel(), dtype=f16, device="cuda")
        ops.latents_to_model_input1(res["x"].cuda().contiguous(), want, P.IN_SCALE)
        oc.assert_bits(mi[0], want.cpu(), label="model_in vs latents_to_model_input1")
    else:
        oc.assert_bits(mi[0], (res["x"].cuda() * P.IN_SCALE).half().cpu().reshape(-1), label="model_in vs (x scale).half()")


@pytest.mark.parametrize("name,family,cfg", STEP_CASES, ids=STEP_IDS)
def test_zero_scale_and_equal_parts_are_the_plain_step(ops, name, family, cfg):
    d = P.step_inputs(name, cfg)
    parts = 3 if cfg else 2
    plain = run_step(ops, family, cfg, d, 0.0, plain=True)
    zero = run_step(ops, family, cfg, d, 0.0)                                # pag_scale = 0: the bits of the plain namesake
    oc.assert_bits(zero["x"], plain["x"], label="x at pag_scale = 0")
    if family == "multistep":
        oc.assert_bits(zero["aux"], plain["aux"], label="x0_prev at pag_scale = 0")
    oc.assert_bits(zero["model_in"].reshape(parts, -1)[:parts - 1], plain["model_in"].reshape(parts - 1, -1), label="model_in at pag_scale = 0")
    same = dict(d, eps=torch.cat([d["eps"][:-1], d["eps"][-2:-1]]))          # ep = ec: an exact zero is added
    equal = run_step(ops, family, cfg, same, P.PAG_SCALE)
    assert torch.equal(equal["x"], plain["x"])
    assert family != "multistep" or torch.equal(equal["aux"], plain["aux"])
    assert torch.equal(equal["model_in"].reshape(parts, -1)[:parts - 1], plain["model_in"].reshape(parts - 1, -1))


def test_step_refusals_touch_nothing(ops):
    d = P.step_inputs("n8", True)
    with pytest.raises(RuntimeError, match="pag_scale=-1"):
        run_step(ops, "five", True, d, -1.0)
    with pytest.raises(RuntimeError, match="pag_scale"):
        run_step(ops, "multistep", True, d, float("nan"))


# ------------------------------------------------------------------ 2. the transformer seam
def build(sd, **kw):
    from lavie_amd.unet import UNet3DConditionModel
    net = UNet3DConditionModel(init_weights=False, **kw)
    net.load_state_dict({k: v.to(f16) for k, v in sd.items()})
    return net.to("cuda", f16)


@pytest.fixture(scope="module")
def base():
    sd = P.base_weights()
    net = build(sd, **P.BASE_KW)
    yield net, sd
    net.disable_pag()


@pytest.fixture(scope="module")
def wide320():
    """a two-level model whose first level has the production width, 320: the row-resident kernels are in reach"""
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    from oracle import unet_fp32 as O
    cfg = UNetConfig(block_out_channels=(320, 640), cross_attention_dim=128, attn_levels=(True, False))
    sd = G.synth16(spec.param_shapes(cfg), 5)
    net = build(sd, sample_size=16, block_out_channels=(320, 640), cross_attention_dim=128,
                down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
    yield net, sd, O.UNetConfig(block_out_channels=(320, 640), cross_attention_dim=128, attn_levels=(True, False))
    net.disable_pag()


def seam(ops, net, sd, ocfg, prefix, layers, C, b, f, h, w, seed, cached=False):
    from lavie_amd.ops import from_rows, to_rows
    from oracle import unet_fp32 as O
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(b, C, f, h, w, generator=g) * torch.linspace(0.5, 2, f).reshape(1, 1, f, 1, 1)).half().float()
    ctx = torch.randn(b, 77, 128, generator=g).half().float()
    with P.patched_oracle(layers, b, 1):
        ref = O.transformer3d(sd, prefix + ".", x, ctx, ocfg)
    plain = O.transformer3d(sd, prefix + ".", x, ctx, ocfg)
    assert rel_l2(ref[-1], plain[-1]) > 3 * TOL_BLOCK                        # the perturbation is visible at this seam
    net.set_pag(layers, 1)
    try:
        ctx_dev = h16(ctx)
        if cached:                                                           # the context bound into the fused text kernel's images
            net.prepare(b, f, h, w, 77)
            ctx_dev = net.cache_context(ctx_dev)
        y = ops.unet_transformer(net, prefix, h16(to_rows(x)), ctx_dev, b, f, h, w)
        got = from_rows(y.float().cpu(), b, f, h, w)
        with pytest.raises(RuntimeError, match="perturbed=1"):               # B <= perturbed
            ops.unet_transformer(net, prefix, h16(to_rows(x[:1])), h16(ctx[:1]), 1, f, h, w)
    finally:
        if cached:
            net.cache_context(None)
        net.disable_pag()
    for e in range(b):
        d = rel_l2(got[e], ref[e])
        print(f"{prefix} entry {e}: rel_l2 vs patched oracle {d:.3e}")
        assert d <= TOL_BLOCK, (e, d)


@pytest.mark.parametrize("route", ["default", "fused_mask=0", "ln_fold=0", "F16-cached-text"])
def test_seam_width_320(ops, wide320, route):
    """16 x 16, F = 2, B = 3, perturbed = 1: the fused head leaves q | k | v; under fused_mask(0) the LayerNorm-folded GEMM does, with
    the fold off the explicit LayerNorm + GEMM.  F = 16 at 8 x 8 with the context cached: attn1.to_out runs inside the fused text
    kernel (launch_cross_block), which must see the copied rows too."""
    from lavie_amd import _lib
    net, sd, ocfg = wide320
    lib, handle = _lib.load(), net.engine_handle()
    try:
        if route == "fused_mask=0":
            _lib.check(lib.lavie_debug_fused_mask(0))
        if route == "ln_fold=0":
            _lib.check(lib.lavie_debug_fused_mask(0))
            _lib.check(lib.lavie_unet_set_ln_fold(handle, 0))
        if route == "F16-cached-text":
            seam(ops, net, sd, ocfg, "down_blocks.0.attentions.0", ("down_blocks.0",), 320, 3, 16, 8, 8, 31, cached=True)
        else:
            seam(ops, net, sd, ocfg, "down_blocks.0.attentions.0", ("down_blocks.0",), 320, 3, 2, 16, 16, 30)
    finally:
        _lib.check(lib.lavie_debug_fused_mask(_lib.FUSED_DEFAULT))
        _lib.check(lib.lavie_unet_set_ln_fold(handle, 1))


def test_seam_mid_block_512(ops, base):
    net, sd = base
    seam(ops, net, sd, P.ocfg(), "mid_block.attentions.0", ("mid_block",), 512, 3, 4, 2, 2, 32)


# ------------------------------------------------------------------ 3. the whole forward
def forward(net, name):
    x, ctx, t = P.forward_inputs(name)
    return net(x.cuda(), t, encoder_hidden_states=ctx.cuda()).sample.clone()


@pytest.mark.parametrize("name", list(P.FORWARD_CASES))
def test_forward_vs_patched_oracle(base, name):
    net, _ = base
    ref, ref_plain = P.forward_refs(name, P.LAYERS_PARITY)
    plain = forward(net, name)
    net.set_pag(P.LAYERS_PARITY, 1)
    try:
        got = forward(net, name)
        again = forward(net, name)
    finally:
        net.disable_pag()
    for e in range(3):
        d = rel_l2(got[e], ref[e])
        print(f"{name} entry {e}: rel_l2(got, patched oracle) = {d:.3e}; plain vs plain oracle {rel_l2(plain[e], ref_plain[e]):.3e}")
        assert d <= TOL_UNET, (e, d)
    sep = rel_l2(got[2], got[1])
    print(f"{name}: rel_l2(perturbed third, prompt third) = {sep:.4f}")
    assert sep > 3 * TOL_UNET
    assert torch.equal(got[:2], plain[:2])                                   # the same launches see the same rows of the leading entries
    assert torch.equal(got, again)                                           # two runs are bit-equal
    assert torch.equal(forward(net, name), plain)                            # off after on: the plain forward bit for bit


@pytest.mark.parametrize("name", list(P.FORWARD_CASES))
def test_mid_block_alone_keeps_the_leading_entries_bits(base, name):
    net, _ = base
    ref, _ = P.forward_refs(name, P.LAYERS_BITS)
    plain = forward(net, name)
    net.set_pag(P.LAYERS_BITS, 1)
    try:
        got = forward(net, name)
    finally:
        net.disable_pag()
    assert torch.equal(got[:2], plain[:2]) and not torch.equal(got[2], plain[2])
    assert max(rel_l2(got[e], ref[e]) for e in range(3)) <= TOL_UNET


def test_refusals_on_a_finalized_engine(base):
    net, _ = base
    net.engine_handle()
    net.set_pag(P.LAYERS_BITS, 1)
    try:
        for bad, text in ((("mid_blocks",), "selects no transformer"), (("up_blocks.0",), "selects no transformer")):
            with pytest.raises(RuntimeError, match=text):
                net.set_pag(bad, 1)
            assert net.pag == (P.LAYERS_BITS, 1)
        net.set_pag(P.LAYERS_BITS, 3)
        with pytest.raises(RuntimeError, match="perturbed=3"):
            forward(net, "F4-16x16")                                         # B = 3 <= perturbed
    finally:
        net.disable_pag()


def test_enabling_after_prepare_needs_no_new_workspace():
    from lavie_amd import _lib
    net = build(P.base_weights(), **P.BASE_KW)
    b, f, h, w, _ = P.FORWARD_CASES["F3-24x40"]
    net.prepare(b, f, h, w, 77)
    lib, handle = _lib.load(), net.engine_handle()
    before = lib.lavie_unet_workspace_bytes(handle)
    plain = forward(net, "F3-24x40")
    net.set_pag(P.LAYERS_PARITY, 1)
    on = forward(net, "F3-24x40")
    assert lib.lavie_unet_workspace_bytes(handle) == before
    assert torch.equal(on[:2], plain[:2]) and rel_l2(on[2], plain[2]) > 3 * TOL_UNET


def test_graph_replay_follows_the_setting(base):
    net, _ = base
    x, ctx, t = P.forward_inputs("F4-16x16")
    x, ctx = x.cuda(), ctx.cuda()
    settings = (("off", ((), 0)), ("on", (P.LAYERS_PARITY, 1)), ("mid", (P.LAYERS_BITS, 1)))
    eager = {}
    for key, s in settings:
        net.set_pag(*s)
        eager[key] = net(x, t, encoder_hidden_states=ctx).sample.clone()
    net.disable_pag()
    assert not torch.equal(eager["on"], eager["off"]) and not torch.equal(eager["on"], eager["mid"])
    try:
        net.enable_graph(True)
        for key, s in settings + settings[:1]:
            net.set_pag(*s)
            for i in range(3):                                               # eager, capture, replay
                assert torch.equal(net(x, t, encoder_hidden_states=ctx).sample, eager[key]), (key, i)
    finally:
        net.enable_graph(False)
        net.disable_pag()


def test_shared_input_is_ignored_while_on(base):
    net, _ = base
    net.set_pag(P.LAYERS_PARITY, 1)
    try:
        want = forward(net, "F4-16x16")
        net.set_cfg_shared_input(True)                                       # B = 3: without PAG this forward would be refused
        assert torch.equal(forward(net, "F4-16x16"), want)
    finally:
        net.set_cfg_shared_input(False)
        net.disable_pag()


# ------------------------------------------------------------------ 4. the pipeline
TINY_KW = dict(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
               down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"))
TINY_LAYERS = ("mid_block", "up_blocks.1")
STEPS = 3


@pytest.fixture(scope="module")
def tiny():
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    sd = G.synth16(spec.param_shapes(UNetConfig(block_out_channels=(256, 512), cross_attention_dim=128, attn_levels=(True, False))), 7)
    return build(sd, **TINY_KW)


def scheduler(kind):
    if kind == "ddpm":
        from lavie_amd.scheduling_ddpm import DDPMScheduler
        return DDPMScheduler()
    if kind == "ddim":
        from lavie_amd.scheduling_ddim import DDIMScheduler
        return DDIMScheduler()
    from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler()


def hand_loop(net, kind, lat, pe, ne, guidance, pag_scale, seed):
    """the model's own forwards plus the formula in fp32 torch"""
    from lavie_amd import sampling
    plan = sampling.StepPlan(scheduler(kind), STEPS)
    gen = torch.Generator().manual_seed(seed)
    guided = guidance > 1.0
    ctx = torch.cat(([ne] if guided else []) + [pe, pe]).half().cuda()
    x, x0_prev = lat.float().cuda(), None
    net.set_pag(TINY_LAYERS, lat.shape[0])
    try:
        for i, t in enumerate(plan.timesteps):
            m = (x * plan.input_scale(i)).half()
            eps = net(torch.cat([m] * ctx.shape[0]).contiguous(), t, encoder_hidden_states=ctx).sample.float()
            ec, ep = eps[-2:-1], eps[-1:]
            e = (eps[:1] + guidance * (ec - eps[:1]) if guided else ec) + pag_scale * (ec - ep)
            k_x, k_e, c_x0, c_xt, c4 = plan.coeffs(i)
            x0 = k_x * x - k_e * e
            if plan.multistep:
                d = x0 + c4 * (x0 - x0_prev) if c4 != 0.0 else x0
                x, x0_prev = c_x0 * d + c_xt * x, x0
            else:
                xn = c_x0 * x0 + c_xt * x
                x = xn + c4 * torch.randn(lat.shape, generator=gen).cuda() if plan.adds_noise((k_x, k_e, c_x0, c_xt, c4)) else xn
    finally:
        net.disable_pag()
    return x.cpu()


@pytest.mark.parametrize("guidance", [7.5, 1.0], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpmsolver++"])
def test_pipeline_steps_are_the_hand_loops(tiny, kind, guidance):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline(unet=tiny, scheduler=scheduler(kind))
    g = torch.Generator().manual_seed(9)
    pe, ne = torch.randn(1, 77, 128, generator=g).half().float(), torch.randn(1, 77, 128, generator=g).half().float()
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, height=64, width=64, video_length=4, num_inference_steps=STEPS,
              guidance_scale=guidance, output_type="latent")
    pag = dict(pag_scale=3.0, pag_applied_layers=TINY_LAYERS)
    run = lambda **extra: pipe(generator=torch.Generator().manual_seed(3), **kw, **extra).video.float().cpu()
    plain = run()
    assert torch.equal(run(pag_scale=0.0, pag_adaptive_scale=0.5, pag_applied_layers=TINY_LAYERS), plain)     # pag_scale = 0: today's call
    on = run(**pag)
    assert tiny.pag == ((), 0)                                               # the setting is off again after the call
    hand = hand_loop(tiny, kind, lat, pe, ne, guidance, 3.0, 3)
    print(f"{kind} guidance={guidance}: on vs hand loop {rel_l2(on, hand):.3e}, on vs pag_scale = 0 {rel_l2(on, plain):.3e}")
    assert rel_l2(on, hand) < 5e-3
    assert rel_l2(on, plain) > 2e-2
    assert torch.equal(run(**pag), on)

    def boom(i, t, x):
        assert tiny.pag == (TINY_LAYERS, 1)                                  # made for the loop
        raise KeyError("stop inside the loop")

    with pytest.raises(KeyError):
        run(callback=boom, **pag)
    assert tiny.pag == ((), 0)
    assert torch.equal(run(), plain)                                         # and the engine's own setting went back with it


def test_adaptive_scale_reaches_the_step(tiny):
    """a fade that reaches 0 before the first step (t < 1000 - 3 / 0.5) leaves the guided trajectory: the batch still carries the
    perturbed part, the step adds an exact zero"""
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline(unet=tiny, scheduler=scheduler("ddim"))
    g = torch.Generator().manual_seed(9)
    pe, ne = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=torch.randn(1, 4, 4, 8, 8, generator=g), height=64, width=64, video_length=4,
              num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent")
    plain = pipe(**kw).video.float().cpu()
    faded = pipe(pag_scale=3.0, pag_adaptive_scale=0.5, pag_applied_layers=TINY_LAYERS, **kw).video.float().cpu()
    half = pipe(pag_scale=3.0, pag_adaptive_scale=0.002, pag_applied_layers=TINY_LAYERS, **kw).video.float().cpu()
    full = pipe(pag_scale=3.0, pag_applied_layers=TINY_LAYERS, **kw).video.float().cpu()
    assert rel_l2(faded, plain) < 5e-3                                       # (B = 3 forwards against B = 2 with the shared prefix: other launches, the hand-loop figure)
    assert rel_l2(full, plain) > rel_l2(half, plain) > rel_l2(faded, plain)
