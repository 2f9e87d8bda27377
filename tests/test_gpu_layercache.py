"""-m gpu: the layer cache of the UNet engine (DeepCache).

Bit properties of the three modes (a refresh forward is the plain forward; a reuse forward on the same inputs right after it recomputes
exactly the shallow layers on a bit-identical cache; a plain forward in between touches nothing), parity of a reuse step at new inputs
against the restated oracle walk of tests/layercache_cases.py at the project's whole-forward tolerance, the VSR model (temporal modules,
class labels), the refusals, and the pipelines against hand-written loops over the model's own forwards.

The model is the reduced base structure of tests/pagcases.py; tests/test_layercache_host.py shows that the parity cases separate the
right output from a stale, wrong-cut or ignored cache by more than 3 TOL_UNET.  No test here times anything."""
import pytest
import torch

import golden_util as G
import layercache_cases as LC
from gpu_util import TOL_UNET, rel_l2

pytestmark = pytest.mark.gpu
f16 = torch.float16
CASES = [(n, d) for n in LC.SHAPES for d in LC.DEPTHS]
IDS = [f"{n}-d{d}" for n, d in CASES]


def build(sd, **kw):
    from lavie_amd.unet import UNet3DConditionModel
    net = UNet3DConditionModel(init_weights=False, **kw)
    net.load_state_dict({k: v.to(f16) for k, v in sd.items()})
    return net.to("cuda", f16)


@pytest.fixture(scope="module")
def base():
    net = build(LC.base_weights(), **LC.BASE_KW)
    yield net
    net.disable_layer_cache()
    net.disable_freeu()


def fwd(net, x, t, ctx, mode=None):
    return net(x, t, encoder_hidden_states=ctx, layer_cache=mode).sample


# ------------------------------------------------------------------ 1. bit properties
def bit_properties(net, name, depth):
    x_old, x_new, ctx = (v.cuda() for v in LC.inputs(name))
    net.enable_layer_cache(depth)
    plain = fwd(net, x_old, LC.T_OLD, ctx)
    refresh = fwd(net, x_old, LC.T_OLD, ctx, "refresh")
    assert torch.equal(refresh, plain)                                   # the full walk, bit for bit
    reuse = fwd(net, x_old, LC.T_OLD, ctx, "reuse")
    assert torch.equal(reuse, refresh)                                   # the shallow layers recomputed on a bit-identical cache
    other = fwd(net, x_new, LC.T_NEW, ctx)                               # a plain forward at other inputs in between ...
    assert not torch.equal(other, plain)
    assert torch.equal(fwd(net, x_old, LC.T_OLD, ctx, "reuse"), refresh)     # ... leaves the cache valid and unchanged
    moved = fwd(net, x_new, LC.T_NEW, ctx, "reuse")                      # and the reuse step follows its own input
    assert not torch.equal(moved, refresh) and not torch.equal(moved, other)
    assert net.layer_cache_bytes() >= x_old.shape[0] * x_old.shape[2] * x_old.shape[3] * x_old.shape[4] * LC.WIDTHS[0] * 2
    return plain


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared-prefix"])
@pytest.mark.parametrize("name,depth", CASES, ids=IDS)
def test_modes_bit_properties(base, name, depth, shared):
    base.disable_freeu()
    x_old, _, ctx = LC.inputs(name)
    base.prepare(*x_old.shape[:1], *x_old.shape[2:], ctx.shape[1])
    base.set_cfg_shared_input(shared)
    try:
        bit_properties(base, name, depth)
    finally:
        base.set_cfg_shared_input(False)


def test_modes_bit_properties_with_freeu(base):
    """FreeU acts in the two deepest up blocks only, layers a reuse step does not run: nothing to special-case."""
    name, depth = "F3-24x40", 1
    base.disable_freeu()
    x_old, _, ctx = (v.cuda() for v in LC.inputs(name))
    off = fwd(base, x_old, LC.T_OLD, ctx)
    base.enable_freeu(0.9, 0.2, 1.5, 1.6)
    try:
        on = bit_properties(base, name, depth)
        assert not torch.equal(on, off)
    finally:
        base.disable_freeu()


# ------------------------------------------------------------------ 2. parity of a reuse step at new inputs
@pytest.mark.parametrize("name,depth", CASES, ids=IDS)
def test_reuse_step_vs_restated_oracle(base, name, depth):
    """refresh at (x, t), reuse at (x', t') against shallow(x', t', feature of the reference full walk at (x, t)).

    Bound: TOL_UNET, the project's tolerance for one whole forward; the shallow walk has fewer layers than the forward that
    tolerance was set for."""
    base.disable_freeu()
    r = LC.refs(name, depth)
    x_old, x_new, ctx = (v.cuda() for v in LC.inputs(name))
    base.enable_layer_cache(depth)
    refresh = fwd(base, x_old, LC.T_OLD, ctx, "refresh")
    reuse = fwd(base, x_new, LC.T_NEW, ctx, "reuse")
    e_full, e_reuse = rel_l2(refresh, r["full_old"]), rel_l2(reuse, r["shallow"])
    print(f"{name} depth {depth}: refresh vs oracle {e_full:.3e}, reuse vs restated shallow walk {e_reuse:.3e} (TOL_UNET {TOL_UNET})")
    assert e_full < TOL_UNET
    assert e_reuse < TOL_UNET


# ------------------------------------------------------------------ 3. the VSR model
SMALL_VSR3 = dict(sample_size=8, block_out_channels=(256, 512, 512),
                  down_block_types=("DownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D"),
                  up_block_types=("CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "UpBlock3D"), only_cross_attention=(True, True, False),
                  layers_per_block=1, cross_attention_dim=128, attention_head_dim=8, down_temporal_idx=(0, 1, 2), mid_temporal=True,
                  up_temporal_idx=(0, 1, 2))


@pytest.fixture(scope="module")
def small_vsr3():
    """The reduced VSR model of tests/test_gpu_vsr.py with a third level, which the layer cache needs.  layers_per_block = 1: depth 1
    is the full depth, so cut B lies right behind the temporal module that follows the upsampler into level 0."""
    from lavie_amd import spec
    from lavie_amd.config import UNetConfig
    from lavie_amd.vsr import UNet3DVSRModel
    cfg = UNetConfig(in_channels=7, block_out_channels=(256, 512, 512), cross_attention_dim=128, attn_levels=(False, True, True),
                     layers_per_block=1, vsr_blocks=True, only_cross_attention=(True, True, False), vsr_temporal_modules=True,
                     num_class_embeds=1000)
    net = UNet3DVSRModel(init_weights=False, **SMALL_VSR3)
    net.load_state_dict({k: v.to(f16) for k, v in G.synth16(spec.param_shapes(cfg), 31).items()})
    return net.to("cuda", f16)


def test_vsr_modes_bit_properties(small_vsr3):
    net = small_vsr3
    g = torch.Generator().manual_seed(12)
    b, f, h, w = 2, 5, 8, 8
    x, x2 = torch.randn(b, 4, f, h, w, generator=g).half().cuda(), torch.randn(b, 4, f, h, w, generator=g).half().cuda()
    low = torch.randn(b, 3, f, h, w, generator=g).half().cuda()
    ctx = torch.randn(b, 77, 128, generator=g).half().cuda()
    labels = torch.tensor([20, 250])
    run = lambda x, t, mode=None: net(x, t, low, encoder_hidden_states=ctx, class_labels=labels, layer_cache=mode).sample
    net.enable_layer_cache(1)
    try:
        plain = run(x, 500)
        refresh = run(x, 500, "refresh")
        assert torch.equal(refresh, plain)
        assert torch.equal(run(x, 500, "reuse"), refresh)
        other = run(x2, 321)
        assert torch.equal(run(x, 500, "reuse"), refresh)
        moved = run(x2, 321, "reuse")
        assert not torch.equal(moved, refresh) and not torch.equal(moved, other)
        assert net.layer_cache_bytes() >= b * f * h * w * 512 * 2            # full depth: level 1's width
        with pytest.raises(ValueError, match="depth=2"):
            net.enable_layer_cache(2)
    finally:
        net.disable_layer_cache()


# ------------------------------------------------------------------ 4. refusals
def test_refusals_return_errors(base):
    from lavie_amd import _lib
    base.disable_freeu()
    x_old, x_new, ctx = (v.cuda() for v in LC.inputs("F4-16x16"))
    base.enable_layer_cache(1)                                           # drops whatever an earlier test cached
    plain = fwd(base, x_old, LC.T_OLD, ctx)
    with pytest.raises(RuntimeError, match="refresh"):                   # reuse before refresh
        fwd(base, x_old, LC.T_OLD, ctx, "reuse")
    fwd(base, x_old, LC.T_OLD, ctx, "refresh")
    b, _, f, h, w = x_old.shape
    base.prepare(b, f, h * 2, w, ctx.shape[1])                           # prepare at another shape invalidates
    with pytest.raises(RuntimeError, match="refresh"):
        fwd(base, x_old, LC.T_OLD, ctx, "reuse")
    fwd(base, x_old, LC.T_OLD, ctx, "refresh")
    with pytest.raises(RuntimeError, match="forward_cached"):            # another B
        fwd(base, x_old[:1], LC.T_OLD, ctx[:1], "reuse")
    # the engine's own tuple check, past the model's prepare: same prepared shape, another batch in the call
    base.prepare(b, f, h, w, ctx.shape[1])
    fwd(base, x_old, LC.T_OLD, ctx, "refresh")
    lib, out = _lib.load(), torch.empty(1, 4, f, h, w, dtype=f16, device="cuda")
    t = torch.full((1,), float(LC.T_OLD), device="cuda")
    import ctypes
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.lavie_unet_forward_cached(base.engine_handle(), p(x_old), p(t), p(ctx), None, p(out), 1, f, h, w, ctx.shape[1], 2, stream)
    assert rc != 0 and b"B=1" in lib.lavie_last_error()
    assert lib.lavie_unet_forward_cached(base.engine_handle(), p(x_old), p(t), p(ctx), None, p(out), 1, f, h, w, ctx.shape[1], 3, stream) != 0
    assert torch.equal(fwd(base, x_old, LC.T_OLD, ctx, "reuse"), plain)  # the refused calls left the cache as it was
    # depth above layers_per_block: the model and the engine
    with pytest.raises(ValueError, match="depth=3"):
        base.enable_layer_cache(3)
    assert lib.lavie_unet_set_layer_cache(base.engine_handle(), 3) != 0 and b"depth=3" in lib.lavie_last_error()
    assert torch.equal(fwd(base, x_old, LC.T_OLD, ctx, "reuse"), plain)
    # the graph entry has no cached form
    base.enable_graph(True)
    try:
        with pytest.raises(RuntimeError, match="graph"):
            fwd(base, x_old, LC.T_OLD, ctx, "reuse")
    finally:
        base.enable_graph(False)
    base.disable_layer_cache()
    assert base.layer_cache_bytes() == 0
    with pytest.raises(RuntimeError, match="enable_layer_cache"):
        fwd(base, x_old, LC.T_OLD, ctx, "reuse")
    assert torch.equal(fwd(base, x_old, LC.T_OLD, ctx), plain)


# ------------------------------------------------------------------ 5. the pipelines
STEPS, INTERVAL, GUIDANCE = 6, 3, 7.5


def test_base_pipeline_is_the_hand_loop(base):
    """denoise(cache_interval=3) over 6 DDIM steps against a loop written here: the model's own forwards with the scheduled modes and
    the same fused step ops; cache_interval = 1 is the call without the argument."""
    from lavie_amd import ops, sampling
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddim import DDIMScheduler
    base.disable_freeu()
    base.disable_layer_cache()
    pipe = VideoGenPipeline(unet=base, scheduler=DDIMScheduler())
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(1, 4, 4, 16, 16, generator=g).cuda()
    ctx = torch.randn(2, 77, 128, generator=g).half().cuda()
    plain = pipe.denoise(lat, ctx, STEPS, GUIDANCE)
    assert torch.equal(pipe.denoise(lat, ctx, STEPS, GUIDANCE, cache_interval=1), plain)
    assert torch.equal(pipe.denoise(lat, ctx, STEPS, GUIDANCE, cache_interval=None, cache_depth=2), plain)
    seen = []
    cached = pipe.denoise(lat, ctx, STEPS, GUIDANCE, cache_interval=INTERVAL, callback=lambda i, t, x: seen.append(base.layer_cache))
    assert seen == [1] * STEPS and base.layer_cache == 0                 # on for the loop, the model's own setting afterwards
    assert not torch.equal(cached, plain)

    plan = sampling.StepPlan(DDIMScheduler(), STEPS)
    x = lat.float().contiguous().clone()
    model_in = torch.empty((2,) + tuple(x.shape[1:]), dtype=f16, device="cuda")
    ops.latents_to_model_input(x, model_in, plan.input_scale(0))
    t_dev = plan.t_dev(x.device)
    modes = LC.schedule(STEPS, INTERVAL)
    assert modes == ["refresh", "reuse", "reuse"] * 2
    base.enable_layer_cache(1)
    try:
        with sampling.engine_session(base, 2, 4, 16, 16, ctx, [model_in] if pipe.cfg_shared_prefix else None) as c:
            for i in range(STEPS):
                eps = base(model_in, t_dev[i], encoder_hidden_states=c, layer_cache=modes[i]).sample
                sampling.step(eps, x, None, model_in, GUIDANCE, plan.coeffs(i), plan.input_scale(i + 1), False)
    finally:
        base.disable_layer_cache()
    assert torch.equal(cached, x)
    # a late start refreshes on its first executed step: the known-latents run at start_step = 2 goes through
    late = pipe.denoise(lat, ctx, STEPS, GUIDANCE, known=lat, start_step=2, cache_interval=INTERVAL)
    assert torch.isfinite(late).all()


def test_vsr_pipeline_is_the_hand_loop(small_vsr3):
    from lavie_amd import ops, sampling
    from lavie_amd.scheduling_ddim import DDIMScheduler
    from lavie_amd.vsr import VideoUpscalePipeline
    net = small_vsr3
    pipe = VideoUpscalePipeline(unet=net, scheduler=DDIMScheduler())
    g = torch.Generator().manual_seed(22)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g).cuda()
    image = torch.randn(1, 3, 4, 8, 8, generator=g).cuda()
    ctx = torch.randn(2, 77, 128, generator=g).half().cuda()
    plain = pipe.denoise(lat, image, ctx, 20, STEPS, GUIDANCE)
    assert torch.equal(pipe.denoise(lat, image, ctx, 20, STEPS, GUIDANCE, cache_interval=1), plain)
    cached = pipe.denoise(lat, image, ctx, 20, STEPS, GUIDANCE, cache_interval=INTERVAL)
    assert net.layer_cache == 0 and not torch.equal(cached, plain)

    plan = sampling.StepPlan(DDIMScheduler(), STEPS)
    x = lat.float().contiguous().clone()
    model_in = torch.empty((2,) + tuple(x.shape[1:]), dtype=f16, device="cuda")
    ops.latents_to_model_input(x, model_in, plan.input_scale(0))
    low = torch.cat([image, image]).to(f16).contiguous()
    labels = torch.full((2,), 20, dtype=torch.int64)
    t_dev = plan.t_dev(x.device)
    modes = LC.schedule(STEPS, INTERVAL)
    net.enable_layer_cache(1)
    try:
        with sampling.engine_session(net, 2, 4, 8, 8, ctx) as c:
            for i in range(STEPS):
                eps = net(model_in, t_dev[i], low, encoder_hidden_states=c, class_labels=labels, layer_cache=modes[i]).sample
                sampling.step(eps, x, None, model_in, GUIDANCE, plan.coeffs(i), plan.input_scale(i + 1), False)
    finally:
        net.disable_layer_cache()
    assert torch.equal(cached, x)
