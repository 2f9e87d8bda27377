"""The host side of the denoising-loss evaluation (lavie_amd/denoising_loss.py) without a GPU: snr and the min-SNR
weights against the closed forms, the chunking of more than sixteen latents, the refusals, the reduction, and the C entries'
argument checks (which touch no device)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import denoise_loss_reference as D
from lavie_amd import _lib, ops
from lavie_amd.denoising_loss import DenoisingLoss, min_snr_weights, noise_levels, snr
from lavie_amd.noise import PhiloxGenerator
from lavie_amd.scheduling_ddpm import DDPMScheduler

T = (0, 1, 500, 999)


def test_snr_and_weights_are_the_closed_forms():
    """snr = abar / (1 - abar), weights min(snr, 5) / snr and min(snr, 5) / (snr + 1), at t in {0, 1, 500, 999} on the scheduler's
    default betas.  The scheduler keeps cumprod(1 - beta) in fp32 from fp32 betas, the closed form here runs in float64: abar_t is a
    product of t + 1 factors, each with the rounding of its beta and of 1 - beta, and t roundings of the running product, so it is
    within (3 t + 3) 2^-24 (relative) of the float64 value; d snr / snr = d abar / (abar (1 - abar))."""
    sch = DDPMScheduler()
    ab = D.abar()[list(T)]
    got = snr(sch, T)
    assert got.dtype == torch.float64 and got.shape == (4,)
    rel = (3 * np.array(T) + 3) * 2.0 ** -24 / (1.0 - ab)
    assert np.all(np.abs(got.numpy() - D.snr(ab)) <= rel * D.snr(ab))
    exact = D.snr(sch.alphas_cumprod.double().numpy()[list(T)])                 # from the scheduler's own abar: float64 roundings only
    assert np.all(np.abs(got.numpy() - exact) <= 8 * 2.0 ** -53 * exact / (1.0 - sch.alphas_cumprod.double().numpy()[list(T)]))
    for kind in ("epsilon", "v_prediction"):
        w = min_snr_weights(got, 5.0, kind).numpy()
        want = D.min_snr_weights(got.numpy(), 5.0, kind)
        assert np.all(np.abs(w - want) <= 4 * 2.0 ** -53 * want)
    w = min_snr_weights(got, 5.0, "epsilon").numpy()
    assert w[0] == 5.0 / got[0] and w[3] == 1.0 and got[0] > 5.0 > got[3]       # clipped at t = 0, not at t = 999
    v = min_snr_weights(got, 5.0, "v_prediction").numpy()
    assert v[3] == float(got[3] / (got[3] + 1.0))
    with pytest.raises(ValueError, match="sample"):
        min_snr_weights(got, 5.0, "sample")
    with pytest.raises(ValueError, match="0..999"):
        snr(sch, [1000])


def test_levels_are_float64_roots_rounded_once():
    sch = DDPMScheduler()
    ab = sch.alphas_cumprod.double().numpy()
    for (a, s), t in zip(noise_levels(sch, T), T):
        assert a == float(np.float32(math.sqrt(ab[t]))) and s == float(np.float32(math.sqrt(1.0 - ab[t])))


class Recorder:
    """stands in for the two operators on CPU tensors: records the calls, writes mse[p] = the latent's first element"""

    def __init__(self):
        self.calls = []

    def noisy_latents(self, x0, seeds, draw, levels, offset=None, out=None):
        self.calls.append(("noisy_latents", tuple(x0.shape), list(seeds), draw, list(levels), offset))
        return x0.to(torch.float16)

    def denoising_loss(self, pred, x0, seeds, draw, levels, kind, offset=None, workspace=None, out=None):
        self.calls.append(("denoising_loss", tuple(pred.shape), list(seeds), draw, list(levels), kind, offset))
        out.copy_(x0.reshape(x0.shape[0], -1)[:, 0].float())
        return out


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "noisy_latents", r.noisy_latents)
    monkeypatch.setattr(ops, "denoising_loss", r.denoising_loss)
    return r


def forward(model_in, timesteps, ctx):
    assert model_in.shape[0] == timesteps.shape[0] == ctx.shape[0]
    return model_in


def test_nineteen_latents_run_as_sixteen_and_three(rec):
    sch = DDPMScheduler()
    x0 = torch.arange(19, dtype=torch.float32).reshape(19, 1, 1, 1, 1).expand(19, 4, 2, 2, 2).contiguous()
    ctx = torch.zeros(19, 3, 8)
    ts = list(range(0, 950, 50))
    for gen in (PhiloxGenerator(100, draw=7), PhiloxGenerator(list(range(300, 319)), draw=7)):
        rec.calls.clear()
        whole = PhiloxGenerator(gen._seed, draw=7)
        out = DenoisingLoss(None, sch, forward=forward).evaluate(x0, ctx, ts, gen)
        assert [c[0] for c in rec.calls] == ["noisy_latents", "denoising_loss"] * 2
        assert [c[2] for c in rec.calls] == [whole[0:16].seeds(16)] * 2 + [whole[16:19].seeds(3)] * 2
        assert whole[0:16].seeds(16) + whole[16:19].seeds(3) == whole.seeds(19)
        assert [c[1][0] for c in rec.calls] == [16, 16, 3, 3] and all(c[3] == 7 for c in rec.calls)
        lv = noise_levels(sch, ts)
        assert rec.calls[0][4] == lv[:16] and rec.calls[3][4] == lv[16:]
        assert gen.draw == 8 and rec.calls[0][5] is None and rec.calls[1][6] is None
        assert out.mse.tolist() == [float(i) for i in range(19)] and out.timesteps == ts


def test_offset_noise_takes_a_draw_of_its_own(rec):
    sch = DDPMScheduler()
    x0 = torch.ones(2, 4, 3, 5, 7)
    gen = PhiloxGenerator(1)
    DenoisingLoss(None, sch, noise_offset=0.1, forward=forward).evaluate(x0, torch.zeros(1, 3, 8), 500, gen)
    assert gen.draw == 2
    assert rec.calls[0][5] == (0.1, 1, 35) and rec.calls[1][6] == (0.1, 1, 35) and rec.calls[0][3] == 0


def test_loss_is_the_float64_mean_of_mse_times_weights(rec):
    sch = DDPMScheduler()
    x0 = torch.tensor([0.1, 0.7, 3.0]).reshape(3, 1, 1, 1, 1).expand(3, 4, 1, 2, 2).contiguous()
    ts = [0, 500, 999]
    for kind in ("epsilon", "v_prediction"):
        out = DenoisingLoss(None, sch, snr_gamma=5.0, prediction_type=kind, forward=forward).evaluate(x0, torch.zeros(3, 3, 8), ts,
                                                                                                         PhiloxGenerator(3))
        w = min_snr_weights(snr(sch, ts), 5.0, kind)
        assert out.mse.dtype == torch.float32 and out.weights.dtype == torch.float64 and torch.equal(out.weights, w)
        assert out.loss == float((out.mse.double() * w).mean())
    plain = DenoisingLoss(None, sch, forward=forward).evaluate(x0, torch.zeros(3, 3, 8), ts, PhiloxGenerator(3))
    assert torch.equal(plain.weights, torch.ones(3, dtype=torch.float64)) and plain.loss == float(plain.mse.double().mean())


def test_sweep_is_the_evaluate_columns(rec):
    sch = DDPMScheduler()
    x0 = torch.tensor([2.0, 5.0]).reshape(2, 1, 1, 1, 1).expand(2, 4, 1, 2, 2).contiguous()
    curve = DenoisingLoss(None, sch, forward=forward).sweep(x0, torch.zeros(2, 3, 8), timesteps=(900, 500, 100), draws=2,
                                                            generator=PhiloxGenerator(9))
    assert curve.shape == (2, 3) and curve.dtype == torch.float64
    draws = [c[3] for c in rec.calls if c[0] == "noisy_latents"]
    assert draws == [0, 1, 2, 3, 4, 5]                                     # one draw number per (timestep, draw)
    assert [c[4][0] for c in rec.calls if c[0] == "noisy_latents"] == [l for l in noise_levels(sch, (900, 500, 100)) for _ in range(2)]


def test_refusals():
    sch = DDPMScheduler()
    x0 = torch.zeros(2, 4, 1, 2, 2)
    scorer = DenoisingLoss(None, sch, forward=forward)
    with pytest.raises(TypeError, match="PhiloxGenerator.*torch.Generator"):
        scorer.evaluate(x0, torch.zeros(2, 3, 8), 5, torch.Generator().manual_seed(0))
    with pytest.raises(TypeError, match="PhiloxGenerator"):
        scorer.evaluate(x0, torch.zeros(2, 3, 8), 5, None)
    with pytest.raises(ValueError, match="3 timesteps for 2"):
        scorer.evaluate(x0, torch.zeros(2, 3, 8), [1, 2, 3], PhiloxGenerator(0))
    with pytest.raises(ValueError, match="3 seeds for 2"):
        scorer.evaluate(x0, torch.zeros(2, 3, 8), 5, PhiloxGenerator([1, 2, 3]))
    with pytest.raises(ValueError, match="prediction_type"):
        DenoisingLoss(None, sch, prediction_type="velocity", forward=forward)
    with pytest.raises(ValueError, match="snr_gamma"):
        DenoisingLoss(None, sch, snr_gamma=5.0, prediction_type="sample", forward=forward)
    with pytest.raises(ValueError, match="unet or a forward"):
        DenoisingLoss(None, sch)
    assert DenoisingLoss(None, sch, forward=forward).kind == "epsilon"     # the scheduler's


def test_pipeline_refuses_sampling_only_options():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    pipe = VideoGenPipeline.__new__(VideoGenPipeline)
    lat, pe = torch.zeros(1, 4, 1, 2, 2), torch.zeros(1, 3, 8)
    for name, what in (("window_length", "frame windows"), ("known_latents", "known latents"), ("pag_scale", "perturbed-attention"),
                       ("cache_interval", "layer cache"), ("free_init", "FreeInit")):
        with pytest.raises(ValueError, match=f"`{name}`.*{what}.*sampling run"):
            pipe.denoising_loss(latents=lat, prompt_embeds=pe, timesteps=5, **{name: 2})
    with pytest.raises(TypeError, match="unexpected keyword argument 'colour'"):
        pipe.denoising_loss(latents=lat, prompt_embeds=pe, timesteps=5, colour=1)
    with pytest.raises(ValueError, match="exactly one of `video` and `latents`"):
        pipe.denoising_loss(prompt_embeds=pe, timesteps=5)
    with pytest.raises(ValueError, match="exactly one of `prompt`"):
        pipe.denoising_loss(latents=lat, timesteps=5)
    with pytest.raises(ValueError, match="`timesteps` is required"):
        pipe.denoising_loss(latents=lat, prompt_embeds=pe)


def test_package_exports_and_binding():
    import lavie_amd
    assert lavie_amd.DenoisingLoss is DenoisingLoss and lavie_amd.snr is snr and lavie_amd.min_snr_weights is min_snr_weights
    lib = _lib.load()
    assert lib.lavie_denoising_loss_workspace_floats(3, 2048) == 3 and lib.lavie_denoising_loss_workspace_floats(3, 2049) == 6
    assert lib.lavie_denoising_loss_workspace_floats(0, 8) == -1 and lib.lavie_denoising_loss_workspace_floats(1, 0) == -1
    assert ops.LOSS_KINDS == {"epsilon": 0, "v_prediction": 1, "sample": 2}


def test_c_entries_refuse_by_name_before_any_launch():
    """Every refusal comes from the argument checks, which touch no device: the pointers are never dereferenced on the device side."""
    lib = _lib.load()

    def refused(rc, text):
        return rc != 0 and text in lib.lavie_last_error().decode()

    seeds = (ctypes.c_ulonglong * 2)(5, 6)
    lv_a, lv_s = (ctypes.c_float * 2)(0.5, 0.5), (ctypes.c_float * 2)(0.5, 0.5)

    def args(**over):
        a = _lib.DenoiseArgsC()
        a.struct_size, a.x0_dtype, a.x0, a.a_host, a.s_host = ctypes.sizeof(_lib.DenoiseArgsC), 1, 4096, lv_a, lv_s
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def key(**over):
        k = _lib.NoiseKeyC()
        k.struct_size, k.count, k.seeds_host, k.per, k.draw = ctypes.sizeof(_lib.NoiseKeyC), 2, seeds, 24, 0
        for name, v in over.items():
            setattr(k, name, v)
        return k

    out = ctypes.c_void_p(8192)
    noisy = lambda a, k, o=out: lib.lavie_noisy_latents_seeded(ctypes.byref(a) if a else None, ctypes.byref(k) if k else None, o, None)
    assert refused(noisy(None, key()), "args is null")
    assert refused(noisy(args(struct_size=8), key()), "struct_size")
    assert refused(noisy(args(), None), "key is null")
    assert refused(noisy(args(), key(count=17)), "count=17")
    assert refused(noisy(args(), key(per=0)), "per=0")
    assert refused(noisy(args(x0_dtype=2), key()), "x0_dtype=2")
    assert refused(noisy(args(x0=None), key()), "x0 is null")
    assert refused(noisy(args(x0=4098), key()), "not aligned")
    assert refused(noisy(args(a_host=None), key()), "a_host is null")
    assert refused(noisy(args(s_host=None), key()), "s_host is null")
    assert refused(noisy(args(offset_hw=5, offset_coef=0.1), key()), "offset_hw=5")
    assert refused(noisy(args(offset_hw=-1), key()), "offset_hw=-1")
    assert refused(noisy(args(offset_hw=8, offset_coef=float("nan")), key()), "offset_coef")
    bad = (ctypes.c_float * 2)(0.5, float("inf"))
    assert refused(noisy(args(s_host=bad), key()), "level 1")
    assert refused(noisy(args(), key(), None), "model_in is null")
    assert refused(noisy(args(), key(), ctypes.c_void_p(8193)), "2-byte")

    def loss(a=None, k=None, pred=8192, kind=0, o=16384, ws=32768, n=2):
        return lib.lavie_denoising_loss_f32(ctypes.byref(a or args()), ctypes.byref(k or key()), pred, kind, o, ws, n, None)
    assert refused(loss(pred=None), "pred is null")
    assert refused(loss(kind=3), "kind=3")
    assert refused(loss(o=None), "out is null")
    assert refused(loss(ws=None), "workspace is null")
    assert refused(loss(n=1), "workspace_floats=1")
    assert refused(loss(a=args(offset_hw=7, offset_coef=0.1)), "offset_hw=7")
    assert refused(loss(k=key(count=0)), "count=0")
