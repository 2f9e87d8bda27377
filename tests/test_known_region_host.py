"""Sampling around known latents, the host side (no GPU): the schedulers' noise levels, the strength arithmetic, the frame
bookkeeping of the clip continuation with a stub pipeline, and every refusal of the pipeline's validation."""
import math
from types import SimpleNamespace

import pytest
import torch

from lavie_amd.pipeline_videogen import VideoGenPipeline
from lavie_amd.scheduling_ddim import DDIMScheduler
from lavie_amd.scheduling_ddpm import DDPMScheduler
from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
from lavie_amd.scheduling_euler_discrete import EulerDiscreteScheduler


@pytest.mark.parametrize("cls", [DDPMScheduler, DDIMScheduler, DPMSolverMultistepScheduler])
def test_noise_level_is_the_closed_form_of_the_schedulers_own_table(cls):
    sch = cls()
    sch.set_timesteps(8)
    for t in [int(v) for v in sch.timesteps]:
        a, s = sch.noise_level(t)
        ab = float(sch.alphas_cumprod[t].double())
        assert a == pytest.approx(math.sqrt(ab), rel=1e-12) and s == pytest.approx(math.sqrt(1.0 - ab), rel=1e-12)
        assert a * a + s * s == pytest.approx(1.0, abs=1e-12)
        # x_t = a x_0 + s noise is the scheduler's own add_noise where it has one
        if hasattr(sch, "add_noise"):
            x0, z = torch.randn(2, 3), torch.randn(2, 3)
            assert torch.allclose(sch.add_noise(x0, z, torch.tensor([t, t])), a * x0 + s * z, atol=1e-6)
    assert sch.noise_level(None) == (1.0, 0.0) and sch.noise_level() == (1.0, 0.0)


def test_euler_noise_level_is_one_and_sigma():
    sch = EulerDiscreteScheduler()
    sch.set_timesteps(6)
    ab = sch.alphas_cumprod.double()
    train = ((1 - ab) / ab).sqrt().numpy()
    for i, t in enumerate([float(v) for v in sch.timesteps]):
        a, s = sch.noise_level(t)
        lo = int(math.floor(t))
        want = train[lo] + (t - lo) * (train[min(lo + 1, 999)] - train[lo])        # linear interpolation at a fractional timestep
        assert a == 1.0 and s == pytest.approx(want, rel=1e-5) and s == pytest.approx(float(sch.sigmas[i]), rel=1e-6)
    assert sch.noise_level(float(sch.timesteps[0]))[1] == pytest.approx(sch.init_noise_sigma)
    assert sch.noise_level(None) == (1.0, 0.0)


@pytest.mark.parametrize("steps", [1, 4, 50])
def test_strength_to_start_step(steps):
    start = VideoGenPipeline.strength_start
    assert start(steps, 1.0) == 0
    for strength in (0.9, 0.5, 0.26, 0.02):
        want = min(steps - int(steps * strength), steps - 1)          # img2img's rule; one step always runs
        assert start(steps, strength) == want
        assert 0 <= start(steps, strength) < steps
    assert start(4, 0.5) == 2 and start(50, 0.5) == 25 and start(50, 0.3) == 35 and start(1, 0.5) == 0
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="strength"):
            start(steps, bad)


class StubPipe:
    """Returns latents whose value is the call number, with the pinned frames copied from known_latents, and records its calls."""
    vae_scale_factor = 8

    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        self.calls.append(kw)
        p = kw["prompt_embeds"].shape[0]
        out = torch.full((p, 4, kw["video_length"], kw["height"] // 8, kw["width"] // 8), float(len(self.calls)))
        if kw.get("known_latents") is not None:
            m = kw["known_mask"].expand_as(out).bool()
            out[m] = kw["known_latents"][m]
        return SimpleNamespace(video=out)


@pytest.mark.parametrize("num_clips,overlap,length", [(1, 4, 16), (3, 4, 16), (4, 1, 16), (2, 7, 8)])
def test_text_to_long_video_frame_bookkeeping(num_clips, overlap, length):
    from lavie_amd.cascade import text_to_long_video
    pipe = StubPipe()
    out = text_to_long_video(pipe, None, num_clips, overlap=overlap, prompt_embeds=torch.zeros(2, 77, 8), height=32, width=48,
                             video_length=length, num_inference_steps=3)
    assert out.shape == (2, 4, length + (num_clips - 1) * (length - overlap), 4, 6)
    assert len(pipe.calls) == num_clips and "known_latents" not in pipe.calls[0]
    # clip k fills frames [k (L - overlap), k (L - overlap) + L): its value is k + 1 except on the overlap, which is stored once
    # and belongs to the clip before it
    for k in range(num_clips):
        lo = k * (length - overlap)
        assert (out[:, :, lo + (overlap if k else 0):lo + length] == k + 1).all()
    for k, call in enumerate(pipe.calls[1:], start=1):
        mask, known = call["known_mask"], call["known_latents"]
        assert mask.shape == (2, 1, length, 4, 6) and known.shape == (2, 4, length, 4, 6)
        assert (mask[:, :, :overlap] == 1).all() and (mask[:, :, overlap:] == 0).all()
        assert (known[:, :, :overlap] == k).all()                      # the tail of the clip before
        assert call["output_type"] == "latent" and call["num_inference_steps"] == 3 and call["height"] == 32


def test_continue_clip_refuses_a_bad_overlap():
    from lavie_amd.cascade import continue_clip
    prev = torch.zeros(1, 4, 16, 4, 4)
    for overlap in (0, 16, 17):
        with pytest.raises(ValueError, match="overlap"):
            continue_clip(StubPipe(), prev, overlap=overlap, prompt_embeds=torch.zeros(1, 77, 8))
    with pytest.raises(ValueError, match="overlap"):
        continue_clip(StubPipe(), prev[:, :, :2], overlap=3, prompt_embeds=torch.zeros(1, 77, 8))
    out = continue_clip(StubPipe(), prev, overlap=4, prompt_embeds=torch.zeros(1, 77, 8))
    assert out.shape == (1, 4, 16, 4, 4)                                # height / width default to those of the previous clip


def test_pipeline_validation_refuses_each_bad_argument():
    pipe = VideoGenPipeline(unet=SimpleNamespace(), scheduler=DDIMScheduler())
    shape = (2, 4, 8, 4, 6)
    known, mask = torch.zeros(shape), torch.ones(2, 1, 8, 4, 6)
    check = pipe.check_known_inputs
    check(None, None, None, 1.0, shape)                                  # the plain call
    check(known, mask, None, 0.5, shape)
    check(known, torch.ones(1, 1, 8, 1, 1), None, 1.0, shape)            # a per-frame mask broadcasts
    for strength in (0.0, 1.01, -1.0, None):
        with pytest.raises(ValueError, match="strength"):
            check(known, mask, None, strength, shape)
    with pytest.raises(ValueError, match="strength"):                    # nothing to start from
        check(None, None, None, 0.5, shape)
    with pytest.raises(ValueError, match="known_mask"):                  # a mask needs known latents
        check(None, mask, None, 1.0, shape)
    with pytest.raises(ValueError, match="both"):                        # video xor known_latents
        check(known, None, torch.zeros(2, 8, 32, 48, 3, dtype=torch.uint8), 1.0, shape)
    with pytest.raises(ValueError, match="known_latents"):
        check(torch.zeros(2, 4, 8, 4, 5), None, None, 1.0, shape)
    for bad in (torch.ones(2, 4, 8, 4, 6), torch.ones(2, 1, 7, 4, 6), torch.ones(8, 4, 6), torch.ones(3, 1, 8, 4, 6)):
        with pytest.raises(ValueError, match="known_mask"):
            check(known, bad, None, 1.0, shape)
    for bad in (mask * 1.5, mask - 1.25, mask * float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            check(known, bad, None, 1.0, shape)
    with pytest.raises(ValueError, match="video"):                       # pixel shapes: uint8 channels-last or float channels-first
        check(None, None, torch.zeros(2, 3, 8, 32, 48, dtype=torch.uint8), 1.0, shape)
    with pytest.raises(ValueError, match="video"):
        check(None, None, torch.zeros(2, 8, 32, 48, 3), 1.0, shape)
    with pytest.raises(ValueError, match="video"):
        check(None, None, torch.zeros(2, 3, 8, 32, 40), 1.0, shape)
    with pytest.raises(ValueError, match="vae"):                         # a video needs the VAE to encode it
        check(None, None, torch.zeros(2, 3, 8, 32, 48), 1.0, shape)
    # denoise itself: the known-latents arguments need `known`
    with pytest.raises(ValueError, match="known"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 1.0, mask=mask)
    with pytest.raises(ValueError, match="known"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 1.0, start_step=2)


def test_encode_video_takes_both_pixel_layouts():
    """uint8 [P, F, H, W, 3] and float [P, 3, F, H, W] in [-1, 1] reach the VAE as the same frames; the result is the posterior
    mode times 0.18215 in [P, 4, F, h, w]."""
    seen = []

    class Vae(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def encode(self, x):
            seen.append(x)
            lat = x[:, :1, ::8, ::8].repeat(1, 4, 1, 1)
            return SimpleNamespace(latent_dist=SimpleNamespace(mode=lambda: lat))

    pipe = VideoGenPipeline(unet=SimpleNamespace(), vae=Vae(), scheduler=DDIMScheduler())
    pix = torch.randint(0, 256, (2, 10, 16, 24, 3), dtype=torch.uint8)
    a = pipe.encode_video(pix)
    b = pipe.encode_video(pix.permute(0, 4, 1, 2, 3).float() / 127.5 - 1.0)
    assert a.shape == (2, 4, 10, 2, 3) and a.dtype == torch.float32 and torch.equal(a, b)
    assert [t.shape[0] for t in seen] == [8, 8, 4, 8, 8, 4]              # 20 frames in chunks of 8
    want = (pix[:, :, ::8, ::8, 0].float() / 127.5 - 1.0) * 0.18215
    assert torch.allclose(a[:, 0], want)
