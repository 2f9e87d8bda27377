"""Sampling long clips as overlapping frame windows, the host side (no GPU): the window schedules and weight profiles, every
refusal of lavie_window_step with pointers that are never dereferenced, and the pipelines' own refusals."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from lavie_amd import _lib
from lavie_amd.windows import check_schedule, cover_counts, window_profile, window_starts


@pytest.mark.parametrize("total,length,stride,want", [(13, 8, 6, [0, 5]), (16, 8, 8, [0, 8]), (10, 6, 2, [0, 2, 4]), (8, 8, 3, [0]),
                                                      (9, 3, 3, [0, 3, 6]), (64, 16, 12, [0, 12, 24, 36, 48])])
def test_window_starts(total, length, stride, want):
    starts = window_starts(total, length, stride)
    assert starts == want
    assert starts[-1] + length == total and min(cover_counts(total, length, starts)) >= 1


def test_vsr_schedule_covers_every_frame_at_most_twice():
    starts = window_starts(61, 8, 6)
    counts = cover_counts(61, 8, starts)
    assert starts[0] == 0 and starts[-1] == 53 and len(starts) == 10
    assert min(counts) >= 1 and max(counts) <= 2


def test_schedules_outside_the_kernels_limits_raise():
    with pytest.raises(ValueError, match="at most 4"):
        window_starts(16, 8, 1)                                   # stride 1 puts frame 7 under windows 0..7
    with pytest.raises(ValueError, match="covered by"):
        window_starts(40, 10, 2)
    assert max(cover_counts(16, 8, window_starts(16, 8, 2))) == 4  # the largest cover count the kernel takes
    with pytest.raises(ValueError, match="uncovered"):
        window_starts(20, 4, 5)
    with pytest.raises(ValueError, match="stride"):
        window_starts(20, 4, 0)
    with pytest.raises(ValueError, match="length"):
        window_starts(4, 8, 2)
    with pytest.raises(ValueError, match="length"):
        window_starts(200, 65, 60)
    with pytest.raises(ValueError, match="windows"):
        window_starts(200, 4, 4)                                   # 50 windows
    with pytest.raises(ValueError, match="no window"):
        check_schedule(10, 4, [0, 6])
    with pytest.raises(ValueError, match="ascending"):
        check_schedule(10, 4, [3, 3, 6])
    with pytest.raises(ValueError, match="ascending"):
        check_schedule(10, 4, [0, 4, 7])


@pytest.mark.parametrize("length", [1, 2, 3, 8, 16, 64])
def test_profiles_are_positive_and_symmetric(length):
    for kind in ("uniform", "triangle"):
        prof = window_profile(length, kind)
        assert len(prof) == length and all(v > 0 for v in prof) and prof == prof[::-1]
    assert window_profile(length, "uniform") == [1.0] * length
    assert window_profile(length, "triangle") == [float(min(i + 1, length - i)) for i in range(length)]
    with pytest.raises(ValueError, match="window_weights"):
        window_profile(length, "gauss")


def test_abi_version_is_unchanged():
    assert _lib.load().lavie_abi_version() == 8 == _lib.ABI_VERSION


# ------------------------------------------------------------------ the C entry point's refusals
P, C, F, L, HW = 1, 2, 13, 8, 8
BASE = 1 << 20             # fake device addresses, 1 MiB apart: never dereferenced, every refusal comes before a HIP call


def make_args(**over):
    """A valid lavie_window_step_args over fake pointers (starts [0, 5] on 13 frames), with fields overridden.  Returns the struct
    and the arrays it borrows."""
    starts = over.pop("starts", [0, 5])
    profile = over.pop("profile", [1, 2, 3, 4, 4, 3, 2, 1])
    eps = over.pop("eps", [BASE * (3 + w) for w in range(len(starts))])
    model_in = over.pop("model_in", [BASE * (40 + w) for w in range(len(starts))])
    a = _lib.WindowStepArgsC()
    a.struct_size = ctypes.sizeof(_lib.WindowStepArgsC)
    a.family, a.cfg, a.P, a.C, a.F, a.hw, a.W, a.L = 0, 1, P, C, F, HW, len(starts), len(profile)
    keep = [(ctypes.c_int * len(starts))(*starts), (ctypes.c_float * len(profile))(*profile),
            (ctypes.c_void_p * len(eps))(*eps), (ctypes.c_void_p * len(model_in))(*model_in)]
    a.starts_host, a.profile_host, a.eps_host, a.model_in_host = keep
    a.x, a.aux = BASE, 2 * BASE
    a.guidance, a.k_x, a.k_eps, a.c_x0, a.c_xt, a.c4, a.next_input_scale = 7.5, 1.0, 0.5, 0.3, 0.7, 0.1, 0.9
    for k, v in over.items():
        setattr(a, k, v)
    return a, keep


def test_window_step_refusals_name_their_argument():
    """Fails on a library without the feature: the symbol does not exist there."""
    lib = _lib.load()

    def refused(word, **over):
        a, keep = make_args(**over)
        rc = lib.lavie_window_step(ctypes.byref(a), None)
        msg = lib.lavie_last_error().decode()
        assert rc != 0 and word in msg, (over, rc, msg)

    assert lib.lavie_window_step(None, None) != 0 and b"args" in lib.lavie_last_error()
    refused("struct_size", struct_size=ctypes.sizeof(_lib.WindowStepArgsC) - 4)
    refused("struct_size", struct_size=0)
    refused("family", family=2)
    refused("P=0", P=0)
    refused("C=-1", C=-1)
    refused("hw=0", hw=0)
    refused("planes", P=4000)
    refused("W=0", W=0)
    refused("W=33", W=33)
    refused("L=0", L=0)
    refused("L=65", L=65)
    for table in ("starts_host", "profile_host", "eps_host", "model_in_host"):
        refused(table, **{table: None})
    refused("ascending", starts=[5, 0])
    refused("ascending", starts=[0, 0])
    refused("starts[0]", starts=[-1, 5])
    refused("past F", starts=[0, 6])
    refused("past F", F=12)
    refused("frame 4 is uncovered", L=4)
    refused("cover count of 5", starts=[0, 1, 2, 3, 4], F=12)
    refused("profile[3]", profile=[1, 2, 3, 0, 4, 3, 2, 1])
    refused("profile[3]", profile=[1, 2, 3, -2, 4, 3, 2, 1])
    refused("profile[7]", profile=[1, 2, 3, 4, 4, 3, 2, float("nan")])
    refused("profile[0]", profile=[float("inf"), 2, 3, 4, 4, 3, 2, 1])
    refused("eps[1] is null", eps=[3 * BASE, None])
    refused("model_in[0] is null", model_in=[None, 41 * BASE])
    refused("x is null", x=None)
    refused("aux is null", aux=None)
    refused("aux is null", aux=None, family=1, c4=0.0)            # the multistep family always writes its history
    refused("x and aux overlap", aux=BASE)
    refused("x and aux overlap", aux=BASE + 64)
    refused("model_in[0] and model_in[1] overlap", model_in=[40 * BASE, 40 * BASE + 32])
    refused("eps[0] and model_in[1] overlap", model_in=[40 * BASE, 3 * BASE])
    refused("x and model_in[0] overlap", model_in=[BASE, 41 * BASE])
    refused("aux and eps[1] overlap", eps=[3 * BASE, 2 * BASE])
    for name in ("guidance", "k_x", "k_eps", "c_x0", "c_xt", "c4", "next_input_scale"):
        refused(name, **{name: float("nan")})
        refused("not finite", **{name: float("inf")})
    refused("x at", x=BASE + 4)
    refused("aux at", aux=2 * BASE + 8)
    refused("eps[0] at", eps=[3 * BASE + 2, 4 * BASE])
    refused("model_in[1] at", model_in=[40 * BASE, 41 * BASE + 6])


# ------------------------------------------------------------------ the pipelines
def test_pipelines_refuse_windows_combined_with_known_latents():
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    from lavie_amd.scheduling_ddim import DDIMScheduler
    unet = SimpleNamespace(config=SimpleNamespace(sample_size=8, in_channels=4), device="cpu")
    pipe = VideoGenPipeline(unet=unet, scheduler=DDIMScheduler())
    shape = (1, 4, 12, 4, 6)
    known, mask = torch.zeros(shape), torch.ones(1, 1, 12, 4, 6)
    with pytest.raises(ValueError, match="window"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 7.5, known=known, mask=mask, window_length=8)
    with pytest.raises(ValueError, match="window"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 7.5, start_step=1, window_length=8)
    with pytest.raises(ValueError, match="window_length"):
        pipe.denoise(torch.zeros(shape), torch.zeros(2, 77, 8), 4, 7.5, window_length=0)
    kw = dict(prompt_embeds=torch.zeros(1, 77, 8), negative_prompt_embeds=torch.zeros(1, 77, 8), height=32, width=48,
              video_length=12, num_inference_steps=2, output_type="latent", window_length=8)
    with pytest.raises(ValueError, match="window"):
        pipe(known_latents=known, known_mask=mask, **kw)
    with pytest.raises(ValueError, match="window"):
        pipe(video=torch.zeros(1, 12, 32, 48, 3, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="window"):
        pipe(known_latents=known, strength=0.5, **kw)


def test_long_video_methods_and_chunk_overlap_arguments():
    """text_to_long_video(method="windows") is one pipeline call over the whole length; upscale_in_chunks(overlap=) one windowed
    call; both validate their arguments; the defaults keep the old paths."""
    from lavie_amd.cascade import text_to_long_video
    from lavie_amd.vsr.pipeline import upscale_in_chunks
    calls = []

    def pipe(**kw):
        calls.append(kw)
        return SimpleNamespace(video=torch.zeros(1, 4, kw["video_length"], 4, 6))

    out = text_to_long_video(pipe, None, 3, overlap=4, method="windows", prompt_embeds=torch.zeros(1, 77, 8), video_length=16)
    assert out.shape[2] == 40 and len(calls) == 1
    assert calls[0]["window_length"] == 16 and calls[0]["window_stride"] == 12 and calls[0]["output_type"] == "latent"
    with pytest.raises(ValueError, match="method"):
        text_to_long_video(pipe, None, 3, method="ring", prompt_embeds=torch.zeros(1, 77, 8))
    with pytest.raises(ValueError, match="overlap"):
        text_to_long_video(pipe, None, 3, overlap=16, method="windows", prompt_embeds=torch.zeros(1, 77, 8))

    seen = []

    def vsr(image=None, **kw):
        seen.append((image.shape[2], kw))
        return SimpleNamespace(images=torch.zeros(1, 4, image.shape[2], 4, 6))

    frames = torch.zeros(1, 3, 20, 4, 6)
    assert upscale_in_chunks(vsr, frames, short_seq=8, overlap=2, noise_level=20).shape[2] == 20
    assert seen == [(20, dict(window_length=8, window_stride=6, noise_level=20))]
    del seen[:]
    assert upscale_in_chunks(vsr, frames, short_seq=8, noise_level=20).shape[2] == 20
    assert seen == [(8, dict(noise_level=20)), (8, dict(noise_level=20)), (4, dict(noise_level=20))]       # today's chunks
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="overlap"):
            upscale_in_chunks(vsr, frames, short_seq=8, overlap=bad)
