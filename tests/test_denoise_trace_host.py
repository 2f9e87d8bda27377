"""The launch trace of both pipelines' denoising loops, case by case, against tests/golden/denoise_traces.json (recorded with this
file's recorder on the commit in front of "one denoising loop under both pipelines"; `PYTHONPATH=. python
tests/test_denoise_trace_host.py` rewrites it from the tree it runs in).  CPU tensors, stub UNets, recording stand-ins for the
device ops at the `ops` level: every fill, blend, UNet call, guidance table, step wrapper, windowed step, frequency mix, engine /
PAG / layer-cache / LoRA switch and callback of a call, in order, then the next draw of the call's generator; for a refused call
the exception's type and full text.  Only the public surface is used (`pipe(...)`, `pipe.denoise(...)`, `upscale_in_chunks`), so a
refactor of the loops cannot change what reaches the device, the order of random draws, or which of two refusals wins."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from lavie_amd import ops, sampling
from lavie_amd.free_init import FreeInit
from lavie_amd.pipeline_videogen import VideoGenPipeline
from lavie_amd.scheduling_ddim import DDIMScheduler
from lavie_amd.scheduling_ddpm import DDPMScheduler
from lavie_amd.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
from lavie_amd.scheduling_euler_discrete import EulerDiscreteScheduler
from lavie_amd.vsr.pipeline import VideoUpscalePipeline, upscale_in_chunks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_traces.json")
SCHEDULERS = {"ddpm": DDPMScheduler, "dpm": DPMSolverMultistepScheduler, "ddim": DDIMScheduler, "euler": EulerDiscreteScheduler}
STEP_KIND = {name: kind for (_, kind, _), name in sampling.STEP_WRAPPERS.items()}


def shape(t):
    return None if t is None else list(t.shape)


def rnd(v, places=9):
    return round(float(v), places)


class RecordingUNet:
    """A UNet-shaped callable with every optional method a loop may use; each call is one event."""
    device = "cpu"

    def __init__(self, events, in_channels=4):
        self.events = events
        self.config = SimpleNamespace(sample_size=8, in_channels=in_channels)
        self.pag, self.layer_cache, self.lora_scale = ((), 0), 0, 1.0

    def __call__(self, x, t, *more, encoder_hidden_states=None, **kw):
        kw = {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in sorted(kw.items())}
        self.events.append(["unet", shape(x), rnd(t, 4), [shape(m) for m in more], shape(encoder_hidden_states), kw])
        return SimpleNamespace(sample=torch.zeros_like(x))

    def prepare(self, *a):
        self.events.append(["prepare"] + list(a))

    def cache_context(self, ctx):
        self.events.append(["cache_context", shape(ctx)])
        return ctx

    def set_cfg_shared_input(self, on):
        self.events.append(["set_cfg_shared_input", bool(on)])

    def set_pag(self, layers, perturbed):
        self.events.append(["set_pag", list(layers), int(perturbed)])
        self.pag = (tuple(layers), int(perturbed))

    def enable_layer_cache(self, depth):
        self.events.append(["enable_layer_cache", depth])
        self.layer_cache = depth

    def disable_layer_cache(self):
        self.events.append(["disable_layer_cache"])
        self.layer_cache = 0

    def set_lora_scale(self, scale):
        self.events.append(["set_lora_scale", scale])
        self.lora_scale = scale


def install(monkeypatch, events):
    """Recording stand-ins for every device op a loop launches; none of them writes."""
    def fill(name):
        def f(x, m, scale=1.0):
            events.append([name, shape(x), shape(m), rnd(scale, 6)])
        return f

    def known_blend(x, model_in, known, mask, noise_known, level, input_scale=1.0):
        events.append(["known_blend", shape(x), shape(model_in), shape(mask), [rnd(v) for v in level], rnd(input_scale, 6)])

    def guidance_table(eps, latents, guidance, rescale, workspace=None, out=None, moments_out=None):
        g = [rnd(v, 6) for v in guidance.tolist()] if isinstance(guidance, torch.Tensor) else rnd(guidance, 6)
        events.append(["guidance_table", [shape(e) for e in eps] if isinstance(eps, list) else shape(eps), latents, g, rnd(rescale, 6),
                       workspace is not None, shape(out)])
        return out

    def step_wrapper(name):
        kind = STEP_KIND[name]
        count = {"none": 0, "scalar": 1, "table": 1, "pag": 1, "pag_cfg": 2}[kind]

        def f(eps, x, aux, model_in, *rest):
            guidance, (coeffs, next_scale), region = rest[:count], rest[count:count + 2], rest[count + 2:]
            scalar = rnd(guidance[0], 6) if kind in ("scalar", "pag_cfg") else shape(guidance[0]) if kind == "table" else None
            pag_scale = rnd(guidance[-1], 6) if kind in ("pag", "pag_cfg") else None
            pinned = [shape(region[1]), [rnd(v) for v in region[3]]] if region else None
            events.append([name, shape(eps), shape(model_in), aux is not None, [rnd(c) for c in coeffs], rnd(next_scale, 6), scalar,
                           pinned, pag_scale])
        return f

    def window_step(name):
        def f(eps, x, aux, model_in, starts, profile, guidance, coeffs, next_input_scale=1.0, multistep=False):
            g = shape(guidance) if isinstance(guidance, torch.Tensor) else None if guidance is None else rnd(guidance, 6)
            events.append([name, [shape(e) for e in eps], shape(x), aux is not None, list(starts), [rnd(v, 6) for v in profile], g,
                           [rnd(c) for c in coeffs], rnd(next_input_scale, 6), bool(multistep)])
        return f

    def freq_mix(x0, e0, z, filt, a, s, r, out=None, model_in=None, input_scale=1.0, workspace=None):
        events.append(["freq_mix", shape(model_in), rnd(a), rnd(s), rnd(r), rnd(input_scale, 6), out is x0, workspace is not None,
                       rnd(z.double().sum(), 3), rnd(e0.double().sum(), 3)])

    monkeypatch.setattr(ops, "latents_to_model_input", fill("latents_to_model_input"))
    monkeypatch.setattr(ops, "latents_to_model_input1", fill("latents_to_model_input1"))
    monkeypatch.setattr(ops, "known_blend", known_blend)
    monkeypatch.setattr(ops, "guidance_table", guidance_table)
    monkeypatch.setattr(ops, "freq_mix", freq_mix)
    for name in set(sampling.STEP_WRAPPERS.values()):
        monkeypatch.setattr(ops, name, step_wrapper(name))
    for name in ("window_step", "window_step_scaled"):
        monkeypatch.setattr(ops, name, window_step(name))


def seeded(seed):
    return torch.Generator().manual_seed(seed)


def base_denoise(scheduler, p=1, frames=4, steps=3, guidance_scale=7.5, parts=None, generator="one", free_init_on_pipe=None, **kw):
    """VideoGenPipeline.denoise on [p, 4, frames, 4, 6]; `parts`: the context's parts per latent when guidance alone does not say."""
    def run(events):
        pipe = VideoGenPipeline(unet=RecordingUNet(events), scheduler=SCHEDULERS[scheduler]())
        if free_init_on_pipe:
            pipe.enable_free_init(**free_init_on_pipe)
        lat = torch.randn(p, 4, frames, 4, 6, generator=seeded(3))
        guided = not isinstance(guidance_scale, float) or guidance_scale > 1.0
        rows = p * (parts if parts is not None else (2 if guided else 1) + (1 if kw.get("pag_scale", 0.0) > 0 else 0))
        gens = [seeded(11 + j) for j in range(p + (generator == "long_list"))] if "list" in generator else [seeded(11)]
        made = {k: (v(lat) if callable(v) else v) for k, v in kw.items()}
        try:
            pipe.denoise(lat, torch.zeros(rows, 77, 8, dtype=torch.float16), steps, guidance_scale,
                         generator=gens if "list" in generator else gens[0],
                         callback=lambda i, t, x: events.append(["callback", i, rnd(t, 4)]), **made)
        finally:
            events.append(["next_draw"] + [[rnd(v, 4) for v in torch.randn(2, generator=g).tolist()] for g in gens])
    return run


def base_call(scheduler, p=1, frames=4, steps=3, free_init_on_pipe=None, **kw):
    """VideoGenPipeline.__call__ with embeddings, 32 x 48 pixels (latents [p, 4, frames, 4, 6]), latent output; a keyword the
    call below sets itself (height, callback_steps, prompt_embeds, ...) replaces that one."""
    def run(events):
        pipe = VideoGenPipeline(unet=RecordingUNet(events), scheduler=SCHEDULERS[scheduler]())
        if free_init_on_pipe:
            pipe.enable_free_init(**free_init_on_pipe)
        g, e = seeded(11), seeded(5)
        made = {k: (v((p, 4, frames, 4, 6)) if callable(v) else v) for k, v in kw.items()}
        args = dict(prompt_embeds=torch.randn(p, 77, 8, generator=e), negative_prompt_embeds=torch.randn(p, 77, 8, generator=e),
                    height=32, width=48, video_length=frames, num_inference_steps=steps, output_type="latent", generator=g,
                    callback=lambda i, t, x: events.append(["callback", i, rnd(t, 4)]))
        args.update(made)
        try:
            pipe(**args)
        finally:
            events.append(["next_draw", [rnd(v, 4) for v in torch.randn(2, generator=g).tolist()]])
    return run


def vsr(scheduler, how="denoise", frames=4, steps=3, **kw):
    """VideoUpscalePipeline on [1, 4, frames, 4, 6] latents / [1, 3, frames, 4, 6] low-res frames: `denoise`, `__call__`, or
    `upscale_in_chunks` with the remaining keywords."""
    def run(events, kw=kw):
        kw = dict(kw)
        pipe = VideoUpscalePipeline(unet=RecordingUNet(events, in_channels=7), scheduler=SCHEDULERS[scheduler]())
        g, e = seeded(11), seeded(5)
        image = torch.randn(1, 3, frames, 4, 6, generator=e)
        emb = dict(prompt_embeds=torch.randn(1, 77, 8, generator=e), negative_prompt_embeds=torch.randn(1, 77, 8, generator=e))
        callback = lambda i, t, x: events.append(["callback", i, rnd(t, 4)])      # noqa: E731
        try:
            if how == "denoise":
                lat = torch.randn(1, 4, frames, 4, 6, generator=seeded(3))
                pipe.denoise(lat, image, torch.zeros(2, 77, 8, dtype=torch.float16), 20, steps, kw.pop("guidance_scale", 9.0),
                             generator=g, callback=callback, **kw)
            elif how == "call":
                pipe(image=image, num_inference_steps=steps, generator=g, callback=callback, **emb, **kw)
            else:
                upscale_in_chunks(pipe, image, num_inference_steps=steps, generator=g, callback=callback, **emb, **kw)
        finally:
            events.append(["next_draw", [rnd(v, 4) for v in torch.randn(2, generator=g).tolist()]])
    return run


def direct_check_pag(*args, **others):
    """VideoGenPipeline.check_pag called on its own: what it returns, or raises."""
    def run(events):
        events.append(["check_pag", bool(VideoGenPipeline.check_pag(*args, **others))])
    return run


def known_of(like):
    """Known latents for latents `like` (a tensor, or its shape)."""
    return torch.randn(tuple(like.shape) if isinstance(like, torch.Tensor) else like, generator=seeded(9))


def mask_of(like):
    """A mask that pins the first frame."""
    shape_ = tuple(like.shape) if isinstance(like, torch.Tensor) else like
    m = torch.zeros(shape_[0], 1, *shape_[2:])
    m[:, :, :1] = 1.0
    return m


WINDOWS = dict(frames=6, window_length=4, window_stride=2)
PAG = dict(pag_scale=3.0)
FREE = dict(num_iters=2)


def cases():
    c = {}
    for s in ("ddpm", "dpm"):
        # ---- VideoGenPipeline.denoise
        c[f"{s}/guided"] = base_denoise(s)
        c[f"{s}/unguided"] = base_denoise(s, guidance_scale=1.0)
        c[f"{s}/guidance_sequence"] = base_denoise(s, p=2, guidance_scale=[5.0, 9.0])
        c[f"{s}/guidance_rescale"] = base_denoise(s, guidance_rescale=0.7)
        c[f"{s}/known_mask_start0"] = base_denoise(s, known=known_of, mask=mask_of)
        c[f"{s}/known_mask_start0_unguided"] = base_denoise(s, guidance_scale=1.0, known=known_of, mask=mask_of)
        c[f"{s}/known_mask_given_noise"] = base_denoise(s, known=known_of, mask=mask_of, known_noise=known_of)
        c[f"{s}/known_nomask_start1"] = base_denoise(s, known=known_of, start_step=1)
        c[f"{s}/known_mask_rescale"] = base_denoise(s, known=known_of, mask=mask_of, guidance_rescale=0.7)
        c[f"{s}/call_strength"] = base_call(s, known_latents=known_of, strength=0.5)
        c[f"{s}/call_known_mask"] = base_call(s, known_latents=known_of, known_mask=mask_of)
        c[f"{s}/windows"] = base_denoise(s, **WINDOWS)
        c[f"{s}/windows_unguided"] = base_denoise(s, guidance_scale=1.0, **WINDOWS)
        c[f"{s}/windows_rescale"] = base_denoise(s, guidance_rescale=0.7, **WINDOWS)
        c[f"{s}/windows_default_stride_uniform"] = base_denoise(s, frames=6, window_length=4, window_weights="uniform")
        c[f"{s}/windows_not_in_force"] = base_denoise(s, window_length=4, window_stride=2)
        c[f"{s}/call_windows"] = base_call(s, **WINDOWS)
        c[f"{s}/pag_guided"] = base_denoise(s, **PAG)
        c[f"{s}/pag_unguided"] = base_denoise(s, p=2, guidance_scale=1.0, **PAG)
        c[f"{s}/pag_adaptive"] = base_denoise(s, pag_adaptive_scale=0.004, pag_applied_layers=("mid_block", "up_blocks.1"), **PAG)
        c[f"{s}/call_pag"] = base_call(s, **PAG)
        c[f"{s}/call_pag_unguided"] = base_call(s, p=2, guidance_scale=1.0, **PAG)
        c[f"{s}/cache"] = base_denoise(s, cache_interval=2)
        c[f"{s}/cache_depth2"] = base_denoise(s, cache_interval=2, cache_depth=2)
        c[f"{s}/cache_start1"] = base_denoise(s, cache_interval=2, known=known_of, start_step=1)
        c[f"{s}/cache_windows_not_in_force"] = base_denoise(s, cache_interval=2, window_length=4)
        c[f"{s}/cache_interval1"] = base_denoise(s, cache_interval=1)
        c[f"{s}/call_cache"] = base_call(s, cache_interval=2, cache_depth=2)
        c[f"{s}/freeinit"] = base_denoise(s, free_init=FREE)
        c[f"{s}/freeinit_object_ideal"] = base_denoise(s, free_init=FreeInit(num_iters=2, method="ideal"))
        c[f"{s}/freeinit_fast"] = base_denoise(s, steps=6, free_init=dict(num_iters=2, use_fast_sampling=True))
        c[f"{s}/freeinit_windows"] = base_denoise(s, free_init=FREE, **WINDOWS)
        c[f"{s}/freeinit_cache"] = base_denoise(s, free_init=FREE, cache_interval=2)
        c[f"{s}/freeinit_pag"] = base_denoise(s, free_init=FREE, **PAG)
        c[f"{s}/freeinit_unguided"] = base_denoise(s, guidance_scale=1.0, free_init=FREE)
        c[f"{s}/freeinit_one_iteration"] = base_denoise(s, free_init=dict(num_iters=1))
        c[f"{s}/freeinit_on_pipeline"] = base_denoise(s, free_init_on_pipe=FREE)
        c[f"{s}/call_freeinit"] = base_call(s, free_init=FREE)
        c[f"{s}/call_freeinit_on_pipeline_overridden"] = base_call(s, free_init_on_pipe=dict(num_iters=3), free_init=dict(num_iters=1))
        c[f"{s}/call_lora_scale"] = base_call(s, cross_attention_kwargs={"scale": 0.5})
        c[f"{s}/call_plain"] = base_call(s)
        c[f"{s}/call_unguided"] = base_call(s, guidance_scale=1.0)
        c[f"{s}/call_sequence_rescale"] = base_call(s, p=2, guidance_scale=[5.0, 9.0], guidance_rescale=0.7, num_images_per_prompt=1)
        c[f"{s}/call_rescale_unguided"] = base_call(s, guidance_scale=1.0, guidance_rescale=0.7)
        c[f"{s}/generator_list"] = base_denoise(s, p=2, generator="list")
        c[f"{s}/callback_steps2"] = base_denoise(s, callback_steps=2)
        # ---- VideoUpscalePipeline
        c[f"{s}/vsr"] = vsr(s)
        c[f"{s}/vsr_windows"] = vsr(s, **WINDOWS)
        c[f"{s}/vsr_guidance_sequence"] = vsr(s, guidance_scale=[9.0])
        c[f"{s}/vsr_rescale"] = vsr(s, guidance_rescale=0.7)
        c[f"{s}/vsr_windows_rescale"] = vsr(s, guidance_rescale=0.7, **WINDOWS)
        c[f"{s}/vsr_cache"] = vsr(s, cache_interval=2)
        c[f"{s}/vsr_call"] = vsr(s, "call")
        c[f"{s}/vsr_call_windows_rescale_cache_off"] = vsr(s, "call", guidance_rescale=0.7, cache_interval=1, **WINDOWS)
        c[f"{s}/vsr_call_cache"] = vsr(s, "call", cache_interval=2, cache_depth=2)
        c[f"{s}/vsr_chunks"] = vsr(s, "chunks", frames=6, short_seq=4)
        c[f"{s}/vsr_chunks_overlap"] = vsr(s, "chunks", frames=6, short_seq=4, overlap=2)
        c[f"{s}/vsr_chunks_cache"] = vsr(s, "chunks", frames=6, short_seq=4, cache_interval=2)
    c["ddim/eta0"] = base_denoise("ddim", eta=0.0)
    c["ddim/eta0.5"] = base_denoise("ddim", eta=0.5)
    c["ddim/eta0.5_windows"] = base_denoise("ddim", eta=0.5, **WINDOWS)
    c["ddim/vsr_eta0.5"] = vsr("ddim", eta=0.5)
    c["euler/guided"] = base_denoise("euler")
    c["euler/known_start1"] = base_denoise("euler", known=known_of, start_step=1)
    c["euler/freeinit_windows"] = base_denoise("euler", free_init=FREE, **WINDOWS)
    c["euler/vsr"] = vsr("euler")

    # ---- refused calls: every combination that is refused, through `denoise` and through `__call__`, and calls where two apply
    video = lambda shape_: torch.zeros(shape_[0], shape_[2], 32, 48, 3, dtype=torch.uint8)      # noqa: E731
    d, k = base_denoise, base_call
    refused = {
        "denoise/free_known": d("ddpm", free_init=FREE, known=known_of),
        "denoise/free_known_noise": d("ddpm", free_init=FREE, known_noise=known_of),
        "denoise/free_start_step": d("ddpm", free_init=FREE, start_step=1),
        "denoise/free_on_pipeline_known_mask": d("ddpm", free_init_on_pipe=FREE, known=known_of, mask=mask_of),
        "denoise/cache_windows": d("ddpm", cache_interval=2, **WINDOWS),
        "denoise/pag_known": d("ddpm", known=known_of, **PAG),
        "denoise/pag_known_mask": d("ddpm", known=known_of, mask=mask_of, **PAG),
        "denoise/pag_mask_only": d("ddpm", mask=mask_of, **PAG),
        "denoise/pag_known_noise_only": d("ddpm", known_noise=known_of, **PAG),
        "denoise/pag_start_step_only": d("ddpm", start_step=1, **PAG),
        "denoise/pag_windows": d("ddpm", **PAG, **WINDOWS),
        "denoise/pag_windows_not_in_force": d("ddpm", window_length=4, **PAG),
        "denoise/pag_rescale": d("ddpm", guidance_rescale=0.5, **PAG),
        "denoise/pag_rescale_unguided": d("ddpm", p=2, guidance_scale=1.0, guidance_rescale=0.5, **PAG),
        "denoise/pag_sequence": d("ddpm", guidance_scale=[7.5], parts=3, **PAG),
        "denoise/pag_three_prompts": d("ddpm", p=3, **PAG),
        "denoise/pag_five_prompts_unguided": d("ddpm", p=5, guidance_scale=1.0, **PAG),
        "denoise/pag_scale_negative": d("ddpm", pag_scale=-1.0),
        "denoise/pag_adaptive_scale_nan": d("ddpm", pag_adaptive_scale=float("nan")),
        "denoise/windows_known_mask": d("ddpm", known=known_of, mask=mask_of, **WINDOWS),
        "denoise/windows_start_step": d("ddpm", start_step=1, **WINDOWS),
        "denoise/windows_not_in_force_known": d("ddpm", known=known_of, window_length=4),
        "denoise/window_length_0": d("ddpm", window_length=0),
        "denoise/mask_without_known": d("ddpm", mask=mask_of),
        "denoise/start_step_without_known": d("ddpm", start_step=1),
        "denoise/start_step_past_the_end": d("ddpm", known=known_of, start_step=3),
        "denoise/cache_interval_0": d("ddpm", cache_interval=0),
        "denoise/cache_depth_0": d("ddpm", cache_interval=2, cache_depth=0),
        "denoise/free_num_iters_0": d("ddpm", free_init=dict(num_iters=0)),
        "denoise/ctx_rows": d("ddpm", parts=3),
        # two refusals at once
        "denoise/free_known+cache_windows": d("ddpm", free_init=FREE, known=known_of, cache_interval=2, **WINDOWS),
        "denoise/free_known+pag_known": d("ddpm", free_init=FREE, known=known_of, **PAG),
        "denoise/free_known+cache_interval_0": d("ddpm", free_init=FREE, known=known_of, cache_interval=0),
        "denoise/free_known+windows_known": d("ddpm", free_init=FREE, known=known_of, **WINDOWS),
        "denoise/cache_windows+pag_windows": d("ddpm", cache_interval=2, **PAG, **WINDOWS),
        "denoise/cache_windows+pag_scale_negative": d("ddpm", cache_interval=2, pag_scale=-1.0, **WINDOWS),
        "denoise/cache_windows+windows_known": d("ddpm", cache_interval=2, known=known_of, **WINDOWS),
        "denoise/pag_known+windows_known": d("ddpm", known=known_of, **PAG, **WINDOWS),
        "denoise/pag_start_step+windows_known": d("ddpm", start_step=1, **PAG, **WINDOWS),
        "denoise/pag_windows+pag_rescale": d("ddpm", guidance_rescale=0.5, **PAG, **WINDOWS),
        "denoise/pag_sequence+pag_rescale": d("ddpm", guidance_scale=[7.5], guidance_rescale=0.5, parts=3, **PAG),
        "denoise/pag_rescale+pag_three_prompts": d("ddpm", p=3, guidance_rescale=0.5, **PAG),
        "denoise/pag_known+mask_without_known": d("ddpm", mask=mask_of, start_step=1, **PAG),
        "denoise/windows_known+window_length_0": d("ddpm", known=known_of, window_length=0),
        "call/cache_windows": k("ddpm", cache_interval=2, **WINDOWS),
        "call/free_known_latents": k("ddpm", free_init=FREE, known_latents=known_of),
        "call/free_known_mask": k("ddpm", free_init=FREE, known_mask=mask_of),
        "call/free_video": k("ddpm", free_init=FREE, video=video),
        "call/free_strength": k("ddpm", free_init=FREE, strength=0.5),
        "call/free_on_pipeline_known_latents": k("ddpm", free_init_on_pipe=FREE, known_latents=known_of),
        "call/windows_known_latents": k("ddpm", known_latents=known_of, known_mask=mask_of, **WINDOWS),
        "call/windows_video": k("ddpm", video=video, **WINDOWS),
        "call/windows_strength": k("ddpm", strength=0.5, **WINDOWS),
        "call/windows_not_in_force_known_latents": k("ddpm", known_latents=known_of, window_length=4),
        "call/pag_known_latents": k("ddpm", known_latents=known_of, **PAG),
        "call/pag_video": k("ddpm", video=video, **PAG),
        "call/pag_known_mask": k("ddpm", known_mask=mask_of, **PAG),
        "call/pag_strength_only": k("ddpm", strength=0.5, **PAG),
        "call/pag_windows": k("ddpm", **PAG, **WINDOWS),
        "call/pag_rescale": k("ddpm", guidance_rescale=0.5, **PAG),
        "call/pag_rescale_unguided": k("ddpm", guidance_scale=1.0, guidance_rescale=0.5, **PAG),
        "call/pag_sequence": k("ddpm", guidance_scale=[7.5], **PAG),
        "call/pag_three_prompts": k("ddpm", p=3, **PAG),
        "call/pag_three_images_per_prompt": k("ddpm", num_images_per_prompt=3, **PAG),
        "call/pag_scale_inf": k("ddpm", pag_scale=float("inf")),
        "call/cache_interval_0": k("ddpm", cache_interval=0),
        "call/window_length_0": k("ddpm", window_length=0),
        "call/rescale_out_of_range": k("ddpm", guidance_rescale=1.5),
        "call/sequence_length": k("ddpm", guidance_scale=[7.5, 5.0]),
        # two refusals at once
        "call/cache_windows+free_known": k("ddpm", cache_interval=2, free_init=FREE, known_latents=known_of, **WINDOWS),
        "call/cache_interval_0+free_known": k("ddpm", cache_interval=0, free_init=FREE, known_latents=known_of),
        "call/cache_windows+pag_windows": k("ddpm", cache_interval=2, **PAG, **WINDOWS),
        "call/free_known+windows_known": k("ddpm", free_init=FREE, known_latents=known_of, **WINDOWS),
        "call/free_known+pag_known": k("ddpm", free_init=FREE, known_latents=known_of, **PAG),
        "call/windows_known+pag_known": k("ddpm", known_latents=known_of, **PAG, **WINDOWS),
        "call/windows_strength+pag_windows": k("ddpm", strength=0.5, **PAG, **WINDOWS),
        "call/pag_known_latents+pag_rescale": k("ddpm", known_latents=known_of, guidance_rescale=0.5, **PAG),
        "call/pag_video+pag_known_mask": k("ddpm", video=video, known_mask=mask_of, **PAG),
        "call/pag_windows+pag_rescale": k("ddpm", guidance_rescale=0.5, **PAG, **WINDOWS),
        "call/pag_sequence+pag_rescale": k("ddpm", guidance_scale=[7.5], guidance_rescale=0.5, **PAG),
        "call/pag_sequence+sequence_length": k("ddpm", guidance_scale=[7.5, 5.0], **PAG),
        "call/pag_rescale+rescale_out_of_range": k("ddpm", guidance_rescale=1.5, **PAG),
        "vsr/denoise_cache_windows": vsr("ddpm", cache_interval=3, **WINDOWS),
        "vsr/denoise_unguided": vsr("ddpm", guidance_scale=1.0),
        "vsr/denoise_window_length_0": vsr("ddpm", window_length=0),
        "vsr/denoise_cache_windows+window_length_0": vsr("ddpm", cache_interval=2, window_length=0),
        "vsr/call_cache_windows": vsr("ddpm", "call", cache_interval=2, **WINDOWS),
        "vsr/chunks_overlap_cache": vsr("ddpm", "chunks", frames=6, short_seq=4, overlap=2, cache_interval=2),
    }
    # calls that are wrong in two unrelated ways: a refusal or range of one argument against a check of another, in the order the
    # checks have always run
    wrong_known = lambda lat: torch.zeros(1, 4, 3, 4, 6)        # noqa: E731
    refused.update({
        "denoise/window_length_0+rescale_range": d("ddpm", window_length=0, guidance_rescale=1.5),
        "denoise/window_stride+rescale_range": d("ddpm", guidance_rescale=1.5, frames=6, window_length=4, window_stride=5),
        "denoise/window_weights+sequence_length": d("ddpm", guidance_scale=[7.5, 5.0], frames=6, window_length=4, window_weights="gauss"),
        "denoise/start_step_without_known+sequence_length": d("ddpm", start_step=1, guidance_scale=[7.5, 5.0]),
        "denoise/mask_without_known+rescale_range": d("ddpm", mask=mask_of, guidance_rescale=-0.5),
        "denoise/start_step_past_the_end+rescale_range": d("ddpm", known=known_of, start_step=5, guidance_rescale=1.5),
        "denoise/sequence_values+ctx_rows": d("ddpm", guidance_scale=[1.0], parts=3),
        "denoise/rescale_range+ctx_rows": d("ddpm", guidance_rescale=1.5, parts=3),
        "denoise/ctx_rows+known_shape": d("ddpm", parts=3, known=wrong_known),
        "denoise/ctx_rows_pag+known_noise_shape": d("ddpm", parts=2, **PAG),
        "denoise/ctx_rows+generator_list": d("ddpm", parts=3, generator="long_list"),
        "denoise/known_shape": d("ddpm", known=wrong_known),
        "denoise/known_shape+generator_list": d("ddpm", known=wrong_known, generator="long_list"),
        "denoise/generator_list+known_noise_shape": d("ddpm", known=known_of, known_noise=wrong_known, generator="long_list"),
        "denoise/known_noise_shape": d("ddpm", known=known_of, known_noise=wrong_known),
        "denoise/steps_above_training+window_length_0": d("ddpm", steps=2000, window_length=0),
        "denoise/steps_above_training+start_step_past_the_end": d("ddpm", steps=2000, known=known_of, start_step=5),
        "denoise/steps_above_training+rescale_range": d("ddpm", steps=2000, guidance_rescale=1.5),
        "denoise/cache_windows+rescale_range": d("ddpm", cache_interval=2, guidance_rescale=1.5, **WINDOWS),
        "denoise/pag_rescale+rescale_range": d("ddpm", guidance_rescale=1.5, **PAG),
        "call/callback_steps+cache_interval_0": k("ddpm", callback_steps=0, cache_interval=0),
        "call/callback_steps+cache_windows": k("ddpm", callback_steps=0, cache_interval=2, **WINDOWS),
        "call/height+free_known": k("ddpm", height=33, free_init=FREE, known_latents=known_of),
        "call/height+windows_known": k("ddpm", height=33, known_latents=known_of, **WINDOWS),
        "call/no_prompt+cache_windows": k("ddpm", prompt_embeds=None, negative_prompt_embeds=None, cache_interval=2, **WINDOWS),
        "call/no_prompt+free_num_iters_0": k("ddpm", prompt_embeds=None, negative_prompt_embeds=None, free_init=dict(num_iters=0)),
        "call/height+pag_known": k("ddpm", height=33, known_latents=known_of, **PAG),
        "call/callback_steps+pag_rescale": k("ddpm", callback_steps=0, guidance_rescale=0.5, **PAG),
        "call/callback_steps+pag_scale_negative": k("ddpm", callback_steps=0, pag_scale=-1.0),
        "call/no_prompt+pag_windows": k("ddpm", prompt_embeds=None, negative_prompt_embeds=None, **PAG, **WINDOWS),
        "call/height+rescale_range": k("ddpm", height=33, guidance_rescale=1.5),
        "call/rescale_range+window_length_0": k("ddpm", guidance_rescale=1.5, window_length=0),
        "call/rescale_range+known_mask_without_known": k("ddpm", guidance_rescale=1.5, known_mask=mask_of),
        "call/sequence_length+strength_without_known": k("ddpm", guidance_scale=[7.5, 5.0], strength=0.5),
        "call/callback_steps": k("ddpm", callback_steps=0),
        "call/height": k("ddpm", height=33),
        "vsr/denoise_unguided+window_length_0": vsr("ddpm", guidance_scale=1.0, window_length=0),
        "vsr/denoise_unguided+window_stride": vsr("ddpm", guidance_scale=1.0, frames=6, window_length=4, window_stride=5),
        "vsr/denoise_rescale_range+window_length_0": vsr("ddpm", guidance_rescale=1.5, window_length=0),
        "vsr/denoise_rescale_range+window_stride": vsr("ddpm", guidance_rescale=1.5, frames=6, window_length=4, window_stride=5),
        "vsr/denoise_cache_interval_0+unguided": vsr("ddpm", cache_interval=0, guidance_scale=1.0),
        "vsr/denoise_cache_windows+unguided": vsr("ddpm", cache_interval=2, guidance_scale=1.0, **WINDOWS),
        "vsr/denoise_sequence_length": vsr("ddpm", guidance_scale=[9.0, 5.0]),
        "vsr/denoise_steps_above_training+window_length_0": vsr("ddpm", steps=2000, window_length=0),
        "vsr/call_rescale_range+cache_windows": vsr("ddpm", "call", guidance_rescale=1.5, cache_interval=2, **WINDOWS),
        "check_pag/known_flag": direct_check_pag(3.0, 0.0, 1, 7.5, 0.0, known=True),
        "check_pag/window_length_before_known": direct_check_pag(3.0, 0.0, 1, 7.5, 0.0, window_length=4, known=True),
        "check_pag/any_name": direct_check_pag(3.0, 0.0, 1, 7.5, 0.0, something=0),
        "check_pag/sequence": direct_check_pag(3.0, 0.0, 1, [7.5], 0.0),
        "check_pag/rescale": direct_check_pag(3.0, 0.0, 1, 7.5, 0.5),
        "check_pag/five_prompts": direct_check_pag(3.0, 0.0, 5, 1.0, 0.0),
        "check_pag/scale_nan": direct_check_pag(float("nan"), 0.0, 1, 7.5, 0.0),
    })
    c.update({f"refused/{name}": run for name, run in refused.items()})
    # check_pag with PAG off judges nothing else
    c["check_pag/off_rescale_range"] = direct_check_pag(0.0, 0.0, 8, 7.5, 1.5, window_length=4, known=True)
    c["check_pag/off_sequence_length"] = direct_check_pag(0.0, 0.0, 1, [7.5, 5.0], 0.0)
    c["check_pag/on"] = direct_check_pag(3.0, 0.001, 2, 7.5, 0.0, known=None, window_length=None)
    c["check_pag/on_unguided_four"] = direct_check_pag(3.0, 0.0, 4, 1.0, 0.0)
    return c


CASES = cases()


def record(monkeypatch, run):
    """The events of one case; a refused call ends with the exception's type and text."""
    events = []
    install(monkeypatch, events)
    try:
        run(events)
    except Exception as e:      # noqa: BLE001
        events.append(["raised", type(e).__name__, str(e)])
    return json.loads(json.dumps(events))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_trace_is_the_recorded_one(monkeypatch, golden, name):
    got, want = record(monkeypatch, CASES[name]), golden[name]
    assert name.startswith("refused/") == (got[-1][0] == "raised"), got[-1]
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: event {n}"
    assert len(got) == len(want)


if __name__ == "__main__":          # rewrite the fixture from the tree this file runs in
    traces = {}
    for case_name, case in CASES.items():
        with pytest.MonkeyPatch.context() as mp:
            traces[case_name] = record(mp, case)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(traces[n], separators=(',', ':'))}" for n in sorted(traces)) + "\n}\n")
    print(f"{len(traces)} cases, {sum(len(t) for t in traces.values())} events -> {GOLDEN}")
