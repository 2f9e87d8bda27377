"""The three-stage cascade of the reference as one on-device driver (BASELINE.json configs[4]): base T2V
(16 x 320 x 512) -> frame interpolation (61 frames) -> video super-resolution (61 x 1280 x 2048).

The reference runs three scripts that hand mp4 files to each other (base/pipelines/sample.py, interpolation/sample.py,
vsr/sample.py); the tensors that cross a stage boundary are the decoded frames in [-1, 1], so the driver keeps them on the
device instead of writing files.  Each step cites the script line it reproduces.  The UNets and samplers are the HIP-path
objects of `lavie_amd`; text encoders and VAEs are stock PyTorch-ROCm objects passed in by the caller (outside the latents
metric)."""
from typing import Optional

import numpy as np
import torch

from .free_init import coerce
from .vsr.pipeline import upscale_in_chunks


def decode_frames(vae, latents: torch.Tensor, scaling: Optional[float] = None, chunk: int = 4) -> torch.Tensor:
    """[b, 4, f, h, w] latents -> frames [b, 3, f, H, W] in [-1, 1] (pipeline_videogen.py:422-427; vsr pipeline :354-358)."""
    scaling = vae.config.scaling_factor if scaling is None else scaling
    b, c, f, h, w = latents.shape
    flat = latents.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w).to(next(vae.parameters()).dtype) / scaling
    out = torch.cat([vae.decode(flat[i:i + chunk]).sample.clamp(-1, 1) for i in range(0, b * f, chunk)], dim=0)
    return out.reshape(b, f, *out.shape[1:]).permute(0, 2, 1, 3, 4)


def interpolation_condition(vae, frames: torch.Tensor, num_frames: int = 61, generator=None) -> torch.Tensor:
    """interpolation/sample.py:74-79, 135-149: the 16 base frames are resampled to `num_frames` by index
    (np.linspace(0, 15, num_frames, dtype=int)), VAE-encoded (x 0.18215), every 4th latent frame is kept and repeated 4x, and
    frames [1:-2] of that are the `copied_video` conditioning.  frames: [b, 3, 16, H, W] in [-1, 1]."""
    b, _, f, H, W = frames.shape
    idx = torch.from_numpy(np.linspace(0, f - 1, num_frames, dtype=int)).to(frames.device)
    vid = frames.index_select(2, idx).permute(0, 2, 1, 3, 4).reshape(b * num_frames, 3, H, W).to(next(vae.parameters()).dtype)
    lat = torch.cat([vae.encode(vid[i:i + 8]).latent_dist.sample(generator) for i in range(0, b * num_frames, 8)], dim=0) * 0.18215
    lat = lat.reshape(b, num_frames, *lat.shape[1:]).permute(0, 2, 1, 3, 4)
    lr = torch.arange(0, num_frames + 1, 4, device=lat.device)
    lr = lr[lr < num_frames]
    copied = torch.repeat_interleave(lat.index_select(2, lr), 4, dim=2)[:, :, 1:-2]
    return copied.float()


@torch.no_grad()
def text_to_video_cascade(base_pipe, interp_unet, interp_diffusion, vsr_pipe, vae, vsr_vae, prompt_embeds, negative_prompt_embeds,
                          vsr_prompt_embeds, vsr_negative_prompt_embeds, interp_prompt_embeds, interp_negative_prompt_embeds,
                          height: int = 320, width: int = 512, base_steps: int = 50, guidance_scale: float = 7.5,
                          interp_frames: int = 61, interp_cfg_scale: float = 4.0, vsr_steps: int = 50,
                          vsr_guidance_scale: float = 7.5, noise_level: int = 150, generator=None, decode_final: bool = True,
                          base_scheduler=None, vsr_scheduler=None, vsr_overlap: int = 0, base_guidance_rescale: float = 0.0,
                          vsr_guidance_rescale: float = 0.0, base_freeu: Optional[dict] = None, vsr_freeu: Optional[dict] = None,
                          base_pag_scale: float = 0.0, base_pag_adaptive_scale: float = 0.0,
                          base_pag_applied_layers=("mid_block",), base_cache_interval: Optional[int] = None,
                          vsr_cache_interval: Optional[int] = None, base_cache_depth: int = 1, vsr_cache_depth: int = 1,
                          base_free_init=None):
    """Returns (base_latents, interp_latents, vsr_latents, frames or None).  Text embeddings are passed per stage (the base
    and interpolation stages use SD-1.4's CLIP, 768 wide; the VSR stage the x4-upscaler's, 1024 wide).
    `base_scheduler` / `vsr_scheduler` replace the two diffusers-style stages' schedulers for this call (for instance a
    DPMSolverMultistepScheduler or a UniPCMultistepScheduler with fewer `base_steps` / `vsr_steps`); the pipelines get their own back
    afterwards.  The interpolation stage samples with its SpacedDiffusion object and has no such switch.  A UniPCMultistepScheduler
    is not combined with `vsr_overlap` > 0 (frame windows) or `base_free_init`: the stage's call refuses by name.
    `vsr_overlap` > 0: the VSR stage samples the 61 frames as ONE run over 8-frame windows sharing that many frames with their
    neighbours (`upscale_in_chunks(overlap=)`) instead of independent chunks; 0 = the reference's chunks.
    `base_guidance_rescale` / `vsr_guidance_rescale`: the `guidance_rescale` of the two diffusers-style stages (0 = off).  The
    interpolation stage's own guidance loop (`forward_with_cfg`) has no such switch.
    `base_freeu` / `vsr_freeu`: dict(s1=, s2=, b1=, b2=) for `enable_freeu` on that stage's UNet during this call; the UNet gets the
    setting it had back afterwards.  None = the UNet's own setting.
    `base_pag_scale` / `base_pag_adaptive_scale` / `base_pag_applied_layers`: perturbed-attention guidance in the base stage (the
    keywords of `VideoGenPipeline.__call__`; 0 = off, the calls without them).  The other two stages have no such switch.
    `base_cache_interval` / `vsr_cache_interval` (with `base_cache_depth` / `vsr_cache_depth`): the layer cache of the two
    diffusers-style stages, the `cache_interval` / `cache_depth` of their pipelines: the whole UNet on every N-th step only; every VSR
    chunk starts with a full step.  None or 1 = the calls without it.  Not with `vsr_overlap` > 0 (frame windows).  The interpolation
    stage's loop has no such switch.
    `base_free_init`: a FreeInit (lavie_amd.free_init) or a mapping of its keywords for the base stage's call (the `free_init` keyword
    of `VideoGenPipeline.__call__`); None = the base pipeline's own setting.  The VSR pipeline and the interpolation sampler have no
    FreeInit."""
    freeu_was = [(pipe.unet, pipe.unet.freeu) for pipe, fu in ((base_pipe, base_freeu), (vsr_pipe, vsr_freeu)) if fu is not None]
    swapped = [(pipe, pipe.scheduler) for pipe, sch in ((base_pipe, base_scheduler), (vsr_pipe, vsr_scheduler)) if sch is not None]
    if base_scheduler is not None:
        base_pipe.scheduler = base_scheduler
    if vsr_scheduler is not None:
        vsr_pipe.scheduler = vsr_scheduler
    try:
        for pipe, fu in ((base_pipe, base_freeu), (vsr_pipe, vsr_freeu)):
            if fu is not None:
                pipe.unet.enable_freeu(fu["s1"], fu["s2"], fu["b1"], fu["b2"])
        return _cascade(base_pipe, interp_unet, interp_diffusion, vsr_pipe, vae, vsr_vae, prompt_embeds, negative_prompt_embeds,
                        vsr_prompt_embeds, vsr_negative_prompt_embeds, interp_prompt_embeds, interp_negative_prompt_embeds, height,
                        width, base_steps, guidance_scale, interp_frames, interp_cfg_scale, vsr_steps, vsr_guidance_scale,
                        noise_level, generator, decode_final, vsr_overlap, base_guidance_rescale, vsr_guidance_rescale,
                        dict(pag_scale=base_pag_scale, pag_adaptive_scale=base_pag_adaptive_scale,
                             pag_applied_layers=base_pag_applied_layers) if base_pag_scale else {},
                        dict(cache_interval=base_cache_interval, cache_depth=base_cache_depth) if base_cache_interval not in (None, 1) else {},
                        dict(cache_interval=vsr_cache_interval, cache_depth=vsr_cache_depth) if vsr_cache_interval not in (None, 1) else {},
                        base_free_init)
    finally:
        for pipe, own in swapped:
            pipe.scheduler = own
        for unet, was in freeu_was:
            unet.enable_freeu(*was)


def _cascade(base_pipe, interp_unet, interp_diffusion, vsr_pipe, vae, vsr_vae, prompt_embeds, negative_prompt_embeds,
             vsr_prompt_embeds, vsr_negative_prompt_embeds, interp_prompt_embeds, interp_negative_prompt_embeds, height, width,
             base_steps, guidance_scale, interp_frames, interp_cfg_scale, vsr_steps, vsr_guidance_scale, noise_level, generator,
             decode_final, vsr_overlap=0, base_guidance_rescale=0.0, vsr_guidance_rescale=0.0, base_pag=None, base_cache=None,
             vsr_cache=None, base_free_init=None):
    dev = base_pipe.device
    base_kw = dict(guidance_rescale=base_guidance_rescale) if base_guidance_rescale else {}       # absent = the calls without it
    base_kw.update(base_pag or {})
    base_kw.update(base_cache or {})
    if base_free_init is not None:
        base_kw["free_init"] = base_free_init
    vsr_kw = dict(guidance_rescale=vsr_guidance_rescale) if vsr_guidance_rescale else {}
    vsr_kw.update(vsr_cache or {})
    # 1. base T2V (base/pipelines/sample.py:78-91)
    base = base_pipe(prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, height=height, width=width,
                     video_length=16, num_inference_steps=base_steps, guidance_scale=guidance_scale, generator=generator,
                     output_type="latent", **base_kw).video
    frames16 = decode_frames(vae, base, 0.18215)
    # 2. interpolation 16 -> 61 frames (interpolation/sample.py:135-174)
    copied = interpolation_condition(vae, frames16, interp_frames)
    z = torch.randn(1, 4, interp_frames, height // 8, width // 8, device=dev)
    z2, copied2 = torch.cat([z] * 2), torch.cat([copied] * 2)
    ctx = torch.cat([interp_prompt_embeds, interp_negative_prompt_embeds], dim=0)                 # prompt first (:157)
    interp = interp_diffusion.ddim_sample_loop(
        interp_unet.forward_with_cfg, z2.shape, z2, clip_denoised=False,
        model_kwargs=dict(encoder_hidden_states=ctx, class_labels=None, cfg_scale=interp_cfg_scale), device=dev, mask=None,
        x_start=copied2, use_concat=True, copy_no_mask=True).chunk(2, dim=0)[0]
    frames61 = decode_frames(vae, interp, 0.18215)
    # 3. video super-resolution in 8-frame chunks (vsr/sample.py:90-123): the decoded frames are the low-res conditioning
    up = upscale_in_chunks(vsr_pipe, frames61, short_seq=8, overlap=vsr_overlap, prompt_embeds=vsr_prompt_embeds,
                           negative_prompt_embeds=vsr_negative_prompt_embeds, num_inference_steps=vsr_steps,
                           guidance_scale=vsr_guidance_scale, noise_level=noise_level, generator=generator, **vsr_kw)
    frames = decode_frames(vsr_vae, up, None, chunk=1) if decode_final else None
    return base, interp, up, frames


# ------------------------------------------------------------------ clips longer than one base call: continuation by pinned overlap
@torch.no_grad()
def continue_clip(pipe, prev_latents: torch.Tensor, overlap: int = 4, **call_kwargs) -> torch.Tensor:
    """One more clip after `prev_latents` [P, C, F, h, w]: a base call whose first `overlap` frames are pinned to the last `overlap`
    frames of `prev_latents` (VideoGenPipeline's `known_latents` / `known_mask`), so they come back bit-equal and temporal attention
    carries them into the free frames.  `call_kwargs` go to the pipeline (prompt or prompt_embeds, steps, generator, ...);
    `video_length` defaults to 16, height / width to those of `prev_latents`; `cache_interval` / `cache_depth` (the layer cache) go
    through like the rest.  FreeInit (`free_init` in `call_kwargs`, or enabled on the pipeline) is refused: the clip's start is pinned,
    not noise.  Returns the new clip's latents, overlap included."""
    p, c, f_prev, h, w = prev_latents.shape
    length = int(call_kwargs.pop("video_length", 16))
    if not 1 <= overlap < length or overlap > f_prev:
        raise ValueError(f"overlap={overlap} must lie in 1..{min(length - 1, f_prev)} (new clip {length} frames, previous {f_prev})")
    known = torch.zeros(p, c, length, h, w, dtype=torch.float32, device=prev_latents.device)
    known[:, :, :overlap] = prev_latents[:, :, f_prev - overlap:]
    mask = torch.zeros(p, 1, length, h, w, dtype=torch.float32, device=prev_latents.device)
    mask[:, :, :overlap] = 1.0
    scale = getattr(pipe, "vae_scale_factor", 8)
    call_kwargs.setdefault("height", h * scale)
    call_kwargs.setdefault("width", w * scale)
    call_kwargs["output_type"] = "latent"
    return pipe(video_length=length, known_latents=known, known_mask=mask, **call_kwargs).video


@torch.no_grad()
def text_to_long_video(pipe, prompt, num_clips: int, overlap: int = 4, method: str = "chain", **call_kwargs) -> torch.Tensor:
    """Latents [P, C, L + (num_clips - 1)(L - overlap), h, w] with L = `video_length` (16).  `prompt` may be None when
    `call_kwargs` carry prompt_embeds.
    method "chain": `num_clips` base clips chained by `continue_clip`, the overlap frames stored once; clip n starts when clip
    n - 1 has finished, and nothing later influences an earlier frame.
    method "windows": ONE run over the whole length as `num_clips` windows of L frames at stride L - overlap, fused at every step
    (VideoGenPipeline's `window_length` / `window_stride`): every forward keeps the trained length, the overlap frames are
    shared in both directions.
    `cache_interval` / `cache_depth` in `call_kwargs` (the layer cache) reach every clip's call with method "chain"; "windows" refuses
    them, as the pipeline does.
    `free_init` in `call_kwargs` (or FreeInit enabled on the pipeline) goes to the calls that start from noise: the one run of
    "windows", whose filter spans the whole length, and a "chain" of one clip.  A longer chain pins every later clip's overlap and is
    refused before anything is sampled."""
    if num_clips < 1:
        raise ValueError(f"num_clips={num_clips} must be >= 1")
    if method not in ("chain", "windows"):
        raise ValueError(f"method={method!r} must be 'chain' or 'windows'")
    length = int(call_kwargs.pop("video_length", 16))
    if prompt is not None:
        call_kwargs["prompt"] = prompt
    call_kwargs["output_type"] = "latent"
    if method == "windows":
        if not 0 <= overlap < length:
            raise ValueError(f"overlap={overlap} must lie in 0..{length - 1} (window of {length} frames)")
        total = length + (num_clips - 1) * (length - overlap)
        return pipe(video_length=total, window_length=length, window_stride=length - overlap, **call_kwargs).video
    setting = call_kwargs.get("free_init")
    if num_clips > 1 and coerce(setting if setting is not None else getattr(pipe, "free_init", None)) is not None:
        raise ValueError("FreeInit cannot be combined with method 'chain' over several clips: every clip after the first starts from "
                         "a pinned overlap, not from noise (use method 'windows')")
    clip = pipe(video_length=length, **call_kwargs).video
    parts = [clip]
    for _ in range(num_clips - 1):
        clip = continue_clip(pipe, clip, overlap, video_length=length, **call_kwargs)
        parts.append(clip[:, :, overlap:])
    return torch.cat(parts, dim=2)
