"""Host-side mirror of `vsr/models/pipeline_stable_diffusion_upscale_video_3d.py` (reference): the latent video upscaling
loop of the VSR stage, and the 8-frame chunk driver of `vsr/sample.py:104-123`.

`__call__` keeps the reference's keywords (prompt / image / num_inference_steps / guidance_scale / noise_level /
negative_prompt / eta / generator / latents / prompt_embeds / negative_prompt_embeds / output_type / callback).  The loop
(:706-735) runs the engine with the fused guidance + scheduler-step kernel: per step the UNet sees
[latents | noised low-res frames | 0] for the [negative | prompt] halves, then `lavie_cfg_sampler_step` applies guidance, the
scheduler update in its five-coefficient form and writes the next fp16 model input (a multistep scheduler, `multistep = True`:
`lavie_cfg_multistep_step` with an x0 history that lives for one call, so for one chunk).  Text encoder and VAE are stock
PyTorch-ROCm objects a caller may attach (outside the latents metric): without them pass `prompt_embeds` and use
`output_type="latent"`."""
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import torch

from .. import sampling
from ..scheduling_ddpm import DDPMScheduler, randn_tensor


@dataclass
class StableDiffusionPipelineOutput:
    images: torch.Tensor
    nsfw_content_detected: Optional[list] = None


class VideoUpscalePipeline:
    def __init__(self, unet, scheduler, low_res_scheduler=None, vae=None, text_encoder=None, tokenizer=None,
                 max_noise_level: int = 350):
        self.unet, self.scheduler, self.vae, self.text_encoder, self.tokenizer = unet, scheduler, vae, text_encoder, tokenizer
        # the x4-upscaler's low_res_scheduler (its scheduler_config.json is not part of the reference tree): DDPM, cosine betas
        self.low_res_scheduler = low_res_scheduler or DDPMScheduler(beta_schedule="squaredcos_cap_v2")
        self.max_noise_level = max_noise_level

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' enable_freeu: forwarded to the UNet (UNet3DConditionModel.enable_freeu), where the setting lives."""
        self.unet.enable_freeu(s1, s2, b1, b2)

    def disable_freeu(self):
        self.unet.disable_freeu()

    @property
    def device(self):
        return self.unet.device

    def check_inputs(self, image, noise_level, callback_steps, prompt, prompt_embeds, negative_prompt_embeds):
        """pipeline_stable_diffusion_upscale_video_3d.py:376-439 (the checks that do not need a tokenizer)."""
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`")
        if prompt is not None and self.text_encoder is None:
            raise ValueError("no text encoder attached: pass prompt_embeds / negative_prompt_embeds")
        if prompt_embeds is not None and negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape")
        if image is None:
            raise ValueError("`image` input cannot be undefined.")
        if noise_level > self.max_noise_level:
            raise ValueError(f"`noise_level` has to be <= {self.max_noise_level} but is {noise_level}")

    def prepare_latents_3d(self, batch_size, num_channels_latents, seq_len, height, width, dtype, device, generator, latents=None):
        """:441-452."""
        shape = (batch_size, num_channels_latents, seq_len, height, width)
        if latents is None:
            latents = randn_tensor(shape, generator=generator, device=device, dtype=dtype)
        else:
            if tuple(latents.shape) != shape:
                raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma

    # ------------------------------------------------------------------ the denoise loop (:706-735)
    @torch.no_grad()
    def denoise(self, latents: torch.Tensor, image: torch.Tensor, ctx: torch.Tensor, noise_level: int,
                num_inference_steps: int, guidance_scale: float, eta: float = 0.0, generator=None,
                callback: Optional[Callable] = None, callback_steps: int = 1, window_length: Optional[int] = None,
                window_stride: Optional[int] = None, window_weights: str = "triangle",
                guidance_rescale: float = 0.0, cache_interval: Optional[int] = None, cache_depth: int = 1) -> torch.Tensor:
        """latents fp32 [P, 4, F, h, w]; image = the NOISED low-res frames [P, 3, F, h, w]; ctx fp16 [2P, n, d] =
        [negative | prompt] -> denoised latents fp32.  The loop and its buffers are lavie_amd.sampling's (`Run`); this
        pipeline's own are the low-res frames and the class labels of its forward.

        `window_length` below F, for a clip longer than the model's window: ONE latent tensor holds all F frames (and one x0
        history for a multistep scheduler); per step the UNet runs on every window of `window_length` frames with that window's
        slice of the low-res frames (sliced once, before the loop), then ONE launch (ops.window_step) averages the windows' noise
        predictions per frame with the normalised `window_weights` profile, advances the whole clip by one scheduler step and
        writes every window's next fp16 model input.  `window_stride` defaults to three quarters of the window.  Unlike
        independent chunks, neighbouring windows share their overlap frames at every step, so there is no seam between them.

        `guidance_scale` may be a sequence with one value > 1 per latent, `guidance_rescale` in (0, 1] is diffusers'
        rescale_noise_cfg inside the fused step: see VideoGenPipeline.denoise.

        `cache_interval` = N > 1: the layer cache (DeepCache; `UNet.enable_layer_cache` at `cache_depth`): the whole UNet runs on
        steps 0, N, 2N, ... of this call, so every chunk starts with a refresh, the shallow walk on the steps between.  Not
        combined with frame windows.  None or 1 is the call without it."""
        _, cache_interval, _ = sampling.check_features(sampling.Surface(("cache",)), latents.shape[2], window_length=window_length,
                                                       cache=(cache_interval, cache_depth),
                                                       unipc=bool(getattr(self.scheduler, "unipc", False)))
        geometry = sampling.window_geometry(latents.shape[2], window_length, window_stride, window_weights)
        plan = sampling.StepPlan(self.scheduler, num_inference_steps, eta)
        # the scalar itself, or the table route with its buffers, allocated here once for the loop
        guidance = sampling.guidance_of(guidance_scale, guidance_rescale, latents, geometry.frames, len(geometry.starts))
        if guidance is None:
            raise NotImplementedError("guidance_scale <= 1 (no classifier-free guidance) is outside the fused MI355X loop")
        # one x0 history per call, so per chunk
        run = sampling.Run(latents, geometry, plan, guidance, 2 * latents.shape[0], generator, cache_interval=cache_interval)
        run.fill(plan.input_scale(0))
        low = []                                            # every window's slice of the low-res frames, for both halves  (:641)
        for s in run.starts:
            img = image[:, :, s:s + run.frames]
            low.append(torch.cat([img, img], dim=0).to(device=run.x.device, dtype=torch.float16).contiguous())
        labels = torch.full((run.batch,), int(noise_level), dtype=torch.int64)                                        # :644
        # text keys / values once per chunk (or once for the whole windowed clip), not once per block and step
        with sampling.layer_cache_session(self.unet, cache_interval, cache_depth), \
                sampling.engine_session(self.unet, run.batch, run.frames, *run.x.shape[3:], ctx) as ctx:
            def forward(w, i, layer_cache_mode):                                                                      # :716-718
                return self.unet(run.model_in[w], run.t_dev[i], low[w], encoder_hidden_states=ctx, class_labels=labels,
                                 **sampling.forward_keywords(layer_cache_mode)).sample
            return run.loop(forward, callback, callback_steps)                                                        # :721-726

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, image: Optional[torch.Tensor] = None,
                 num_inference_steps: int = 75, guidance_scale: float = 9.0, noise_level: int = 20, negative_prompt=None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, output_type: Optional[str] = "latent",
                 return_dict: bool = True, callback=None, callback_steps: int = 1, window_length: Optional[int] = None,
                 window_stride: Optional[int] = None, window_weights: str = "triangle", guidance_rescale: float = 0.0,
                 cache_interval: Optional[int] = None, cache_depth: int = 1):
        """`guidance_scale`: one number > 1, or a sequence with one value > 1 per prompt (repeated per `num_images_per_prompt`);
        `guidance_rescale` in [0, 1]: diffusers' rescale_noise_cfg inside the fused step; `cache_interval` = N > 1: the layer cache,
        the whole UNet on every N-th step only, at `cache_depth` (not with `window_length`).  See `denoise`."""
        self.check_inputs(image, noise_level, callback_steps, prompt, prompt_embeds, negative_prompt_embeds)
        if prompt is not None:
            raise NotImplementedError("text encoding is not built: pass prompt_embeds / negative_prompt_embeds")
        if negative_prompt_embeds is None:
            raise ValueError("negative_prompt_embeds is required for classifier-free guidance")
        device = self.device
        batch = prompt_embeds.shape[0] * (num_images_per_prompt or 1)
        _, scales, guidance_rescale = sampling.check_guidance(guidance_scale, guidance_rescale, prompt_embeds.shape[0],
                                                              num_images_per_prompt or 1)
        if scales is not None:
            guidance_scale = scales                # one value per latent
        ctx = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0).to(device, torch.float16).contiguous()
        image = image.to(device=device, dtype=torch.float32)
        # 5. add noise to the low-res frames at `noise_level` (:629-633)
        noise = randn_tensor(image.shape, generator=generator, device=device, dtype=torch.float32)
        image = self.low_res_scheduler.add_noise(image, noise, torch.tensor([noise_level] * image.shape[0]))
        seq_len, height, width = image.shape[2:]
        latents = self.prepare_latents_3d(batch, 4, seq_len, height, width, torch.float32, device, generator, latents)
        if 4 + image.shape[1] != self.unet.config.in_channels:                                       # :692-701
            raise ValueError(f"Incorrect configuration settings! The config of `pipeline.unet` expects "
                             f"{self.unet.config.in_channels} but received 4 + {image.shape[1]} channels")
        features = {}                          # a feature's keywords reach `denoise` only when the feature is on
        if guidance_rescale:
            features.update(guidance_rescale=guidance_rescale)
        if cache_interval not in (None, 1):
            features.update(cache_interval=cache_interval, cache_depth=cache_depth)
        latents = self.denoise(latents, image, ctx, noise_level, num_inference_steps, guidance_scale, eta, generator, callback,
                               callback_steps, window_length, window_stride, window_weights, **features)
        if output_type != "latent":
            if self.vae is None:
                raise ValueError("no vae attached: use output_type='latent'")
            b, c, f, h, w = latents.shape
            frames = latents.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
            scale = 1.0 / self.vae.config.scaling_factor                                                # :354-358
            dec = [self.vae.decode(frames[i:i + 4].to(next(self.vae.parameters()).dtype) * scale).sample.clamp(-1, 1).cpu()
                   for i in range(0, b * f, 4)]                                                        # :757-770, short_seq 4
            latents = torch.cat(dec, dim=0)
        if not return_dict:
            return (latents,)
        return StableDiffusionPipelineOutput(images=latents)


def upscale_in_chunks(pipeline: VideoUpscalePipeline, vframes: torch.Tensor, short_seq: int = 8, overlap: int = 0, **kw) -> torch.Tensor:
    """vsr/sample.py:104-123: clips longer than `short_seq` frames go through the pipeline `short_seq` frames at a time
    (same generator across chunks); outputs are concatenated along the frame axis.
    overlap > 0 (not in the reference): the whole clip is ONE run over windows of `short_seq` frames that share `overlap` frames
    with their neighbours, fused at every step (`VideoUpscalePipeline.denoise(window_length=)`), so the chunks no longer meet at a seam.
    `cache_interval` / `cache_depth` in `kw` (the layer cache) reach every chunk's call, so each chunk starts with a full step; with
    overlap > 0 on a clip longer than `short_seq` the pipeline refuses them."""
    total = vframes.shape[2]
    if not 0 <= overlap < short_seq:
        raise ValueError(f"overlap={overlap} must lie in 0..{short_seq - 1} (short_seq={short_seq})")
    if total <= short_seq:
        return pipeline(image=vframes, **kw).images
    if overlap > 0:
        return pipeline(image=vframes, window_length=short_seq, window_stride=short_seq - overlap, **kw).images
    outs = [pipeline(image=vframes[:, :, s:min(total, s + short_seq)], **kw).images for s in range(0, total, short_seq)]
    return torch.cat(outs, dim=2)
