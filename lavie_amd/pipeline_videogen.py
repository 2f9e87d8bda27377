"""Host-side mirror of `base/pipelines/pipeline_videogen.py` (reference): `VideoGenPipeline`.

Keeps the reference call surface (`__call__` keywords, `prompt_embeds=` / `negative_prompt_embeds=` /
`latents=` / `generator=` / `callback`, pipeline_videogen.py:512-535) and its loop semantics
(662-689): CFG batch [negative | prompt], `u + s (c - u)`, DDPM ancestral step.  The loop body runs
on the MI355X: the UNet through liblavie_hip.so and CFG + scheduler step as one fused kernel.
CLIP text encoding and VAE decoding are NOT part of this package's compute path: pass any stock
PyTorch-ROCm `tokenizer`/`text_encoder`/`vae` objects to use them, or work with embeddings and
`output_type="latent"` (what the benchmark measures: video-latents/s).

Image conditioning (the fork's inference.py:248-353): with a `mapper` (lavie_amd.mapping.MappingNetwork) attached, an image
widens each CFG half's context to `cat([text, mapper(image, text)], 1)`: 154 tokens for a 77-token prompt.  The image comes
as `image_tensor` (through `clip_processor` + `clip_model.vision_model`: stock PyTorch, or the engine's HipCLIPVisionModel /
HipMappingNetwork of lavie_amd.image_encoder, see enable_engine_image_encoder) or as precomputed vision features
`image_embeds`.  Without a mapper `image_tensor` is accepted and ignored, as before."""
import contextlib
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import torch

from . import free_init as free_init_mod
from . import ops, sampling          # noqa: F401  (`ops`: the device ops, as callers of this module reach them)
from .scheduling_ddpm import DDPMScheduler, randn_tensor


@dataclass
class StableDiffusionPipelineOutput:
    video: torch.Tensor


class VideoGenPipeline:
    # With guidance the UNet input is the latents twice (line 666): let the engine compute the layers in front of the first text
    # cross-attention once per step (UNet3DConditionModel.set_cfg_shared_input).  False = both halves computed, as the reference does.
    cfg_shared_prefix = True

    # how `denoise` and `__call__` speak to sampling.check_features: the order in which each has always judged its features, and
    # its own words for FreeInit and for the known-latents arguments
    DENOISE = sampling.Surface(("free_init", "cache", "pag", "window_length"), "FreeInit (`free_init`)",
                               "known latents (`known` / `mask` / `known_noise` / `start_step`)")
    CALL = sampling.Surface(("cache", "free_init", "window_length"), "FreeInit (`free_init` / enable_free_init)",
                            "`known_latents` / `known_mask` / `video` / `strength`")
    CALL_PAG = sampling.Surface(("pag",))

    def __init__(self, vae=None, text_encoder=None, tokenizer=None, unet=None, scheduler=None, clip_model=None,
                 clip_processor=None, mapper=None):
        if unet is None:
            raise ValueError("unet is required")
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.clip_model, self.clip_processor, self.mapper = clip_model, clip_processor, mapper
        self.unet = unet
        self.scheduler = scheduler or DDPMScheduler()
        self.vae_scale_factor = 8                        # 2 ** (len(vae.config.block_out_channels) - 1) for SD-1.x
        self.free_init = None                            # enable_free_init / disable_free_init

    def to(self, device):
        self.unet.to(device)
        for m in (self.vae, self.text_encoder, self.clip_model, self.mapper):
            if m is not None and hasattr(m, "to"):          # (callers may hand in placeholders for the CLIP objects)
                m.to(device)
        return self

    # ------------------------------------------------------------------ the text encoder on the engine
    def enable_engine_text_encoder(self):
        """Wraps the attached stock CLIPTextModel in a HipCLIPTextModel (its weights copied to the engine, rounded to fp16): `prompt=`
        then runs on the engine, bit-reproducible and with a prompt's embeddings independent of the batch it is encoded in.
        disable_engine_text_encoder puts the stock module back."""
        from .text_encoder import HipCLIPTextModel
        if self.text_encoder is None:
            raise ValueError("no text_encoder attached")
        if not isinstance(self.text_encoder, HipCLIPTextModel):
            self.text_encoder = HipCLIPTextModel.from_stock(self.text_encoder, device=self.device)

    def disable_engine_text_encoder(self):
        from .text_encoder import HipCLIPTextModel
        if isinstance(self.text_encoder, HipCLIPTextModel):
            if self.text_encoder._stock is None:
                raise ValueError("the engine text encoder was not built from a stock module: nothing to put back")
            self.text_encoder = self.text_encoder._stock

    # ------------------------------------------------------------------ memory knobs of the reference pipeline object
    # base/pipelines/sample.py:72 calls enable_xformers_memory_efficient_attention() unconditionally; the diffusers base class also
    # offers attention slicing and the pipeline VAE slicing / tiling (pipeline_videogen.py:174-204).  They trade speed for memory in
    # the stock attention (`_sliced_attention`, xformers) and the stock VAE; here attention is always the fused flash-style HIP
    # kernel (scores are never materialised) and 288 GB of HBM make the VAE knobs moot, so they are accepted and change nothing.
    def load_lora_weights(self, sd_or_path, scale: float = 1.0, alpha=None, adapter_name=None):
        """The fork's saved adapter (save_lora_weights: `unet.`-prefixed peft keys, fine_tuning.py:689-698) onto the UNet
        (UNet3DConditionModel.load_lora).  Without `adapter_name` it replaces whatever is loaded; with one it is added to (or
        replaced among) the named adapters, which set_adapters blends."""
        self.unet.load_lora(sd_or_path, scale=scale, alpha=alpha, adapter_name=adapter_name)

    def set_adapters(self, adapter_names, adapter_weights=None):
        """diffusers' set_adapters: the active adapters and their blend weights (UNet3DConditionModel.set_adapters)."""
        self.unet.set_adapters(adapter_names, adapter_weights)

    def delete_adapters(self, adapter_names):
        self.unet.delete_adapters(adapter_names)

    def get_list_adapters(self):
        return {"unet": self.unet.get_list_adapters()}

    def get_active_adapters(self):
        return self.unet.get_active_adapters()

    def unload_lora_weights(self):
        """Removes every adapter."""
        self.unet.unload_lora()

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' enable_freeu: forwarded to the UNet (UNet3DConditionModel.enable_freeu), where the setting lives."""
        self.unet.enable_freeu(s1, s2, b1, b2)

    def disable_freeu(self):
        self.unet.disable_freeu()

    def enable_free_init(self, num_iters: int = 3, use_fast_sampling: bool = False, method: str = "butterworth", order: int = 4,
                         spatial_stop_frequency: float = 0.25, temporal_stop_frequency: float = 0.25):
        """diffusers' enable_free_init (FreeInitMixin), same names and defaults: every later `__call__` / `denoise` samples
        `num_iters` times and refines the initial noise in between (lavie_amd.free_init; `denoise`).  The setting lives on the
        pipeline; a `free_init=` keyword of a call overrides it for that call."""
        self.free_init = free_init_mod.FreeInit(num_iters, use_fast_sampling, method, order, spatial_stop_frequency,
                                                temporal_stop_frequency)

    def disable_free_init(self):
        self.free_init = None

    def load_mapper(self, path_or_sd, num_heads: int = 12, engine: bool = False):
        """The fork's saved image mapper (`mapper.pt`, fine_tuning.py:701) -> self.mapper on the pipeline's device, eval mode.
        Works with a LoRA adapter loaded as well: that pair is the fork's sampling configuration.  engine=True: the same network
        on the engine (HipMappingNetwork) instead of torch.nn."""
        from .mapping import MappingNetwork
        net = MappingNetwork.from_checkpoint(path_or_sd, num_heads=num_heads)      # validates keys and shapes for either form
        if engine:
            from .image_encoder import HipMappingNetwork
            self.mapper = HipMappingNetwork.from_stock(net, device=self.device)
            self.mapper._stock = net.to(self.device)
        else:
            self.mapper = net.to(self.device)
        return self.mapper

    # ------------------------------------------------------------------ image conditioning on the engine
    def enable_engine_image_encoder(self, processor=False):
        """Wraps the attached stock `clip_model` (a CLIPModel or a CLIPVisionModel) and `mapper` (a MappingNetwork) in
        HipCLIPVisionModel / HipMappingNetwork (weights copied to the engine, rounded to fp16): `image_tensor=` then runs on the
        engine, bit-reproducible and with an image's tokens independent of the batch.  Either part may be absent or wrapped
        already.  `clip_processor` (resize, crop, normalise) stays the caller's, as the tokenizer does, unless processor=True: then
        the attached stock CLIPImageProcessor is wrapped in HipCLIPImageProcessor (the same pixel_values bit for bit,
        from uint8 images, on the device).  disable_engine_image_encoder puts the stock objects back."""
        from .image_encoder import HipCLIPVisionModel, HipMappingNetwork
        if processor:
            from .clip_score import HipCLIPImageProcessor
            if self.clip_processor is None:
                raise ValueError("processor=True, but no clip_processor is attached")
            if not isinstance(self.clip_processor, HipCLIPImageProcessor):
                self.clip_processor = HipCLIPImageProcessor.from_stock(self.clip_processor, device=self.device)
        if self.clip_model is None and self.mapper is None:
            raise ValueError("no clip_model or mapper attached")
        if self.clip_model is not None and not isinstance(self.clip_model, HipCLIPVisionModel):
            self.clip_model = HipCLIPVisionModel.from_stock(self.clip_model, device=self.device)
        if self.mapper is not None and not isinstance(self.mapper, HipMappingNetwork):
            self.mapper = HipMappingNetwork.from_stock(self.mapper, device=self.device)

    def disable_engine_image_encoder(self):
        from .image_encoder import HipCLIPVisionModel, HipMappingNetwork
        from .clip_score import HipCLIPImageProcessor
        if isinstance(self.clip_processor, HipCLIPImageProcessor) and self.clip_processor._stock is not None:
            self.clip_processor = self.clip_processor._stock
        for attr, cls in (("clip_model", HipCLIPVisionModel), ("mapper", HipMappingNetwork)):
            obj = getattr(self, attr)
            if isinstance(obj, cls):
                if obj._stock is None:
                    raise ValueError(f"the engine {attr} was not built from a stock module: nothing to put back")
                setattr(self, attr, obj._stock)

    def enable_xformers_memory_efficient_attention(self, attention_op=None):
        """No-op: attn1 / attn2 always run the fused online-softmax kernel (attention.hip); nothing to switch on."""
        return None

    def disable_xformers_memory_efficient_attention(self):
        return None

    def set_attention_slice(self, slice_size="auto"):
        """No-op (unet.py:297-360 slices the materialised score matrix; this engine has none)."""
        return None

    def enable_attention_slicing(self, slice_size="auto"):
        return self.set_attention_slice(slice_size)

    def disable_attention_slicing(self):
        return self.set_attention_slice(None)

    def enable_vae_slicing(self):
        """Forwarded to the attached VAE when it has the switch (a stock diffusers AutoencoderKL), else a no-op."""
        if self.vae is not None and hasattr(self.vae, "enable_slicing"):
            self.vae.enable_slicing()

    def disable_vae_slicing(self):
        if self.vae is not None and hasattr(self.vae, "disable_slicing"):
            self.vae.disable_slicing()

    def enable_vae_tiling(self):
        if self.vae is not None and hasattr(self.vae, "enable_tiling"):
            self.vae.enable_tiling()

    def disable_vae_tiling(self):
        if self.vae is not None and hasattr(self.vae, "disable_tiling"):
            self.vae.disable_tiling()

    # ------------------------------------------------------------------ the reference's YAML (base/configs/sample.yaml:16-40)
    @staticmethod
    def from_sample_yaml(path_or_dict, unet, vae=None, text_encoder=None, tokenizer=None):
        """Builds (pipeline, call_kwargs, cfg) from the keys base/pipelines/sample.py reads off its OmegaConf object:
        `sample_method` + `beta_start` / `beta_end` / `beta_schedule` choose and configure the scheduler (sample.py:44-63),
        `video_length`, `image_size`, `num_sampling_steps`, `guidance_scale` become the `__call__` keywords of sample.py:83-89,
        an optional `guidance_rescale` (not a key of the reference) becomes the keyword of that name,
        an optional `freeu: {s1:, s2:, b1:, b2:}` (not a key of the reference either) is set on the UNet (enable_freeu),
        optional `pag_scale` / `pag_adaptive_scale` / `pag_applied_layers` (a name or a list of names) become the keywords of those names,
        optional `cache_interval` / `cache_depth` (the layer cache; not keys of the reference) become the keywords of those names,
        an optional `free_init: {num_iters:, use_fast_sampling:, method:, order:, spatial_stop_frequency:, temporal_stop_frequency:}`
        (not a key of the reference) is set on the pipeline (enable_free_init),
        `seed` is returned in cfg for torch.manual_seed (sample.py:22-23); with `noise: engine` (not a key of the reference) it also
        becomes `generator=noise.PhiloxGenerator(seed)`, seeded engine noise (`noise: torch`, the default, adds nothing).  `use_fp16` and
        `enable_xformers_memory_efficient_attention` are read by nobody in sample.py and are ignored here as well.
        PyYAML's safe loader replaces omegaconf (absent from the image); interpolation / `${...}` references are not resolved."""
        if isinstance(path_or_dict, dict):
            cfg = dict(path_or_dict)
        else:
            import yaml
            with open(path_or_dict) as f:
                cfg = yaml.safe_load(f) or {}
        method = cfg.get("sample_method", "ddpm")
        betas = dict(beta_start=float(cfg.get("beta_start", 1e-4)), beta_end=float(cfg.get("beta_end", 0.02)),
                     beta_schedule=cfg.get("beta_schedule", "linear"))
        if method == "ddpm":
            scheduler = DDPMScheduler(**betas)
        elif method == "ddim":
            from .scheduling_ddim import DDIMScheduler
            scheduler = DDIMScheduler(**betas)
        elif method == "eulerdiscrete":
            from .scheduling_euler_discrete import EulerDiscreteScheduler
            scheduler = EulerDiscreteScheduler(**betas)
        elif method == "dpmsolver++":          # not a branch of sample.py: the second-order multistep sampler of this package
            from .scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
            scheduler = DPMSolverMultistepScheduler(**betas)
        else:
            raise NotImplementedError(f"sample_method {method!r} (sample.py:44-63 knows ddim / eulerdiscrete / ddpm)")
        size = cfg.get("image_size", [320, 512])
        call_kwargs = dict(video_length=int(cfg.get("video_length", 16)), height=int(size[0]), width=int(size[1]),
                           num_inference_steps=int(cfg.get("num_sampling_steps", 50)),
                           guidance_scale=float(cfg.get("guidance_scale", 7.5)))
        if "guidance_rescale" in cfg:
            call_kwargs["guidance_rescale"] = float(cfg["guidance_rescale"])
        for key, conv in (("pag_scale", float), ("pag_adaptive_scale", float),       # perturbed-attention guidance (not keys of the reference)
                          ("pag_applied_layers", lambda v: (v,) if isinstance(v, str) else tuple(v))):
            if key in cfg:
                call_kwargs[key] = conv(cfg[key])
        for key in ("cache_interval", "cache_depth"):
            if key in cfg:
                call_kwargs[key] = int(cfg[key])
        kind = cfg.get("noise", "torch")
        if kind not in ("torch", "engine"):
            raise ValueError(f"`noise` must be 'torch' or 'engine' but is {kind!r}")
        if kind == "engine":
            from .noise import PhiloxGenerator
            call_kwargs["generator"] = PhiloxGenerator(int(cfg.get("seed", 0)))
        pipe = VideoGenPipeline(vae=vae, text_encoder=text_encoder, tokenizer=tokenizer, unet=unet, scheduler=scheduler)
        if "freeu" in cfg:                      # {s1:, s2:, b1:, b2:}, all four: the setting goes onto the model
            fu = cfg["freeu"]
            pipe.enable_freeu(fu["s1"], fu["s2"], fu["b1"], fu["b2"])
        if "free_init" in cfg:                  # any of FreeInit's keywords; the rest keep diffusers' defaults: set on the pipeline
            pipe.enable_free_init(**dict(cfg["free_init"] or {}))
        return pipe, call_kwargs, cfg

    @property
    def device(self):
        return self.unet.device

    # ------------------------------------------------------------------ prompt handling (273-420)
    def _image_features(self, image_tensor, image_embeds, device):
        """CLIP vision features [1 or B, 257, input_dim] for the mapper (inference.py:286-290), or None without an image."""
        if image_embeds is not None:
            return image_embeds.to(device=device)
        if image_tensor is None:
            return None
        if self.clip_model is None or self.clip_processor is None:
            raise ValueError("a mapper is attached and an image given, but there is no clip_model / clip_processor: "
                             "attach them or pass image_embeds")
        pixels = self.clip_processor(images=image_tensor, return_tensors="pt").pixel_values
        # a CLIPModel (the fork's object) holds the tower as .vision_model; a CLIPVisionModel may be the tower itself
        vision = getattr(self.clip_model, "vision_model", self.clip_model)
        pixels = pixels.to(**self._home(vision))
        return vision(pixel_values=pixels).last_hidden_state.to(device=device)

    @staticmethod
    def _home(module):
        """device and dtype a part wants its inputs in: its own .device / .dtype (the engine objects) or its first parameter's"""
        if isinstance(getattr(module, "device", None), torch.device) and isinstance(getattr(module, "dtype", None), torch.dtype):
            return dict(device=module.device, dtype=module.dtype)
        param = next(module.parameters())
        return dict(device=param.device, dtype=param.dtype)

    def _widen(self, embeds, image_features):
        """cat([embeds, mapper(image, embeds)], 1) (inference.py:299-306, 339-345); one image broadcasts over the prompts."""
        if image_features.shape[0] not in (1, embeds.shape[0]):
            raise ValueError(f"got {image_features.shape[0]} images for {embeds.shape[0]} prompts (expected 1 or one per prompt)")
        # the engine mapper reads one image for every prompt itself (same bits as the repeated image, one memory projection)
        img = image_features if getattr(self.mapper, "broadcasts_image", False) else image_features.expand(embeds.shape[0], -1, -1)
        home = self._home(self.mapper)
        mapped = self.mapper(img.to(**home), embeds.to(**home))
        return torch.cat([embeds, mapped.to(device=embeds.device, dtype=embeds.dtype)], dim=1)

    def _encode_prompt(self, prompt, device, num_images_per_prompt, do_cfg, negative_prompt, prompt_embeds,
                       negative_prompt_embeds, image_features=None):
        if prompt_embeds is None:
            if self.tokenizer is None or self.text_encoder is None:
                raise ValueError("no tokenizer/text_encoder attached: pass prompt_embeds / negative_prompt_embeds")
            ids = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length,
                                 truncation=True, return_tensors="pt").input_ids
            prompt_embeds = self.text_encoder(ids.to(device))[0]
        prompt_embeds = prompt_embeds.to(device=device)
        bs, n, _ = prompt_embeds.shape
        if image_features is not None:
            prompt_embeds = self._widen(prompt_embeds, image_features)
        n_ctx = prompt_embeds.shape[1]
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs * num_images_per_prompt, n_ctx, -1)
        if not do_cfg:
            return prompt_embeds
        if negative_prompt_embeds is None:
            if self.tokenizer is None or self.text_encoder is None:
                raise ValueError("no tokenizer/text_encoder attached: pass negative_prompt_embeds")
            neg = [""] * bs if negative_prompt is None else ([negative_prompt] if isinstance(negative_prompt, str) else negative_prompt)
            ids = self.tokenizer(neg, padding="max_length", max_length=n, truncation=True, return_tensors="pt").input_ids
            negative_prompt_embeds = self.text_encoder(ids.to(device))[0]
        negative_prompt_embeds = negative_prompt_embeds.to(device=device)
        if image_features is not None:
            negative_prompt_embeds = self._widen(negative_prompt_embeds, image_features)
        negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs * num_images_per_prompt, n_ctx, -1)
        return torch.cat([negative_prompt_embeds, prompt_embeds])           # line 418: unconditional half first

    def check_inputs(self, prompt, height, width, callback_steps, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`. Please make sure to only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError("Cannot forward both `negative_prompt` and `negative_prompt_embeds`.")
        if prompt_embeds is not None and negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                             f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")

    def prepare_latents(self, batch_size, num_channels_latents, video_length, height, width, dtype, device, generator,
                        latents=None):
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            latents = randn_tensor(shape, generator=generator, device=device, dtype=dtype)
        else:
            if tuple(latents.shape) != shape:
                raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {shape}")
            latents = latents.to(device=device, dtype=dtype)
        return latents * self.scheduler.init_noise_sigma

    def decode_latents(self, latents):
        """pipeline_videogen.py:422-429 (stock PyTorch-ROCm VAE; outside the latents/s metric)."""
        if self.vae is None:
            raise ValueError("no vae attached: use output_type='latent'")
        b, c, f, h, w = latents.shape
        frames = (latents / 0.18215).permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
        video = self.vae.decode(frames.to(next(self.vae.parameters()).dtype)).sample
        video = video.reshape(b, f, *video.shape[1:]).permute(0, 1, 3, 4, 2)
        return ((video / 2 + 0.5) * 255).add_(0.5).clamp_(0, 255).to(dtype=torch.uint8).cpu().contiguous()

    # ------------------------------------------------------------------ the denoise loop (662-689)
    @torch.no_grad()
    def denoise(self, latents: torch.Tensor, ctx: torch.Tensor, num_inference_steps: int, guidance_scale: float,
                generator=None, callback: Optional[Callable] = None, callback_steps: int = 1, eta: float = 0.0,
                known: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                known_noise: Optional[torch.Tensor] = None, start_step: int = 0, window_length: Optional[int] = None,
                window_stride: Optional[int] = None, window_weights: str = "triangle",
                guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                pag_applied_layers=("mid_block",), cache_interval: Optional[int] = None, cache_depth: int = 1,
                free_init=None) -> torch.Tensor:
        """latents fp32 [P, C, F, h, w] on the device, ctx fp16 [2P, n, d] = [negative | prompt] (guidance_scale > 1) or
        [P, n, d] = prompt only (guidance_scale <= 1: no classifier-free guidance, :626) -> denoised fp32.  One loop, one step
        launch per denoising step: the loop and its buffers are lavie_amd.sampling's (`Run`), which features combine is
        `sampling.check_features`'s; what is this pipeline's own are the context, the PAG setting and the order of the sessions.

        `guidance_scale` may be a sequence with one value > 1 per latent; `guidance_rescale` = phi in (0, 1] rescales every
        latent's guided prediction to phi std(prompt prediction) / std(guided prediction) + (1 - phi) (diffusers'
        rescale_noise_cfg; ignored without guidance).  Either one adds the two small launches of `ops.guidance_table` in front of
        the step, which then reads scale and factor per latent from device memory (`sampling.GuidanceTable`); a windowed step
        rescales each window's prediction from that window's own statistics before the windows are averaged.

        Around known latents (the known-region replacement of diffusers' legacy inpaint / img2img loop): `known` are clean
        latents shaped as `latents`.  After every step the step kernel itself overwrites the part `mask` pins (1 = keep `known`,
        0 = free, [P, 1, F, h, w] or broadcastable to it) with `known` re-noised to the level the step just reached,
        x_t = a known + s known_noise, and the last step lands on `known` itself.  `known_noise` is ONE tensor for the whole run
        (drawn from `generator` before the loop when not given).  start_step = 0: x starts as `latents` with the pinned part
        replaced.  start_step > 0 (a run at reduced strength): the loop runs timesteps[start_step:] and x starts as `known`
        noised to timesteps[start_step] everywhere, `latents` only gives the shape.  mask = None pins nothing during the steps
        (plain img2img).

        Frame windows, for a clip longer than the model's window (MultiDiffusion along the frame axis): with `window_length`
        below F, ONE latent tensor holds all F frames; per step the UNet runs on every window of `window_length` frames (starts 0,
        stride, 2 stride, ..., the last one clamped to the clip's end: lavie_amd.windows), then ONE launch (ops.window_step)
        averages the windows' noise predictions per frame with the normalised `window_weights` profile, advances the whole clip
        by one scheduler step and writes every window's next fp16 model input.  `window_stride` defaults to three quarters of the
        window.  A frame that one window covers gets the plain step's bits.  The engine is prepared and the context cached once,
        for the window shape; the step's own noise is drawn for the whole clip.

        Perturbed-attention guidance (Ahn et al.; diffusers' AnimateDiffPAGPipeline): with `pag_scale` > 0 one more copy of the
        prompt-conditioned latents rides in the batch, ctx = [negative | prompt | prompt] ([3P, n, d]; [prompt | prompt] without
        classifier-free guidance), and in the transformers `pag_applied_layers` selects (state-dict prefixes, `UNet.set_pag`) the
        spatial self-attention of that last part is the identity on values.  The step folds the third prediction in,
        eps = e_cfg + s_t (eps_prompt - eps_perturbed), s_t = max(pag_scale - pag_adaptive_scale (1000 - t), 0), in the one launch
        (ops.cfg_pag_sampler_step and kin).  The UNet's PAG setting is made for the loop and restored afterwards, also after an
        exception.  Not combined with known latents, frame windows, `guidance_rescale` > 0 or a `guidance_scale` sequence; at most
        2 prompts per call with guidance, 4 without (the engine's batch limit of 8).  pag_scale = 0 is the call without it.

        Layer cache (DeepCache; `UNet.enable_layer_cache`): with `cache_interval` = N > 1 the whole UNet runs on the executed steps
        0, N, 2N, ... (the first step a run takes always refreshes, also when `start_step` > 0) and the steps between run only the
        first `cache_depth` layers of the first down block and the last `cache_depth` + 1 of the last up block on the activation the
        latest full step left.  An approximation whose quality at a given N is the caller's trade-off.  The UNet's own setting
        comes back after the loop.  Not combined with frame windows.  None or 1 is the call without it.

        FreeInit (Wu et al.; diffusers' enable_free_init; lavie_amd.free_init): with `free_init` (a FreeInit or a mapping of its
        keywords) of num_iters = N > 1 the loop runs N times inside ONE engine session, on the same buffers.  Between two
        iterations one call of ops.freq_mix re-noises the result to the last training timestep with the noise the call started
        from (`latents` = init_noise_sigma e0), keeps its low spatio-temporal frequencies, takes the high ones from fresh noise
        drawn from `generator`, and writes the next iteration's fp32 latents and fp16 model input itself (with frame windows the
        filter spans the whole clip and every window's input is then cut from the mixed clip as at the start of a run).  Every
        iteration starts at position 0 of its own timestep table (`use_fast_sampling`: FreeInit.steps_at steps), so a multistep
        history and the layer cache restart with it, and `callback`'s step index restarts as well.  Not combined with known
        latents: the run's start is not noise there.  None or num_iters = 1 is the call without it, launch for launch."""
        free, cache_interval, pag = sampling.check_features(
            self.DENOISE, latents.shape[2], latents.shape[0], known=dict(known=known, mask=mask, known_noise=known_noise),
            late_start=start_step != 0, window_length=window_length, guidance=(guidance_scale, guidance_rescale),
            pag=(pag_scale, pag_adaptive_scale), cache=(cache_interval, cache_depth),
            free_init=free_init if free_init is not None else self.free_init, unipc=bool(getattr(self.scheduler, "unipc", False)))
        geometry = sampling.window_geometry(latents.shape[2], window_length, window_stride, window_weights)
        if known is None and (mask is not None or known_noise is not None or start_step != 0):
            raise ValueError("`mask`, `known_noise` and `start_step` need `known` latents")

        def plan_at(iteration):                            # every FreeInit iteration has a plan of its own (`use_fast_sampling`)
            return sampling.StepPlan(self.scheduler, free.steps_at(iteration, num_inference_steps) if free else num_inference_steps, eta)
        plan = plan_at(0)
        if known is not None and not 0 <= start_step < len(plan.timesteps):
            raise ValueError(f"`start_step`={start_step} must lie in 0..{len(plan.timesteps) - 1}")
        # None, the scalar itself, or the table route with its buffers, allocated here once for the loop
        guidance = sampling.guidance_of(guidance_scale, guidance_rescale, latents, geometry.frames, len(geometry.starts))
        p = latents.shape[0]
        nb = p * ((2 if guidance is not None else 1) + (1 if pag else 0))      # [negative |] prompt [| perturbed]  (:666)
        if ctx.shape[0] != nb:
            raise ValueError(f"ctx has {ctx.shape[0]} rows, expected {nb} for {p} latents at guidance_scale={guidance_scale}" +
                             (f", pag_scale={pag_scale}" if pag else ""))
        run = sampling.Run(latents, geometry, plan, guidance, nb, generator, pag=(pag_scale, pag_adaptive_scale) if pag else None,
                           known=(known, mask, known_noise, start_step) if known is not None else None, cache_interval=cache_interval)
        if free is not None:                                # the state of the iterations, beside the run's buffers
            run.free = free_init_mod.FreeInitRun(free, self.scheduler, run.x, generator, plan_at)
        run.fill(plan.input_scale(start_step))
        # with guidance the two halves of every model input are the same latents (one fp16 value written into both by the loop's
        # own step kernel, pinned or not, windowed or not): the engine may compute the layers in front of the first text
        # cross-attention once
        shared = run.model_in if run.guided and self.cfg_shared_prefix and not pag else None
        pag_was = self.unet.pag if pag else None           # the model's own setting comes back after the loop, whatever happens in it
        try:
            if pag:
                self.unet.set_pag(pag_applied_layers, p)
            with sampling.layer_cache_session(self.unet, cache_interval, cache_depth), \
                    sampling.engine_session(self.unet, run.batch, run.frames, *run.x.shape[3:], ctx, shared) as ctx:
                def forward(w, i, layer_cache_mode):                                                         # line 670
                    return self.unet(run.model_in[w], run.t_dev[i], encoder_hidden_states=ctx,
                                     **sampling.forward_keywords(layer_cache_mode)).sample
                return run.loop(forward, callback, callback_steps)
        finally:
            if pag_was is not None:
                self.unet.set_pag(*pag_was)

    @staticmethod
    def check_pag(pag_scale, pag_adaptive_scale, prompts: int, guidance_scale, guidance_rescale, **others) -> bool:
        """The perturbed-attention-guidance arguments of a call on `prompts` latents -> whether PAG is on (pag_scale > 0).  `others`:
        the call's arguments PAG is not combined with, by name (None = absent).  Raises before anything reaches the engine.
        (sampling.check_features, with PAG as the only feature judged.)"""
        return sampling.check_features(sampling.Surface(("pag",)), 0, prompts, known=others, guidance=(guidance_scale, guidance_rescale),
                                       pag=(pag_scale, pag_adaptive_scale))[2]

    @staticmethod
    def strength_start(num_inference_steps: int, strength: float) -> int:
        """First position of the timestep table a run at `strength` in (0, 1] takes: steps - int(steps * strength), the img2img
        rule; at least one step always runs."""
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"`strength` must lie in (0, 1] but is {strength}")
        return min(num_inference_steps - int(num_inference_steps * strength), num_inference_steps - 1)

    def check_known_inputs(self, known_latents, known_mask, video, strength, shape):
        """The arguments of sampling around known latents, against the latent `shape` [P, C, F, h, w] of the call."""
        if not isinstance(strength, (int, float)) or not 0.0 < strength <= 1.0:
            raise ValueError(f"`strength` must lie in (0, 1] but is {strength}")
        if video is not None and known_latents is not None:
            raise ValueError("Cannot forward both `video` and `known_latents`. Please make sure to only forward one of the two.")
        have = video is not None or known_latents is not None
        if known_mask is not None and not have:
            raise ValueError("`known_mask` needs `known_latents` or `video`: there is nothing to keep.")
        if strength < 1.0 and not have:
            raise ValueError("`strength` < 1 needs `known_latents` or `video` to start from.")
        if known_latents is not None and tuple(known_latents.shape) != tuple(shape):
            raise ValueError(f"Unexpected `known_latents` shape, got {tuple(known_latents.shape)}, expected {tuple(shape)}")
        if video is not None:
            p, _, f, h, w = shape
            k = self.vae_scale_factor
            pixels = ((p, f, h * k, w * k, 3), (p, 3, f, h * k, w * k))
            want = pixels[0] if video.dtype == torch.uint8 else pixels[1]
            if not (video.dtype == torch.uint8 or video.is_floating_point()) or tuple(video.shape) != want:
                raise ValueError(f"`video` must be uint8 {pixels[0]} or float {pixels[1]} in [-1, 1], got {video.dtype} "
                                 f"{tuple(video.shape)}")
            if self.vae is None:
                raise ValueError("no vae attached: pass `known_latents` instead of `video`")
        if known_mask is not None:
            want = (shape[0], 1) + tuple(shape[2:])
            try:
                ok = known_mask.dim() == 5 and tuple(torch.broadcast_shapes(tuple(known_mask.shape), want)) == want
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError(f"`known_mask` must be broadcastable to {want}, got {tuple(known_mask.shape)}")
            if not bool(((known_mask >= 0) & (known_mask <= 1)).all()):
                raise ValueError("`known_mask` values must lie in [0, 1] (1 keeps the known latents, 0 is free)")

    def encode_video(self, video: torch.Tensor) -> torch.Tensor:
        """Pixels [P, F, H, W, 3] uint8 or [P, 3, F, H, W] float in [-1, 1] -> latents [P, 4, F, H/8, W/8] fp32: the posterior
        mode of `self.vae`, times 0.18215 (the inverse of decode_latents)."""
        if video.dtype == torch.uint8:
            video = video.permute(0, 4, 1, 2, 3).float() / 127.5 - 1.0
        b, c, f, h, w = video.shape
        param = next(self.vae.parameters())
        frames = video.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w).to(device=param.device, dtype=param.dtype)
        lat = torch.cat([self.vae.encode(frames[i:i + 8]).latent_dist.mode() for i in range(0, b * f, 8)], dim=0) * 0.18215
        return lat.reshape(b, f, *lat.shape[1:]).permute(0, 2, 1, 3, 4).float().contiguous()

    # keywords of `__call__` that only mean something in a sampling run: `denoising_loss` refuses them by name
    SAMPLING_ONLY = {"window_length": "frame windows", "window_stride": "frame windows", "window_weights": "frame windows",
                     "known_latents": "known latents", "known_mask": "known latents", "strength": "known latents",
                     "pag_scale": "perturbed-attention guidance", "pag_adaptive_scale": "perturbed-attention guidance",
                     "pag_applied_layers": "perturbed-attention guidance", "cache_interval": "the layer cache",
                     "cache_depth": "the layer cache", "free_init": "FreeInit"}

    @torch.no_grad()
    def denoising_loss(self, video: Optional[torch.Tensor] = None, latents: Optional[torch.Tensor] = None, prompt=None,
                       prompt_embeds: Optional[torch.Tensor] = None, image_tensor=None, image_embeds: Optional[torch.Tensor] = None,
                       timesteps=None, seed=0, snr_gamma=None, noise_offset: float = 0.0, prediction_type=None, **sampling_only):
        """The training objective evaluated forward on held-out clips (lavie_amd.denoising_loss.DenoisingLoss.evaluate): the clips are
        encoded as `encode_video` does (or `latents` [P, 4, F, h, w], already scaled, are taken), the context comes from the paths
        `__call__` uses (prompt or prompt_embeds, widened by the mapper when one is attached and an image is given; one prompt serves
        every clip), noise of `seed` (an int, a list with one per clip, or a PhiloxGenerator) is added at `timesteps` (one int, or one
        per clip) and the UNet's prediction is scored against the target.  The active LoRA adapters and scales apply: the engine serves
        them merged.  No guidance is involved.  Options of a sampling run (frame windows, known latents, PAG, the layer cache,
        FreeInit) are refused by name."""
        from .denoising_loss import DenoisingLoss
        from .noise import PhiloxGenerator
        for name in sampling_only:
            if name not in self.SAMPLING_ONLY:
                raise TypeError(f"denoising_loss() got an unexpected keyword argument {name!r}")
            raise ValueError(f"denoising_loss: `{name}` ({self.SAMPLING_ONLY[name]}) only means something in a sampling run")
        if (video is None) == (latents is None):
            raise ValueError("denoising_loss: pass exactly one of `video` and `latents`")
        if (prompt is None) == (prompt_embeds is None):
            raise ValueError("denoising_loss: pass exactly one of `prompt` and `prompt_embeds`")
        if timesteps is None:
            raise ValueError("denoising_loss: `timesteps` is required (one int, or one per clip)")
        device = self.device
        x0 = self.encode_video(video) if video is not None else latents
        x0 = x0.to(device=device).contiguous()
        image_features = self._image_features(image_tensor, image_embeds, device) if self.mapper is not None else None
        ctx = self._encode_prompt(prompt, device, 1, False, None, prompt_embeds, None, image_features).to(torch.float16).contiguous()
        generator = seed if isinstance(seed, PhiloxGenerator) else PhiloxGenerator(seed)
        scorer = DenoisingLoss(self.unet, self.scheduler, snr_gamma=snr_gamma, noise_offset=noise_offset, prediction_type=prediction_type)
        return scorer.evaluate(x0, ctx, timesteps, generator)

    @contextlib.contextmanager
    def _lora_scale(self, scale):
        """diffusers' LoRA strength (`cross_attention_kwargs["scale"]`) for one call only, restored also on an exception; None
        leaves the UNet alone."""
        if scale is None:
            yield
            return
        was = self.unet.lora_scale
        self.unet.set_lora_scale(scale)
        try:
            yield
        finally:
            self.unet.set_lora_scale(was)

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, image_tensor=None, height: Optional[int] = None,
                 width: Optional[int] = None, video_length: int = 16, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: Optional[str] = "pil", return_dict: bool = True, callback=None, callback_steps: int = 1,
                 cross_attention_kwargs=None, image_embeds: Optional[torch.Tensor] = None,
                 known_latents: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None,
                 video: Optional[torch.Tensor] = None, strength: float = 1.0, window_length: Optional[int] = None,
                 window_stride: Optional[int] = None, window_weights: str = "triangle", guidance_rescale: float = 0.0,
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, pag_applied_layers=("mid_block",),
                 cache_interval: Optional[int] = None, cache_depth: int = 1, free_init=None):
        """`free_init`: a FreeInit (or a mapping of its keywords) for this call instead of the pipeline's own setting
        (enable_free_init); not with `known_latents` / `known_mask` / `video` / `strength` < 1.
        `guidance_scale`: one number, or a sequence with one value > 1 per prompt (repeated per `num_images_per_prompt`; a
        sequence always means guidance is on).  `guidance_rescale` in [0, 1]: diffusers' rescale_noise_cfg inside the fused step;
        ignored with a scalar `guidance_scale` <= 1, as in diffusers.  `pag_scale` > 0: perturbed-attention guidance in the
        transformers `pag_applied_layers` names, fading by `pag_adaptive_scale` per timestep below 1000.  `cache_interval` = N > 1: the layer cache, the whole UNet on every
        N-th step only, at `cache_depth`; not with `window_length`.  See `denoise`."""
        judged = dict(known=dict(known_latents=known_latents, video=video, known_mask=known_mask), late_start=strength != 1.0,
                      window_length=window_length, guidance=(guidance_scale, guidance_rescale), pag=(pag_scale, pag_adaptive_scale),
                      cache=(cache_interval, cache_depth), free_init=free_init if free_init is not None else self.free_init,
                      unipc=bool(getattr(self.scheduler, "unipc", False)))
        sampling.check_features(self.CALL, video_length, **judged)
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds)
        batch_size = 1 if isinstance(prompt, str) else len(prompt) if prompt is not None else prompt_embeds.shape[0]
        device = self.device
        # PAG's count needs the prompts, so it is judged here, behind `check_inputs`, as it always was
        pag = sampling.check_features(self.CALL_PAG, video_length, batch_size * (num_images_per_prompt or 1), **judged)[2]
        do_cfg, scales, guidance_rescale = sampling.check_guidance(guidance_scale, guidance_rescale, batch_size,
                                                                   num_images_per_prompt or 1)
        if scales is not None:
            guidance_scale = scales                # one value per latent
        # image conditioning only with a mapper attached; without one the image is ignored, as the upstream pipeline does
        image_features = self._image_features(image_tensor, image_embeds, device) if self.mapper is not None else None
        ctx = self._encode_prompt(prompt, device, num_images_per_prompt, do_cfg, negative_prompt, prompt_embeds,
                                  negative_prompt_embeds, image_features).to(torch.float16).contiguous()
        if pag:                                # [negative | prompt | prompt] or [prompt | prompt]: the last part rides perturbed
            ctx = torch.cat([ctx, ctx[-(ctx.shape[0] // (2 if do_cfg else 1)):]]).contiguous()
        latents = self.prepare_latents(batch_size * num_images_per_prompt, self.unet.config.in_channels, video_length,
                                       height, width, torch.float32, device, generator, latents)
        # sampling around known latents (pinned frames, video-to-video, clip continuation): `denoise(known=)`
        self.check_known_inputs(known_latents, known_mask, video, strength, latents.shape)
        features = {}                          # a feature's keywords reach `denoise` only when the feature is on: absent = the call without it
        if video is not None or known_latents is not None:
            known = self.encode_video(video) if video is not None else known_latents
            features.update(known=known.to(device=device, dtype=torch.float32), mask=known_mask,
                            start_step=self.strength_start(num_inference_steps, strength))
        elif window_length is not None:    # clips longer than the window: overlapping frame windows
            features.update(window_length=window_length, window_stride=window_stride, window_weights=window_weights)
        if guidance_rescale:
            features.update(guidance_rescale=guidance_rescale)
        if pag:
            features.update(pag_scale=pag_scale, pag_adaptive_scale=pag_adaptive_scale, pag_applied_layers=pag_applied_layers)
        if cache_interval not in (None, 1):
            features.update(cache_interval=cache_interval, cache_depth=cache_depth)
        if free_init is not None:              # (the pipeline's own setting is read by `denoise` itself)
            features.update(free_init=free_init)
        with self._lora_scale((cross_attention_kwargs or {}).get("scale")):
            latents = self.denoise(latents, ctx, num_inference_steps, guidance_scale, generator, callback, callback_steps, eta, **features)
        video = latents if output_type == "latent" else self.decode_latents(latents)
        if not return_dict:
            return (video,)
        return StableDiffusionPipelineOutput(video=video)
