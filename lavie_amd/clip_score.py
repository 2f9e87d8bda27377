"""CLIP image processor and CLIPSIM scoring on the engine.

`HipCLIPImageProcessor` stands where a pipeline expects `clip_processor`: `proc(images=x, return_tensors="pt").pixel_values` is the
stock `CLIPImageProcessor`'s tensor bit for bit (fp32), made on the device from uint8 pixels by `ops.clip_preprocess`.
`ClipScorer` is `CLIPModel`'s scoring surface over the engine towers: `get_text_features`, `get_image_features`,
`logits_per_image`, and `score` / `rank` for CLIPSIM, the mean over a clip's frames of 100 cos(image features, text features).
The tokenizer stays stock.  Two calls agree bit for bit, and an image's or a prompt's features do not depend on the batch."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .image_encoder import HipCLIPVisionModel
from .text_encoder import HipCLIPTextModel

BICUBIC = 3          # PIL.Image.Resampling.BICUBIC, the only filter built


def _edge(value, names, what):
    """224, {"shortest_edge": 224}, {"height": 224, "width": 224}, SizeDict -> 224"""
    if value is None:
        raise ValueError(f"HipCLIPImageProcessor: the stock processor has no {what}")
    if isinstance(value, (int, np.integer)):
        return int(value)
    get = value.get if isinstance(value, dict) else lambda k, d=None: getattr(value, k, d)
    found = [int(get(k)) for k in names if get(k) is not None]
    if not found or any(v != found[0] for v in found):
        raise ValueError(f"HipCLIPImageProcessor: {what}={value!r} is not one edge (a shortest-edge resize and a square crop are built)")
    return found[0]


class HipCLIPImageProcessor:
    def __init__(self, size=224, crop_size=224, image_mean=ops.CLIP_MEAN, image_std=ops.CLIP_STD, dtype=torch.float32, device="cuda"):
        self.size, self.crop_size = _edge(size, ("shortest_edge",), "size"), _edge(crop_size, ("height", "width"), "crop_size")
        self.image_mean, self.image_std = tuple(float(v) for v in image_mean), tuple(float(v) for v in image_std)
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise ValueError("HipCLIPImageProcessor: image_mean and image_std have three entries")
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"HipCLIPImageProcessor: dtype {dtype} is not fp32 or fp16")
        self.dtype, self.device = dtype, torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("HipCLIPImageProcessor lives on a HIP device")
        self._stock = None

    @classmethod
    def from_stock(cls, processor, dtype=torch.float32, device="cuda"):
        """A transformers CLIPImageProcessor of the usual kind: bicubic shortest-edge resize, centre crop, 1 / 255, normalise."""
        for switch in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
            if getattr(processor, switch, True) is False:
                raise ValueError(f"HipCLIPImageProcessor: `{switch}=False` is not built (the four steps always run)")
        resample = getattr(processor, "resample", BICUBIC)
        if resample is not None and int(resample) != BICUBIC:
            raise ValueError(f"HipCLIPImageProcessor: resample={resample!r} is not built (bicubic only)")
        factor = getattr(processor, "rescale_factor", 1 / 255)
        if factor is not None and float(factor) != 1 / 255:
            raise ValueError(f"HipCLIPImageProcessor: rescale_factor={factor!r} is not built (1 / 255 only)")
        self = cls(size=processor.size, crop_size=processor.crop_size, image_mean=processor.image_mean, image_std=processor.image_std,
                   dtype=dtype, device=device)
        self._stock = processor
        return self

    def _pixels(self, images):
        """-> uint8 [B, H, W, 3] on the device, one upload for inputs of equal size"""
        if isinstance(images, (list, tuple)):
            if not images:
                raise ValueError("HipCLIPImageProcessor: empty list of images")
            arrays = [np.asarray(im.convert("RGB")) if hasattr(im, "convert") else (im.cpu().numpy() if torch.is_tensor(im) else np.asarray(im))
                      for im in images]
            if any(a.ndim != 3 for a in arrays):
                raise ValueError("HipCLIPImageProcessor: a list holds single images [H, W, 3]")
            if any(a.shape != arrays[0].shape for a in arrays):
                raise ValueError(f"HipCLIPImageProcessor: mixed sizes {sorted({a.shape for a in arrays})[:3]} in one call are not built: "
                                 "call once per size")
            images = np.stack(arrays)
        elif hasattr(images, "convert"):
            images = np.asarray(images.convert("RGB"))
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images))
        if not torch.is_tensor(images):
            raise ValueError(f"HipCLIPImageProcessor: {type(images).__name__} is not a tensor, an array, a PIL image or a list of them")
        if images.dtype != torch.uint8:
            raise ValueError(f"HipCLIPImageProcessor: {images.dtype} pixels are not built: pass uint8 (float inputs would need the stock "
                             "processor's own rounding to bytes)")
        if images.dim() == 3:
            images = images[None]
        if images.dim() != 4:
            raise ValueError(f"HipCLIPImageProcessor: images must be [H, W, 3], [B, H, W, 3] or [B, 3, H, W], got {tuple(images.shape)}")
        last, first = images.shape[-1] == 3, images.shape[1] == 3
        if last and first:
            raise ValueError(f"HipCLIPImageProcessor: {tuple(images.shape)} has three entries on axis 1 and on the last axis: the layout "
                             "is ambiguous (and either edge of 3 is below the short edge the resize takes)")
        if not last and not first:
            raise ValueError(f"HipCLIPImageProcessor: no axis of three channels in {tuple(images.shape)}")
        if first:
            images = images.permute(0, 2, 3, 1)
        return images.to(self.device).contiguous()

    def __call__(self, images=None, return_tensors="pt", **kwargs):
        extra = [k for k, v in kwargs.items() if v is not None]
        if extra:
            raise ValueError(f"HipCLIPImageProcessor: per-call overrides {extra} are not built: configure the object")
        if return_tensors not in ("pt", None):
            raise ValueError(f"HipCLIPImageProcessor: return_tensors={return_tensors!r} is not built (device tensors only)")
        px = ops.clip_preprocess(self._pixels(images), self.size, self.crop_size, self.image_mean, self.image_std, dtype=self.dtype)
        return SimpleNamespace(pixel_values=px)

    preprocess = __call__


class ClipScorer:
    MAX_BATCH = 16            # images / prompts per tower call

    def __init__(self, state_dict, config, device="cuda", processor=None):
        """state_dict: CLIPModel.state_dict(); config: CLIPConfig or a dict with text_config, vision_config (dicts of the towers'
        fields) and projection_dim."""
        get = config.get if isinstance(config, dict) else lambda k, d=None: getattr(config, k, d)
        tcfg, vcfg = get("text_config"), get("vision_config")
        if tcfg is None or vcfg is None:
            raise ValueError("ClipScorer: the config needs text_config and vision_config")
        tget = tcfg.get if isinstance(tcfg, dict) else lambda k, d=None: getattr(tcfg, k, d)
        vget = vcfg.get if isinstance(vcfg, dict) else lambda k, d=None: getattr(vcfg, k, d)
        self.device = torch.device(device)
        sd = state_dict
        for k in ("visual_projection.weight", "text_projection.weight", "logit_scale", "vision_model.post_layernorm.weight",
                  "vision_model.post_layernorm.bias"):
            if k not in sd:
                raise ValueError(f"ClipScorer: the state dict lacks {k}")
        self.text = HipCLIPTextModel({k: v for k, v in sd.items() if k.startswith("text_model.")}, tcfg, device=device)
        self.vision = HipCLIPVisionModel({k: v for k, v in sd.items() if k.startswith("vision_model.")}, vcfg, device=device)
        half = lambda k: sd[k].detach().to(device=self.device, dtype=torch.float16).contiguous()
        f32 = lambda k: sd[k].detach().to(device=self.device, dtype=torch.float16).float().contiguous()      # the fp16 values, as the towers'
        self.visual_projection, self.text_projection = half("visual_projection.weight"), half("text_projection.weight")
        self.post_ln_weight, self.post_ln_bias = f32("vision_model.post_layernorm.weight"), f32("vision_model.post_layernorm.bias")
        self.logit_scale = float(sd["logit_scale"])
        self.eos_token_id = int(tget("eos_token_id", 2) if tget("eos_token_id", 2) is not None else 2)
        self.eps = float(vget("layer_norm_eps", 1e-5) or 1e-5)
        self.image_size = int(vget("image_size"))
        if self.visual_projection.shape[0] != self.text_projection.shape[0]:
            raise ValueError("ClipScorer: the two projections differ in their output width")
        self.processor = processor or HipCLIPImageProcessor(size=self.image_size, crop_size=self.image_size, device=device)
        self._stock = None

    @classmethod
    def from_stock(cls, clip_model, device=None, processor=None):
        dev = device or next(clip_model.parameters()).device
        if torch.device(dev).type != "cuda":
            dev = "cuda"
        if processor is not None and not isinstance(processor, HipCLIPImageProcessor):
            processor = HipCLIPImageProcessor.from_stock(processor, device=dev)
        self = cls(clip_model.state_dict(), clip_model.config, device=dev, processor=processor)
        self._stock = clip_model
        return self

    @classmethod
    def from_state_dict(cls, sd, config_dict, device="cuda", processor=None):
        return cls(sd, config_dict, device=device, processor=processor)

    # ------------------------------------------------------------------ features
    @torch.no_grad()
    def get_text_features(self, input_ids, normalize=False):
        """fp32 [B, D]: text_projection of the pooled row (CLIPModel.get_text_features); normalize: divided by its L2 norm"""
        out = torch.empty((input_ids.shape[0], self.text_projection.shape[0]), dtype=torch.float32, device=self.device)
        for b0 in range(0, input_ids.shape[0], self.MAX_BATCH):
            ids = input_ids[b0:b0 + self.MAX_BATCH]
            ops.clip_embed(self.text(ids).last_hidden_state, self.text_projection, ids=ids, eos_token_id=self.eos_token_id,
                           normalize=normalize, out=out[b0:b0 + ids.shape[0]])
        return out

    @torch.no_grad()
    def get_image_features(self, pixel_values, normalize=False):
        """fp32 [B, D]: visual_projection of post_layernorm of the class row (CLIPModel.get_image_features)"""
        out = torch.empty((pixel_values.shape[0], self.visual_projection.shape[0]), dtype=torch.float32, device=self.device)
        for b0 in range(0, pixel_values.shape[0], self.MAX_BATCH):
            px = pixel_values[b0:b0 + self.MAX_BATCH]
            ops.clip_embed(self.vision(pixel_values=px).last_hidden_state, self.visual_projection, row=0, ln_weight=self.post_ln_weight,
                           ln_bias=self.post_ln_bias, eps=self.eps, normalize=normalize, out=out[b0:b0 + px.shape[0]])
        return out

    def _image_features_u8(self, pixels_u8):
        return self.get_image_features(self.processor(images=pixels_u8).pixel_values, normalize=True)

    @torch.no_grad()
    def logits_per_image(self, pixels_u8, input_ids):
        """fp32 [N, P] = exp(logit_scale) cos(image n, prompt p) (CLIPModel's logits_per_image) from uint8 pixels and token ids"""
        return ops.clip_similarity(self._image_features_u8(pixels_u8), self.get_text_features(input_ids, normalize=True),
                                   scale=math.exp(self.logit_scale))

    @torch.no_grad()
    def score(self, video_u8, input_ids):
        """CLIPSIM: video_u8 uint8 [P, F, H, W, 3], input_ids [P, L] -> fp32 [P], the mean over frames of 100 cos(frame, prompt)"""
        if not torch.is_tensor(video_u8) or video_u8.dtype != torch.uint8 or video_u8.dim() != 5 or video_u8.shape[-1] != 3:
            raise ValueError("ClipScorer.score: video_u8 must be a uint8 tensor [P, F, H, W, 3]")
        p, f = video_u8.shape[:2]
        if input_ids.shape[0] != p:
            raise ValueError(f"ClipScorer.score: {p} clips but {input_ids.shape[0]} prompts")
        img = self._image_features_u8(video_u8.reshape(p * f, *video_u8.shape[2:]))
        return ops.clip_similarity(img, self.get_text_features(input_ids, normalize=True), frames=f)

    def rank(self, video_u8, input_ids):
        """indices of the clips from the best score to the worst; equal scores keep their index order"""
        s = self.score(video_u8, input_ids).cpu()
        return sorted(range(s.numel()), key=lambda i: (-float(s[i]), i))
