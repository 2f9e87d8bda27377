"""Image conditioning on the engine (lavie_vision_* and lavie_mapper_* of include/lavie_hip.h).

`HipCLIPVisionModel` stands where the pipeline expects `clip_model` (or its `.vision_model`): `enc(pixel_values=px)` returns an
object with `.last_hidden_state` and `[0]`, the fp16 `[B, tokens, C]` hidden states WITHOUT `post_layernorm`, as transformers
defines `last_hidden_state`.  `HipMappingNetwork` stands where it expects `mapper`: `(image_embeds, text_embeds) -> [B, seq_out,
output_dim]` fp16, as `MappingNetwork.forward`.  Two calls agree bit for bit, and an image's or a prompt's block has the same bits at
every batch size and position in the batch.  Not built: the pooled output (`pooler_output`, `post_layernorm`), the projections of
`CLIPModel`, `output_hidden_states`, `output_attentions`, `interpolate_pos_encoding`, the image processor (resize / crop /
normalise stays the caller's `clip_processor`, as the tokenizer does)."""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib, ops
from ._engine_object import LastHiddenState, _EngineObject, _load, clip_config_dict, clip_layer_keys

ACTS = ops.ACT_KINDS                  # hidden_act -> lavie_vision_config.act
MAX_BATCH = 16                        # lavie_vision_encode, lavie_mapper_encode: 1 <= B <= 16
VISION_CONFIG_KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                      "hidden_act", "layer_norm_eps")
VISION_IGNORED = ("vision_model.embeddings.position_ids",      # a buffer of older transformers versions, not a weight
                  "vision_model.post_layernorm.weight", "vision_model.post_layernorm.bias")      # the pooled output's norm
MAPPER_IGNORED = ("text_proj.weight", "text_proj.bias")        # built and saved by the reference, unused by its forward


# ------------------------------------------------------------------ the vision tower
def vision_state_dict_keys(config: dict):
    """The keys the engine expects, in its order: those of CLIPVisionModel(config).state_dict() minus VISION_IGNORED."""
    v = "vision_model."
    return [v + "embeddings.class_embedding", v + "embeddings.patch_embedding.weight", v + "embeddings.position_embedding.weight",
            v + "pre_layrnorm.weight", v + "pre_layrnorm.bias"] + clip_layer_keys(v, config["num_hidden_layers"])


def normalize_vision_keys(sd: dict) -> dict:
    """The engine's names are the classic checkpoint keys, `vision_model.`-prefixed; transformers 5 builds CLIPVisionModel flat and
    its state_dict() drops the prefix.  Both spellings are taken; a CLIPModel's state dict keeps its vision tower's keys only."""
    out = {}
    for k, v in sd.items():
        if k.startswith(("text_model.", "visual_projection.", "text_projection.", "logit_scale")):
            continue
        k = k if k.startswith("vision_model.") else "vision_model." + k
        if k not in VISION_IGNORED:
            out[k] = v
    return out


def vision_config_dict(config) -> dict:
    """The eight fields the engine reads, from a transformers CLIPVisionConfig (or a CLIPConfig holding one) or a dict."""
    if not isinstance(config, dict) and getattr(config, "vision_config", None) is not None:
        config = config.vision_config
    return clip_config_dict(config, VISION_CONFIG_KEYS, "vision tower")


def vision_config_c(cfg: dict) -> "_lib.VisionConfigC":
    if cfg["hidden_act"] not in ACTS:
        raise ValueError(f"hidden_act {cfg['hidden_act']!r} is not built: the engine has {sorted(ACTS)}")
    c = _lib.VisionConfigC()
    c.struct_size = ctypes.sizeof(_lib.VisionConfigC)
    c.hidden, c.intermediate, c.layers = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["num_hidden_layers"])
    c.heads, c.image_size, c.patch_size = int(cfg["num_attention_heads"]), int(cfg["image_size"]), int(cfg["patch_size"])
    c.act, c.eps = ACTS[cfg["hidden_act"]], float(cfg["layer_norm_eps"])
    return c


class VisionEncoderOutput(LastHiddenState):
    """`out[0]` and `out.last_hidden_state`, as the stock model's output offers them; the pooled output is not built."""

    @property
    def pooler_output(self):
        raise NotImplementedError("HipCLIPVisionModel: `pooler_output` is not built (post_layernorm of the class token belongs to "
                                  "the pooled output; the mapper reads last_hidden_state)")


class HipCLIPVisionModel(_EngineObject):
    _destroy = "lavie_vision_destroy"

    def __init__(self, state_dict, config, device="cuda"):
        """state_dict: CLIPVisionModel.state_dict() or CLIPModel.state_dict() (any float dtype; rounded to fp16 here); config:
        CLIPVisionConfig, CLIPConfig or dict."""
        self._cfg = vision_config_dict(config)
        self.config = config if not isinstance(config, dict) else SimpleNamespace(**config)
        self.device = torch.device(device)
        self.dtype = torch.float16
        self._stock = None                 # the object from_stock wrapped (VideoGenPipeline.disable_engine_image_encoder hands it back)
        self._h = None
        c = vision_config_c(self._cfg)
        if self.device.type != "cuda":
            raise ValueError("HipCLIPVisionModel lives on a HIP device")
        lib = _lib.load()
        sd = normalize_vision_keys(state_dict)
        want = vision_state_dict_keys(self._cfg)
        if set(sd) != set(want):
            raise ValueError(f"state dict does not match the config: missing {sorted(set(want) - set(sd))[:4]}, "
                             f"unexpected {sorted(set(sd) - set(want))[:4]}")
        h = ctypes.c_void_p()
        _lib.check(lib.lavie_vision_create(ctypes.byref(c), ctypes.byref(h)), "lavie_vision_create")
        self._h = h
        _load(lib, "lavie_vision", h, want, sd, self.device)

    @classmethod
    def from_stock(cls, clip_model_or_vision_model, device=None):
        """A transformers CLIPModel (its vision tower is taken), CLIPVisionModel or CLIPVisionTransformer."""
        m = clip_model_or_vision_model
        tower = getattr(m, "vision_model", m)
        dev = device or next(tower.parameters()).device
        if torch.device(dev).type != "cuda":
            dev = "cuda"
        self = cls(tower.state_dict(), m.config, device=dev)
        self._stock = m
        return self

    @classmethod
    def from_state_dict(cls, sd, config_dict, device="cuda"):
        return cls(sd, config_dict, device=device)

    @property
    def vision_model(self):
        """A CLIPModel-shaped lookup (`clip_model.vision_model`) finds the tower: the object itself."""
        return self

    @property
    def tokens(self):
        return 1 + (self._cfg["image_size"] // self._cfg["patch_size"]) ** 2

    def workspace_bytes(self, b):
        n = _lib.load().lavie_vision_workspace_bytes(self._h, b)
        if n < 0:
            _lib.check(-1, "lavie_vision_workspace_bytes")
        return n

    @torch.no_grad()
    def __call__(self, pixel_values=None, output_attentions=None, output_hidden_states=None, interpolate_pos_encoding=None, **kwargs):
        for name, val in (("output_attentions", output_attentions), ("output_hidden_states", output_hidden_states),
                          ("interpolate_pos_encoding", interpolate_pos_encoding)):
            if val is not None and val is not False:
                raise NotImplementedError(f"HipCLIPVisionModel: `{name}` is not built (per-layer outputs and resized position tables "
                                          "are outside the engine tower)")
        extra = [k for k, v in kwargs.items() if v is not None and v is not False and k != "return_dict"]
        if extra:
            raise NotImplementedError(f"HipCLIPVisionModel: {extra} not built")
        s = self._cfg["image_size"]
        if pixel_values is None or pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
            raise ValueError("pixel_values must be a [B, 3, S, S] tensor")
        if tuple(pixel_values.shape[2:]) != (s, s):
            raise ValueError(f"pixel_values: image size {tuple(pixel_values.shape[2:])} is not the config's ({s}, {s}); "
                             "interpolated position tables are not built")
        if pixel_values.shape[0] < 1:
            raise ValueError("pixel_values: empty batch")
        if pixel_values.dtype not in (torch.float16, torch.float32):
            pixel_values = pixel_values.float()
        lib = _lib.load()
        b = pixel_values.shape[0]
        with torch.cuda.device(self.device):
            px = pixel_values.to(device=self.device).contiguous()
            flag = 1 if px.dtype == torch.float32 else 0
            out = torch.empty((b, self.tokens, self._cfg["hidden_size"]), dtype=torch.float16, device=self.device)
            for b0 in range(0, b, MAX_BATCH):          # an image's bits do not depend on the batch around it: chunks are exact
                n = min(MAX_BATCH, b - b0)
                _lib.check(lib.lavie_vision_encode(self._h, ctypes.c_void_p(px[b0:b0 + n].data_ptr()), flag, n,
                                                   ctypes.c_void_p(out[b0:b0 + n].data_ptr()), ops._stream()), "lavie_vision_encode")
        return VisionEncoderOutput(out)


# ------------------------------------------------------------------ the mapper
def mapper_state_dict_keys(layers: int):
    """The keys the engine expects, in its order: those of MappingNetwork.state_dict() minus MAPPER_IGNORED."""
    keys = ["image_pos_embedding", "text_pos_embedding", "image_proj.weight", "image_proj.bias"]
    for i in range(layers):
        p = f"transformer_decoder.layers.{i}."
        for att in ("self_attn", "multihead_attn"):
            keys += [f"{p}{att}.in_proj_weight", f"{p}{att}.in_proj_bias", f"{p}{att}.out_proj.weight", f"{p}{att}.out_proj.bias"]
        keys += [f"{p}linear1.weight", f"{p}linear1.bias", f"{p}linear2.weight", f"{p}linear2.bias"]
        for n in ("norm1", "norm2", "norm3"):
            keys += [f"{p}{n}.weight", f"{p}{n}.bias"]
    return keys


def mapper_config_from_state_dict(sd: dict, num_heads: int, eps: float = 1e-5) -> dict:
    """Widths, lengths and the layer count are read off the tensors; the head count is not recorded in them."""
    for k in ("image_proj.weight", "image_pos_embedding", "text_pos_embedding"):
        if k not in sd:
            raise ValueError(f"mapper checkpoint: missing key {k!r}")
    output_dim, input_dim = sd["image_proj.weight"].shape
    layers = {int(k.split(".")[2]) for k in sd if k.startswith("transformer_decoder.layers.")}
    if not layers:
        raise ValueError("mapper checkpoint: no transformer_decoder layers")
    return dict(input_dim=int(input_dim), output_dim=int(output_dim), layers=max(layers) + 1, heads=int(num_heads),
                dim_feedforward=int(sd["transformer_decoder.layers.0.linear1.weight"].shape[0]),
                seq_in=int(sd["image_pos_embedding"].shape[-2]), seq_out=int(sd["text_pos_embedding"].shape[-2]), eps=float(eps))


def mapper_config_c(cfg: dict) -> "_lib.MapperConfigC":
    c = _lib.MapperConfigC()
    c.struct_size = ctypes.sizeof(_lib.MapperConfigC)
    c.input_dim, c.output_dim, c.layers, c.heads = cfg["input_dim"], cfg["output_dim"], cfg["layers"], cfg["heads"]
    c.dim_feedforward, c.seq_in, c.seq_out, c.eps = cfg["dim_feedforward"], cfg["seq_in"], cfg["seq_out"], cfg["eps"]
    return c


class HipMappingNetwork(_EngineObject):
    _destroy = "lavie_mapper_destroy"
    broadcasts_image = True            # image_embeds [1, ...] serves every prompt (VideoGenPipeline._widen need not expand it)

    def __init__(self, state_dict, num_heads=12, device="cuda", eps=1e-5):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        sd = {k: v for k, v in sd.items() if k not in MAPPER_IGNORED}
        self._cfg = mapper_config_from_state_dict(sd, num_heads, eps)
        self.device = torch.device(device)
        self.dtype = torch.float16
        self._stock = None
        self._h = None
        if self.device.type != "cuda":
            raise ValueError("HipMappingNetwork lives on a HIP device")
        want = mapper_state_dict_keys(self._cfg["layers"])
        if set(sd) != set(want):
            raise ValueError(f"mapper checkpoint: missing keys {sorted(set(want) - set(sd))[:4]}, unexpected keys "
                             f"{sorted(set(sd) - set(want))[:4]}")
        lib = _lib.load()
        c = mapper_config_c(self._cfg)
        h = ctypes.c_void_p()
        _lib.check(lib.lavie_mapper_create(ctypes.byref(c), ctypes.byref(h)), "lavie_mapper_create")
        self._h = h
        _load(lib, "lavie_mapper", h, want, sd, self.device)

    @classmethod
    def from_stock(cls, mapper, device=None):
        """A lavie_amd.mapping.MappingNetwork (or the reference's): its weights copied to the engine, rounded to fp16."""
        dev = device or next(mapper.parameters()).device
        if torch.device(dev).type != "cuda":
            dev = "cuda"
        layer = mapper.transformer_decoder.layers[0]
        self = cls(mapper.state_dict(), num_heads=layer.self_attn.num_heads, device=dev, eps=layer.norm1.eps)
        self._stock = mapper
        return self

    @classmethod
    def from_checkpoint(cls, path_or_sd, num_heads=12, device="cuda"):
        """A saved mapper (a path to `torch.save(mapper.state_dict())` or the state dict itself), as MappingNetwork.from_checkpoint."""
        sd = torch.load(path_or_sd, map_location="cpu", weights_only=True) if isinstance(path_or_sd, str) else dict(path_or_sd)
        return cls(sd, num_heads=num_heads, device=device)

    def workspace_bytes(self, b):
        n = _lib.load().lavie_mapper_workspace_bytes(self._h, b)
        if n < 0:
            _lib.check(-1, "lavie_mapper_workspace_bytes")
        return n

    @torch.no_grad()
    def __call__(self, image_embeds, text_embeds, out=None, row0=0):
        """image_embeds [Bi, seq_in, input_dim] with Bi = 1 (one image for every prompt) or B; text_embeds [B, seq_out, output_dim]
        -> [B, seq_out, output_dim] fp16.  out / row0: write the rows row0 .. row0 + seq_out - 1 of a contiguous fp16
        [B, rows, output_dim] tensor instead (a context buffer whose other rows are left alone); returns `out` then."""
        c = self._cfg
        if image_embeds.dim() != 3 or tuple(image_embeds.shape[1:]) != (c["seq_in"], c["input_dim"]):
            raise ValueError(f"image_embeds must be [Bi, {c['seq_in']}, {c['input_dim']}], got {tuple(image_embeds.shape)}")
        if text_embeds.dim() != 3 or tuple(text_embeds.shape[1:]) != (c["seq_out"], c["output_dim"]):
            raise ValueError(f"text_embeds must be [B, {c['seq_out']}, {c['output_dim']}], got {tuple(text_embeds.shape)}")
        b, bi = text_embeds.shape[0], image_embeds.shape[0]
        if b < 1 or bi not in (1, b):
            raise ValueError(f"got {bi} images for {b} prompts (expected 1 or one per prompt)")
        lib = _lib.load()
        with torch.cuda.device(self.device):
            img = image_embeds.to(device=self.device, dtype=torch.float16).contiguous()
            txt = text_embeds.to(device=self.device, dtype=torch.float16).contiguous()
            if out is None:
                out, row0 = torch.empty((b, c["seq_out"], c["output_dim"]), dtype=torch.float16, device=self.device), 0
            elif not (out.is_cuda and out.device == img.device and out.dtype == torch.float16 and out.is_contiguous() and out.dim() == 3
                      and out.shape[0] == b and out.shape[2] == c["output_dim"]):
                raise ValueError(f"out must be a contiguous fp16 [{b}, rows, {c['output_dim']}] tensor on {self.device}")
            for b0 in range(0, b, MAX_BATCH):          # a prompt's bits do not depend on the batch around it: chunks are exact
                n = min(MAX_BATCH, b - b0)
                im = img if bi == 1 else img[b0:b0 + n]
                _lib.check(lib.lavie_mapper_encode(self._h, ctypes.c_void_p(im.data_ptr()), im.shape[0], ctypes.c_void_p(txt[b0:b0 + n].data_ptr()),
                                                   n, ctypes.c_void_p(out[b0:b0 + n].data_ptr()), out.shape[1], int(row0), ops._stream()),
                           "lavie_mapper_encode")
        return out
