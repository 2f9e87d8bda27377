"""transformers' CLIPTextModel on the engine (lavie_text_* of include/lavie_hip.h).

`HipCLIPTextModel` stands where a pipeline expects its `text_encoder`: `enc(input_ids)[0]` and `.last_hidden_state` are the fp16
`[B, L, C]` hidden states with the final LayerNorm applied.  Two calls on the same ids agree bit for bit, and a prompt's `[L, C]`
block has the same bits at every batch size and position in the batch.  Not built: pooled / projected outputs, key-padding masks,
`output_hidden_states`, the tokenizer."""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib, ops
from ._engine_object import LastHiddenState, _EngineObject, _load, clip_config_dict, clip_layer_keys

ACTS = ops.ACT_KINDS                  # hidden_act -> lavie_text_config.act
MAX_BATCH = 16                        # lavie_text_encode: 1 <= B <= 16
CONFIG_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
               "max_position_embeddings", "hidden_act", "layer_norm_eps")
IGNORED_KEYS = ("text_model.embeddings.position_ids",)      # a buffer of older transformers versions, not a weight


def state_dict_keys(config: dict):
    """The keys the engine expects, in its order: those of CLIPTextModel(config).state_dict() (see normalize_keys)."""
    return (["text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight"]
            + clip_layer_keys("text_model.", config["num_hidden_layers"])
            + ["text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias"])


def normalize_keys(sd: dict) -> dict:
    """The engine's names are the classic checkpoint keys, `text_model.`-prefixed (transformers < 5 and every published CLIP text
    checkpoint); transformers 5 builds CLIPTextModel flat and its state_dict() drops the prefix.  Both spellings are taken."""
    out = {}
    for k, v in sd.items():
        if k in IGNORED_KEYS or "text_model." + k in IGNORED_KEYS:
            continue
        out[k if k.startswith("text_model.") else "text_model." + k] = v
    return out


def config_dict(config) -> dict:
    """The eight fields the engine reads, from a transformers CLIPTextConfig or a dict with its names."""
    return clip_config_dict(config, CONFIG_KEYS, "text encoder")


def config_c(cfg: dict) -> "_lib.TextConfigC":
    if cfg["hidden_act"] not in ACTS:
        raise ValueError(f"hidden_act {cfg['hidden_act']!r} is not built: the engine has {sorted(ACTS)}")
    c = _lib.TextConfigC()
    c.struct_size = ctypes.sizeof(_lib.TextConfigC)
    c.vocab_size, c.hidden, c.intermediate = int(cfg["vocab_size"]), int(cfg["hidden_size"]), int(cfg["intermediate_size"])
    c.layers, c.heads, c.max_positions = int(cfg["num_hidden_layers"]), int(cfg["num_attention_heads"]), int(cfg["max_position_embeddings"])
    c.act, c.eps = ACTS[cfg["hidden_act"]], float(cfg["layer_norm_eps"])
    return c


class TextEncoderOutput(LastHiddenState):
    """What `HipCLIPTextModel.__call__` returns."""


class HipCLIPTextModel(_EngineObject):
    _destroy = "lavie_text_destroy"

    def __init__(self, state_dict, config, device="cuda"):
        """state_dict: CLIPTextModel.state_dict() (any float dtype; rounded to fp16 here); config: CLIPTextConfig or dict."""
        self._cfg = config_dict(config)
        self.config = config if not isinstance(config, dict) else SimpleNamespace(**config)
        self.device = torch.device(device)
        self.dtype = torch.float16
        self._stock = None                 # the module from_stock wrapped (VideoGenPipeline.disable_engine_text_encoder hands it back)
        self._h = None
        c = config_c(self._cfg)
        if self.device.type != "cuda":
            raise ValueError("HipCLIPTextModel lives on a HIP device")
        lib = _lib.load()
        sd = normalize_keys(state_dict)
        want = state_dict_keys(self._cfg)
        if set(sd) != set(want):
            raise ValueError(f"state dict does not match the config: missing {sorted(set(want) - set(sd))[:4]}, "
                             f"unexpected {sorted(set(sd) - set(want))[:4]}")
        h = ctypes.c_void_p()
        _lib.check(lib.lavie_text_create(ctypes.byref(c), ctypes.byref(h)), "lavie_text_create")
        self._h = h
        _load(lib, "lavie_text", h, want, sd, self.device)

    @classmethod
    def from_stock(cls, clip_text_model, device=None):
        dev = device or next(clip_text_model.parameters()).device
        if torch.device(dev).type != "cuda":
            dev = "cuda"
        self = cls(clip_text_model.state_dict(), clip_text_model.config, device=dev)
        self._stock = clip_text_model
        return self

    @classmethod
    def from_state_dict(cls, sd, config_dict, device="cuda"):
        return cls(sd, config_dict, device=device)

    def workspace_bytes(self, b, l):
        n = _lib.load().lavie_text_workspace_bytes(self._h, b, l)
        if n < 0:
            _lib.check(-1, "lavie_text_workspace_bytes")
        return n

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, position_ids=None, output_hidden_states=None, **kwargs):
        for name, val in (("attention_mask", attention_mask), ("position_ids", position_ids),
                          ("output_hidden_states", output_hidden_states)):
            if val is not None and val is not False:
                raise NotImplementedError(f"HipCLIPTextModel: `{name}` is not built (key-padding masks, custom positions and "
                                          "per-layer outputs are outside the engine encoder)")
        extra = [k for k, v in kwargs.items() if v is not None and v is not False and k != "return_dict"]
        if extra:
            raise NotImplementedError(f"HipCLIPTextModel: {extra} not built")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int32, torch.int64):
            raise ValueError("input_ids must be a [B, L] integer tensor")
        b, l = input_ids.shape
        v = self._cfg["vocab_size"]
        if not 1 <= l <= self._cfg["max_position_embeddings"]:
            raise ValueError(f"input_ids: L = {l} must be 1..max_position_embeddings = {self._cfg['max_position_embeddings']}")
        if b < 1:
            raise ValueError("input_ids: empty batch")
        if int(input_ids.min()) < 0 or int(input_ids.max()) >= v:      # on the host, before upload: the kernel would clamp
            raise ValueError(f"input_ids must lie in [0, {v}), got [{int(input_ids.min())}, {int(input_ids.max())}]")
        lib = _lib.load()
        with torch.cuda.device(self.device):
            ids = input_ids.to(device=self.device, dtype=torch.int32).contiguous()
            out = torch.empty((b, l, self._cfg["hidden_size"]), dtype=torch.float16, device=self.device)
            for b0 in range(0, b, MAX_BATCH):          # a prompt's bits do not depend on the batch around it: chunks are exact
                n = min(MAX_BATCH, b - b0)
                _lib.check(lib.lavie_text_encode(self._h, ctypes.c_void_p(ids[b0:b0 + n].data_ptr()), n, l,
                                                 ctypes.c_void_p(out[b0:b0 + n].data_ptr()), ops._stream()), "lavie_text_encode")
        return TextEncoderOutput(out)
