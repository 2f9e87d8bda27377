"""What the engine-backed encoders share (text_encoder.py, image_encoder.py, fvd.py): the object the pipelines handle as a part, the
loading of a handle's weights, and the CLIP layer's keys and config reader of the text encoder and the vision tower."""
import ctypes

import torch

from . import _lib, ops

CLIP_LAYER_KEYS = tuple(f"self_attn.{proj}.{wb}" for proj in ("k_proj", "v_proj", "q_proj", "out_proj") for wb in ("weight", "bias")) + (
    "layer_norm1.weight", "layer_norm1.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias",
    "layer_norm2.weight", "layer_norm2.bias")


def clip_layer_keys(prefix: str, layers: int):
    """The 16 keys of every `{prefix}encoder.layers.{i}.`, in the engine's order."""
    return [f"{prefix}encoder.layers.{i}.{k}" for i in range(int(layers)) for k in CLIP_LAYER_KEYS]


def clip_config_dict(config, keys, noun: str) -> dict:
    """The fields `keys` of a transformers config or a dict with its names; `noun` names the model in the error."""
    get = config.get if isinstance(config, dict) else lambda k, d=None: getattr(config, k, d)
    cfg = {k: get(k) for k in keys}
    cfg["hidden_act"] = cfg["hidden_act"] or "quick_gelu"
    cfg["layer_norm_eps"] = 1e-5 if cfg["layer_norm_eps"] is None else cfg["layer_norm_eps"]
    missing = [k for k, v in cfg.items() if v is None]
    if missing:
        raise ValueError(f"{noun} config lacks {missing}")
    return cfg


class LastHiddenState(tuple):
    """`out[0]` and `out.last_hidden_state`, as the stock model's output offers them."""

    def __new__(cls, last_hidden_state):
        return super().__new__(cls, (last_hidden_state,))

    @property
    def last_hidden_state(self):
        return self[0]


def _load(lib, prefix, h, want, sd, device, dtype=torch.float16):
    """set_param for every key of `want` (as `dtype`, the one the handle reads), finalize, and the end of the loan"""
    with torch.cuda.device(device):
        held = []
        for k in want:
            t = sd[k].detach().to(device=device, dtype=dtype).contiguous()
            held.append(t)
            _lib.check(getattr(lib, prefix + "_set_param")(h, k.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()), prefix + "_set_param")
        _lib.check(getattr(lib, prefix + "_finalize")(h, ops._stream()), prefix + "_finalize")
        torch.cuda.current_stream().synchronize()      # the tensors were borrowed until the stream drains
    del held


class _EngineObject:
    """What the pipelines ask of every part: .to(device), .eval(), .parameters(); the engine copy stays where it was built."""
    _destroy = None

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            try:
                getattr(_lib.load(), self._destroy)(self._h)
            except Exception:
                pass
            self._h = None

    def to(self, device=None, *args, **kwargs):
        if device is not None and not isinstance(device, torch.dtype):
            d = torch.device(device)
            if d.type != "cuda" or (d.index is not None and self.device.index is not None and d.index != self.device.index):
                raise ValueError(f"{type(self).__name__} was built on {self.device} and cannot move to {d}")
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())
