"""Host-side mirror of `base/models/unet.py` (reference): `UNet3DConditionModel`.

Same constructor keywords (the ones live on the inference path), same state-dict key names and
shapes (unet.py:142-295), same `forward(sample, timestep, encoder_hidden_states, ...).sample`
surface (unet.py:366-375, 509-512) — but the module holds no compute of its own: forward hands the
fp16 parameters and inputs to the gfx950 engine in liblavie_hip.so.  There is no eager/CPU path."""
import ctypes
import json
import math
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import _lib, lora as _lora, spec
from .config import UNetConfig
from .weights import rotary_freqs


@dataclass
class UNet3DConditionOutput:
    sample: torch.Tensor


def _attach(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    """Registers `param` under the reference's dotted state-dict name, creating plain containers."""
    parts = dotted.split(".")
    mod = root
    for name in parts[:-1]:
        child = mod._modules.get(name)
        if child is None:
            child = nn.Module()
            mod.add_module(name, child)
        mod = child
    mod.register_parameter(parts[-1], param)


class UNet3DConditionModel(nn.Module):
    _supported_down = ("CrossAttnDownBlock3D", "DownBlock3D")
    # transformer-block variant (UNetConfig fields); lavie_amd.interpolation.unet overrides it
    _block_variant = dict(sparse_causal_attn1=False, temporal_plain=False, ff_before_temporal=False)
    _allow_first_frame = False
    _allow_vsr_options = False            # only_cross_attention tuples / use_linear_projection (lavie_amd.vsr.unet)
    _lora_supported = True                # load_lora(); lavie_amd.vsr.unet refuses it

    def __init__(
        self,
        sample_size: Optional[int] = None,
        in_channels: int = 4,
        out_channels: int = 4,
        center_input_sample: bool = False,
        flip_sin_to_cos: bool = True,
        freq_shift: int = 0,
        down_block_types: Tuple[str, ...] = ("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D"),
        mid_block_type: str = "UNetMidBlock3DCrossAttn",
        up_block_types: Tuple[str, ...] = ("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D"),
        only_cross_attention: bool = False,
        block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280),
        layers_per_block: int = 2,
        downsample_padding: int = 1,
        mid_block_scale_factor: float = 1,
        act_fn: str = "silu",
        norm_num_groups: int = 32,
        norm_eps: float = 1e-5,
        cross_attention_dim: int = 1280,
        attention_head_dim: int = 8,
        dual_cross_attention: bool = False,
        use_linear_projection: bool = False,
        class_embed_type: Optional[str] = None,
        num_class_embeds: Optional[int] = None,
        upcast_attention: bool = False,
        resnet_time_scale_shift: str = "default",
        use_first_frame: bool = False,
        use_relative_position: bool = False,
        init_weights: bool = True,
    ):
        """`init_weights=False` (not a reference keyword) skips the ~1 min CPU default initialisation of the
        909 M parameters when a state dict is about to be loaded anyway."""
        super().__init__()
        # options that leave the benchmarked inference path (SURVEY.md §8a "Not on the path")
        unsupported = {
            "center_input_sample": center_input_sample,
            "only_cross_attention": only_cross_attention and not self._allow_vsr_options,
            "dual_cross_attention": dual_cross_attention,
            "use_linear_projection": use_linear_projection and not self._allow_vsr_options,
            "class_embed_type": class_embed_type, "num_class_embeds": num_class_embeds,
            "upcast_attention": upcast_attention, "use_first_frame": use_first_frame and not self._allow_first_frame,
            "use_relative_position": use_relative_position,
        }
        bad = [k for k, v in unsupported.items() if v]
        if bad or not flip_sin_to_cos or freq_shift != 0 or resnet_time_scale_shift != "default" \
                or act_fn not in ("silu", "swish") or mid_block_type != "UNetMidBlock3DCrossAttn" \
                or downsample_padding != 1 or mid_block_scale_factor != 1 or not isinstance(attention_head_dim, int):
            raise NotImplementedError(f"UNet3DConditionModel option outside the MI355X path: {bad or 'see constructor'}")
        if len(down_block_types) != len(block_out_channels) or len(up_block_types) != len(block_out_channels):
            raise ValueError("down_block_types / up_block_types / block_out_channels must have equal lengths")
        attn = tuple(t == "CrossAttnDownBlock3D" for t in down_block_types)
        for t in down_block_types:
            if t not in self._supported_down:
                raise ValueError(f"{t} does not exist.")
        expect_up = tuple("CrossAttnUpBlock3D" if a else "UpBlock3D" for a in reversed(attn))
        if tuple(up_block_types) != expect_up:
            raise NotImplementedError("up_block_types must mirror down_block_types")

        self.sample_size = sample_size
        self.cfg = UNetConfig(sample_size=sample_size or 64, in_channels=in_channels, out_channels=out_channels,
                              block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
                              heads=attention_head_dim, cross_attention_dim=cross_attention_dim,
                              norm_groups=norm_num_groups, norm_eps=norm_eps, attn_levels=attn,
                              **dict(self._block_variant, sparse_causal_attn1=bool(use_first_frame) and self._allow_first_frame),
                              **self._vsr_config(only_cross_attention, use_linear_projection, len(block_out_channels)))
        self.cfg.validate()
        self.config = SimpleNamespace(
            sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
            center_input_sample=False, block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
            cross_attention_dim=cross_attention_dim, attention_head_dim=attention_head_dim,
            norm_num_groups=norm_num_groups, norm_eps=norm_eps, class_embed_type=None,
            down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types))
        self.num_upsamplers = len(block_out_channels) - 1

        # parameters under the reference's names; values follow the reference constructor's defaults
        for name, shape in spec.iter_params(self.cfg):
            if name.endswith("rotary_emb.freqs"):       # incl. the VSR model's shared `temporal_rotary_emb.freqs`
                p = nn.Parameter(rotary_freqs(self.cfg.rotary_dim), requires_grad=False)
            else:
                p = nn.Parameter(torch.empty(shape), requires_grad=False)
                if init_weights:
                    self._default_init(name, p.data)
            _attach(self, name, p)

        self._engine = None
        self._engine_key = None
        self._prepared = None
        self._cached_ctx = None
        self._graph = False
        self._graph_io = {}
        # the loaded adapters (load_lora), on the host: {target weight name: {adapter name: (A fp32 [r, K], B fp32 [N, r],
        # per-target scale)}} ({} without one), per adapter its engine slot, blend weight and whether it is active (set_adapters),
        # and the global scale; every engine build registers them again, only unload_lora() / delete_adapters() / fuse_lora() remove
        self._lora = {}
        self._lora_adapters = {}
        self._lora_scale = 1.0

    def _vsr_config(self, only_cross_attention, use_linear_projection, levels: int) -> dict:
        """UNetConfig fields of the VSR block variant; the base and interpolation models have none."""
        return {}

    # ------------------------------------------------------------------ init / bookkeeping
    @staticmethod
    def _default_init(name: str, t: torch.Tensor) -> None:
        if t.dim() == 1:
            (nn.init.ones_ if name.endswith("weight") else nn.init.zeros_)(t)
            if name.endswith("bias") and "norm" not in name:     # Linear/Conv bias: U(-1/sqrt(fan_in), ..) in torch;
                nn.init.zeros_(t)                                # kept at zero here, checkpoints overwrite it
        elif name.endswith("relative_attention_bias.weight"):
            nn.init.normal_(t)
        elif name.endswith("attn_temp.to_out.0.weight"):
            nn.init.zeros_(t)                                     # attention.py:475
        else:
            fan_in = t[0].numel()
            bound = 1.0 / fan_in ** 0.5
            nn.init.uniform_(t, -bound, bound)

    @property
    def dtype(self) -> torch.dtype:
        return self.conv_in.weight.dtype

    @property
    def device(self) -> torch.device:
        return self.conv_in.weight.device

    def _apply(self, fn, *a, **k):            # .to()/.half()/.cuda() replace parameter storage
        self._drop_engine()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._drop_engine()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _drop_engine(self):
        eng = self.__dict__.get("_engine")
        if eng:
            _lib.load().lavie_unet_destroy(eng)
        self.__dict__["_engine"] = None
        self.__dict__["_engine_key"] = None
        self.__dict__["_prepared"] = None
        self.__dict__["_cached_ctx"] = None
        self.__dict__["_graph_io"] = {}

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    # ------------------------------------------------------------------ engine
    def _config_c(self) -> "_lib.UNetConfigC":
        c = _lib.UNetConfigC()
        c.struct_size = ctypes.sizeof(_lib.UNetConfigC)
        cfg = self.cfg
        c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
        c.num_levels = len(cfg.block_out_channels)
        for i, (w, a) in enumerate(zip(cfg.block_out_channels, cfg.attn_levels)):
            c.block_out_channels[i] = w
            c.attn_levels[i] = int(a)
        c.layers_per_block, c.heads = cfg.layers_per_block, cfg.heads
        c.cross_attention_dim, c.norm_groups, c.norm_eps = cfg.cross_attention_dim, cfg.norm_groups, cfg.norm_eps
        c.rotary_dim, c.rel_buckets, c.rel_max_distance = cfg.rotary_dim, cfg.rel_buckets, cfg.rel_max_distance
        c.sparse_causal_attn1, c.temporal_plain = int(cfg.sparse_causal_attn1), int(cfg.temporal_plain)
        c.ff_before_temporal = int(cfg.ff_before_temporal)
        c.vsr_blocks = int(cfg.vsr_blocks)
        for i, v in enumerate(cfg.only_cross_attention):
            c.only_cross_attention[i] = int(v)
        c.vsr_temporal_modules, c.num_class_embeds = int(cfg.vsr_temporal_modules), int(cfg.num_class_embeds)
        return c

    def _ensure_engine(self):
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("UNet3DConditionModel runs on MI355X only: move the model to a HIP device "
                               "(model.to('cuda', torch.float16)); there is no CPU path")
        if self.dtype != torch.float16:
            raise RuntimeError("UNet3DConditionModel computes in fp16: call .half() / .to(dtype=torch.float16)")
        if self._engine is not None:        # invalidated by _apply()/load_state_dict(); see refresh_engine()
            return self._engine
        key = dev.index
        lib = _lib.load()
        handle = ctypes.c_void_p()
        cfg_c = self._config_c()
        with torch.cuda.device(dev):
            _lib.check(lib.lavie_unet_create(ctypes.byref(cfg_c), ctypes.byref(handle)), "lavie_unet_create")
            try:
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                keep = []            # tensors made for the engine (contiguous / padded copies) stay alive until finalize
                for name, p in self.named_parameters():
                    t = self._engine_tensor(name, p.data if p.data.is_contiguous() else p.data.contiguous())
                    keep.append(t)
                    _lib.check(lib.lavie_unet_set_param(handle, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()),
                               f"lavie_unet_set_param({name})")
                _lib.check(lib.lavie_unet_finalize(handle, stream), "lavie_unet_finalize")
                if self.freeu != (1.0, 1.0, 1.0, 1.0):
                    _lib.check(lib.lavie_unet_set_freeu(handle, *self.freeu), "lavie_unet_set_freeu")
                if self.pag != ((), 0):
                    self._set_pag_engine(lib, handle, *self.pag)
                if self.layer_cache:
                    _lib.check(lib.lavie_unet_set_layer_cache(handle, self.layer_cache), "lavie_unet_set_layer_cache")
                if self._lora:
                    keep += self._lora_register(handle, stream)
                    _lib.check(lib.lavie_unet_lora_set_scale(handle, float(self._lora_scale)), "lavie_unet_lora_set_scale")
                    _lib.check(lib.lavie_unet_lora_apply(handle, stream), "lavie_unet_lora_apply")
                torch.cuda.current_stream().synchronize()
            except Exception:
                lib.lavie_unet_destroy(handle)
                raise
        self.__dict__["_engine"] = handle
        self.__dict__["_engine_key"] = key
        return handle

    def _engine_tensor(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """Hook: the tensor handed to the engine for state-dict entry `name` (identity here)."""
        return t

    def refresh_engine(self):
        """Re-packs the weights after parameters were modified in place."""
        self._drop_engine()
        return self._ensure_engine()

    # ------------------------------------------------------------------ LoRA adapters (served merged: lavie_unet_lora_*)
    def _lora_slots(self):
        """[(adapter name, slot, weight the engine gets)] in ascending slot order = the order of the terms of the blend."""
        return sorted(((n, st["slot"], st["weight"] if st["active"] else 0.0) for n, st in self._lora_adapters.items()),
                      key=lambda e: e[1])

    def _lora_names(self, names, what):
        names = [names] if isinstance(names, str) else list(names)
        for n in names:
            if n not in self._lora_adapters:
                raise ValueError(f"{what}: no adapter named {n!r} (loaded: {self.get_list_adapters()})")
        if len(set(names)) != len(names):
            raise ValueError(f"{what}: an adapter is named twice in {names}")
        return names

    def _lora_forget(self, name) -> None:
        """Drops adapter `name` from the host-side state."""
        for target in [t for t, per in self._lora.items() if name in per]:
            del self._lora[target][name]
            if not self._lora[target]:
                del self._lora[target]
        del self._lora_adapters[name]

    def _lora_engine(self, fn) -> None:
        """Runs fn(lib, handle, stream) on the built engine, if there is one, then applies and synchronises."""
        handle = self.__dict__.get("_engine")
        if not handle:
            return
        lib = _lib.load()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            keep = fn(lib, handle, stream)       # device copies stay alive until the engine's copies of them have run
            _lib.check(lib.lavie_unet_lora_set_scale(handle, float(self._lora_scale)), "lavie_unet_lora_set_scale")
            _lib.check(lib.lavie_unet_lora_apply(handle, stream), "lavie_unet_lora_apply")
            torch.cuda.current_stream().synchronize()
            del keep

    def _lora_register(self, handle, stream, only=None) -> list:
        """Registers the adapters (all, or the one named `only`) in their slots on `handle` with base = the module's own weights
        and sets the slots' weights; the caller applies and synchronises.  Returns the device tensors to keep alive until then."""
        lib = _lib.load()
        params = dict(self.named_parameters())
        keep = []
        for adapter, slot, weight in self._lora_slots():
            if only is not None and adapter != only:
                continue
            for name, per in self._lora.items():
                if adapter not in per:
                    continue
                a, b, s = per[adapter]
                w = params[name].data.contiguous()
                ad = a.to(self.device, torch.float32).contiguous()
                bd = b.to(self.device, torch.float32).contiguous()
                keep += [w, ad, bd]
                _lib.check(lib.lavie_unet_lora_set_slot(handle, slot, name.encode(), ctypes.c_void_p(w.data_ptr()),
                                                        ctypes.c_void_p(ad.data_ptr()), ctypes.c_void_p(bd.data_ptr()), a.shape[0],
                                                        float(s), stream), f"lavie_unet_lora_set_slot({slot}, {name})")
            _lib.check(lib.lavie_unet_lora_set_slot_weight(handle, slot, float(weight)), "lavie_unet_lora_set_slot_weight")
        return keep

    @staticmethod
    def _lora_clear_slots(lib, handle, stream, slots) -> None:
        for slot in slots:
            _lib.check(lib.lavie_unet_lora_clear_slot(handle, slot, None, stream), "lavie_unet_lora_clear_slot")
            _lib.check(lib.lavie_unet_lora_set_slot_weight(handle, slot, 1.0), "lavie_unet_lora_set_slot_weight")

    def load_lora(self, sd_or_path, scale: float = 1.0, alpha: Optional[float] = None, adapter_name: Optional[str] = None) -> None:
        """Loads a LoRA adapter (state dict, `.safetensors` / `.bin` / `.pt` file, or a directory holding
        `pytorch_lora_weights.safetensors`) onto the to_q / to_k / to_v / to_out.0 projections.  Per-target factor alpha / r
        (peft's scaling; 1.0 without alpha, the fork's lora_alpha = r), `alpha` overrides.
        adapter_name=None: replaces every loaded adapter with this one; `scale` is the global strength (set_lora_scale).
        With a name: adds the adapter, or replaces the one of that name, and keeps the others (up to 8 in all, blended in one merge in
        the order of their slots: the lowest free one is taken); it is active and `scale` is its blend weight (set_adapters); the
        global strength stays.  The module parameters stay the base weights (fuse_lora() writes the merge in)."""
        if not self._lora_supported:
            raise NotImplementedError(f"{type(self).__name__}: LoRA adapters are not supported on this model")
        cfg_alpha = None
        if isinstance(sd_or_path, (str, os.PathLike)):
            sd_or_path, cfg_alpha = _lora.load_lora_file(os.fspath(sd_or_path))
        shapes = {n: tuple(p.shape) for n, p in self.named_parameters()}
        tensors = _lora.normalize_lora_state_dict(sd_or_path, shapes)
        if not tensors:
            raise ValueError("load_lora: the state dict holds no LoRA matrices")
        scales = _lora.target_scales(tensors, alpha if alpha is not None else cfg_alpha)
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"load_lora: scale {scale} is not finite")
        if adapter_name is None:
            name, slot, weight = _lora.DEFAULT_ADAPTER, 0, 1.0
            stale = [st["slot"] for st in self._lora_adapters.values()]
            self.__dict__["_lora"] = {}
            self.__dict__["_lora_adapters"] = {}
            self.__dict__["_lora_scale"] = scale
        else:
            name, weight = str(adapter_name), scale
            if not name:
                raise ValueError("load_lora: adapter_name is empty")
            if name in self._lora_adapters:
                slot = self._lora_adapters[name]["slot"]
                stale = [slot]
                self._lora_forget(name)
            else:
                if len(self._lora_adapters) >= _lora.MAX_ADAPTERS:
                    raise ValueError(f"load_lora: {_lora.MAX_ADAPTERS} adapters are loaded already, the most the engine blends "
                                     f"({self.get_list_adapters()}); delete one first")
                used = {st["slot"] for st in self._lora_adapters.values()}
                slot = min(i for i in range(_lora.MAX_ADAPTERS) if i not in used)
                stale = []
        self._lora_adapters[name] = {"slot": slot, "weight": weight, "active": True}
        for n, (a, b, _) in tensors.items():
            self._lora.setdefault(n, {})[name] = (a, b, scales[n])

        def on_engine(lib, handle, stream):
            self._lora_clear_slots(lib, handle, stream, stale)
            return self._lora_register(handle, stream, only=name)
        self._lora_engine(on_engine)

    def set_adapters(self, names, weights=None) -> None:
        """The active set of the loaded adapters and their blend weights (finite floats, default 1.0; one number goes to all):
        W = W0 + sum (global scale * weight * alpha / r) B A over the active ones.  Loaded adapters that are not named stay resident
        and contribute nothing."""
        names = self._lora_names(names, "set_adapters")
        if weights is None:
            weights = [1.0] * len(names)
        elif isinstance(weights, (int, float)):
            weights = [weights] * len(names)
        weights = [float(w) for w in weights]
        if len(weights) != len(names):
            raise ValueError(f"set_adapters: {len(names)} names, {len(weights)} weights")
        for n, w in zip(names, weights):
            if not math.isfinite(w):
                raise ValueError(f"set_adapters: weight {w} of {n!r} is not finite")
        for n, st in self._lora_adapters.items():
            st["active"] = n in names
        for n, w in zip(names, weights):
            self._lora_adapters[n]["weight"] = w

        def on_engine(lib, handle, stream):
            for _, slot, weight in self._lora_slots():
                _lib.check(lib.lavie_unet_lora_set_slot_weight(handle, slot, float(weight)), "lavie_unet_lora_set_slot_weight")
        self._lora_engine(on_engine)

    def delete_adapters(self, names) -> None:
        """Removes the named adapters; the others keep their slots, weights and state."""
        names = self._lora_names(names, "delete_adapters")
        slots = [self._lora_adapters[n]["slot"] for n in names]
        for n in names:
            self._lora_forget(n)
        self._lora_engine(lambda lib, handle, stream: self._lora_clear_slots(lib, handle, stream, slots))

    def get_list_adapters(self) -> list:
        """Names of the loaded adapters, in blend (slot) order."""
        return [n for n, _, _ in self._lora_slots()]

    def get_active_adapters(self) -> list:
        """Names of the adapters that contribute, in blend (slot) order."""
        return [n for n, _, _ in self._lora_slots() if self._lora_adapters[n]["active"]]

    def set_lora_scale(self, scale: float) -> None:
        """Global adapter strength over the whole blend (diffusers' cross_attention_kwargs={"scale": s}); 0 gives the base model's
        outputs exactly."""
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"set_lora_scale: scale {scale} is not finite")
        self.__dict__["_lora_scale"] = scale
        handle = self.__dict__.get("_engine")
        if handle:
            lib = _lib.load()
            with torch.cuda.device(self.device):
                _lib.check(lib.lavie_unet_lora_set_scale(handle, scale), "lavie_unet_lora_set_scale")
                _lib.check(lib.lavie_unet_lora_apply(handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                           "lavie_unet_lora_apply")

    @property
    def lora_scale(self) -> float:
        return self._lora_scale

    def unload_lora(self) -> None:
        """Removes every adapter: the engine goes back to the base weights (bit-identical to a model that never had one)."""
        slots = [st["slot"] for st in self._lora_adapters.values()]
        self.__dict__["_lora"] = {}
        self.__dict__["_lora_adapters"] = {}
        self.__dict__["_lora_scale"] = 1.0
        self._lora_engine(lambda lib, handle, stream: self._lora_clear_slots(lib, handle, stream, sorted(set(slots + [0]))))

    @torch.no_grad()
    def fuse_lora(self) -> None:
        """Writes the merged weights the engine serves (the same kernels, inputs and fp32 factors: lavie_lora_merge_multi_f16 over
        the adapters in slot order) into the module parameters and removes every adapter; the engine is rebuilt from them on next
        use."""
        if not self._lora:
            return
        if self.device.type != "cuda" or self.dtype != torch.float16:
            raise RuntimeError("fuse_lora: the model must be on a HIP device in fp16")
        from . import ops
        params = dict(self.named_parameters())
        order = self._lora_slots()
        with torch.cuda.device(self.device):
            for name, per in self._lora.items():
                p = params[name]
                terms = [(per[ad][0].to(self.device, torch.float32).contiguous(), per[ad][1].to(self.device, torch.float32).contiguous(),
                          _lora.blend_factor(self._lora_scale, weight, per[ad][2]))       # the engine's fp32 product
                         for ad, _, weight in order if ad in per]
                p.data.copy_(ops.lora_merge_multi(p.data.contiguous(), terms))
        self.__dict__["_lora"] = {}
        self.__dict__["_lora_adapters"] = {}
        self.__dict__["_lora_scale"] = 1.0
        self._drop_engine()

    def engine_handle(self):
        """The `lavie_unet_t` behind this module (built on first use)."""
        return self._ensure_engine()

    def prepare(self, batch: int, frames: int, height: int, width: int, ctx_len: int = 77) -> None:
        """Sizes the engine workspace for latents [batch, C, frames, height, width] (allocates)."""
        handle = self._ensure_engine()
        want = (batch, frames, height, width, ctx_len)
        if self._prepared == want:
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().lavie_unet_prepare(handle, *want), "lavie_unet_prepare")
        self.__dict__["_prepared"] = want

    def cache_context(self, encoder_hidden_states: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Computes the text keys / values of every transformer block once for this context (lavie_unet_cache_context) and
        returns the fp16 device tensor to pass as `encoder_hidden_states` while it is cached — a denoise loop calls this
        before its first step and `cache_context(None)` after its last.  The tensor must not be modified meanwhile."""
        handle = self._ensure_engine()
        lib = _lib.load()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if encoder_hidden_states is None:
                self.__dict__["_cached_ctx"] = None
                _lib.check(lib.lavie_unet_cache_context(handle, None, 0, 0, stream), "lavie_unet_cache_context")
                return None
            if self._prepared is None:
                raise RuntimeError("cache_context: call prepare(batch, frames, height, width, ctx_len) first")
            ctx = encoder_hidden_states.to(device=self.device, dtype=torch.float16).contiguous()
            _lib.check(lib.lavie_unet_cache_context(handle, ctypes.c_void_p(ctx.data_ptr()), ctx.shape[0], ctx.shape[1], stream),
                       "lavie_unet_cache_context")
        self.__dict__["_cached_ctx"] = ctx          # keeps the tensor (and so its address) alive while cached
        return ctx

    def set_cfg_shared_input(self, on: bool) -> None:
        """Classifier-free guidance feeds the UNet `torch.cat([latents] * 2)` (pipeline_videogen.py:666): with on=True the caller
        vouches that sample[b] == sample[b + B/2] (and the timesteps likewise) in the forwards that follow, and the engine computes
        the layers in front of the first text cross-attention once (lavie_unet_set_cfg_shared_input).  The denoise loops that
        build the duplicated input themselves switch it on around their steps and off afterwards."""
        handle = self._ensure_engine()
        _lib.check(_lib.load().lavie_unet_set_cfg_shared_input(handle, 1 if on else 0), "lavie_unet_set_cfg_shared_input")

    # ------------------------------------------------------------------ FreeU (diffusers' enable_freeu / disable_freeu)
    @property
    def freeu(self):
        """(s1, s2, b1, b2) in force; (1, 1, 1, 1) = off."""
        return self.__dict__.get("_freeu", (1.0, 1.0, 1.0, 1.0))

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """FreeU (Si et al.), diffusers' names and argument order: in up block i in {0, 1}, in front of every resnet, the first half
        of the running activation's channels is scaled by b_{i+1} and the four lowest modes of the skip's 2-D spectrum by s_{i+1}
        (lavie_unet_set_freeu; the launches run inside the engine's forward).  Every value must be finite and > 0; (1, 1, 1, 1) is off.
        The setting lives on the model: it holds for every forward that follows, through every pipeline, until disable_freeu()."""
        vals = tuple(float(v) for v in (s1, s2, b1, b2))
        if not all(math.isfinite(v) and v > 0.0 for v in vals):
            raise ValueError(f"enable_freeu: s1={s1} s2={s2} b1={b1} b2={b2} must all be finite and > 0")
        if self.__dict__.get("_engine"):
            _lib.check(_lib.load().lavie_unet_set_freeu(self._engine, *vals), "lavie_unet_set_freeu")
        self.__dict__["_freeu"] = vals

    def disable_freeu(self) -> None:
        self.enable_freeu(1.0, 1.0, 1.0, 1.0)

    # ------------------------------------------------------------------ perturbed-attention guidance (diffusers' PAG pipelines)
    @property
    def pag(self):
        """(layers, perturbed) in force; ((), 0) = off."""
        return self.__dict__.get("_pag", ((), 0))

    @staticmethod
    def _set_pag_engine(lib, handle, layers, perturbed) -> None:
        arr = (ctypes.c_char_p * max(len(layers), 1))(*[name.encode() for name in layers])
        _lib.check(lib.lavie_unet_set_pag(handle, arr, len(layers), int(perturbed)), "lavie_unet_set_pag")

    def set_pag(self, layers, perturbed: int) -> None:
        """Perturbed-attention guidance (Ahn et al.) in the forwards that follow: in every transformer whose state-dict prefix starts
        with an entry of `layers` ("mid_block", "down_blocks.2", "up_blocks.1.attentions.0", ...), attn1 of the last `perturbed` batch
        entries is the identity map on values, to_out(to_v(norm1(x))) (lavie_unet_set_pag).  No layers or perturbed = 0 is off.  The
        setting lives on the model until disable_pag(); the pipeline makes it for the length of one call."""
        layers = (layers,) if isinstance(layers, str) else tuple(str(name) for name in layers)
        perturbed = int(perturbed)
        if perturbed < 0:
            raise ValueError(f"set_pag: perturbed={perturbed} must be >= 0")
        if not layers or perturbed == 0:
            layers, perturbed = (), 0
        if self.__dict__.get("_engine"):
            self._set_pag_engine(_lib.load(), self._engine, layers, perturbed)
        else:                               # no engine yet: the names are checked against the module tree, as the engine will
            known = {name.split(".transformer_blocks.")[0] for name, _ in self.named_parameters() if ".transformer_blocks." in name}
            for entry in layers:
                if not any(k == entry or k.startswith(entry + ".") for k in known):
                    raise ValueError(f"set_pag: layers entry {entry!r} selects no transformer")
        self.__dict__["_pag"] = (layers, perturbed)

    def disable_pag(self) -> None:
        self.set_pag((), 0)

    # ------------------------------------------------------------------ layer cache (DeepCache)
    LAYER_CACHE_MODES = {None: 0, "refresh": 1, "reuse": 2}

    @property
    def layer_cache(self) -> int:
        """The depth of the layer cache's cuts; 0 = off."""
        return self.__dict__.get("_layer_cache", 0)

    def enable_layer_cache(self, depth: int = 1) -> None:
        """Feature caching across denoising steps (DeepCache, Ma et al.): forward(layer_cache="refresh") runs the whole network and
        keeps the activation that enters the last `depth` + 1 layers of the last up block; forward(layer_cache="reuse") runs only the
        first `depth` layers of the first down block and those up layers on it (lavie_unet_set_layer_cache).  depth in
        1..layers_per_block; the model needs three levels or more.  A call drops what is cached.  The cached tensor is whatever the
        refresh computed: weights, adapters, FreeU or PAG changed before a reuse are the caller's business."""
        depth = int(depth)
        if not 1 <= depth <= self.cfg.layers_per_block:
            raise ValueError(f"enable_layer_cache: depth={depth} must be in 1..{self.cfg.layers_per_block} (layers_per_block)")
        if len(self.cfg.block_out_channels) < 3:
            raise ValueError(f"enable_layer_cache: the model has {len(self.cfg.block_out_channels)} levels, the layer cache needs 3")
        self._set_layer_cache(depth)

    def disable_layer_cache(self) -> None:
        self._set_layer_cache(0)

    def _set_layer_cache(self, depth: int) -> None:
        if self.__dict__.get("_engine"):
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().lavie_unet_set_layer_cache(self._engine, depth), "lavie_unet_set_layer_cache")
        self.__dict__["_layer_cache"] = depth

    def layer_cache_bytes(self) -> int:
        """Device bytes the cache holds now (allocated by prepare / the first forward of a shape)."""
        handle = self.__dict__.get("_engine")
        return int(_lib.load().lavie_unet_layer_cache_bytes(handle)) if handle else 0

    def _layer_cache_mode(self, layer_cache) -> int:
        """forward's `layer_cache` argument as the engine's mode, after the checks that need no engine."""
        if layer_cache not in self.LAYER_CACHE_MODES:
            raise ValueError(f"layer_cache={layer_cache!r} must be None, 'refresh' or 'reuse'")
        if layer_cache is not None and not self.layer_cache:
            raise RuntimeError(f"layer_cache={layer_cache!r} needs enable_layer_cache(depth) first")
        if layer_cache is not None and self.__dict__.get("_graph"):
            raise RuntimeError("the layer cache has no graph-replayed form: enable_graph(False) first")
        return self.LAYER_CACHE_MODES[layer_cache]

    def enable_graph(self, on: bool = True) -> None:
        """Replay the forward from a hipGraph (lavie_unet_forward_graph).  While on, the timestep and the output live in
        per-shape buffers owned by this module, so the captured addresses repeat from call to call: the returned tensor is
        OVERWRITTEN by the next forward of the same shape (a denoise loop consumes it at once), and `sample` /
        `encoder_hidden_states` should be the same fp16 device tensors on every step (new addresses only cost a re-capture)."""
        self.__dict__["_graph"] = bool(on)
        if not on:
            self.__dict__["_graph_io"] = {}

    # ------------------------------------------------------------------ forward (unet.py:366-512)
    @torch.no_grad()
    def forward(self, sample: torch.Tensor, timestep: Union[torch.Tensor, float, int],
                encoder_hidden_states: torch.Tensor = None, class_labels: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, use_image_num: int = 0, return_dict: bool = True,
                layer_cache: Optional[str] = None):
        mode = self._layer_cache_mode(layer_cache)
        if class_labels is not None or attention_mask is not None or use_image_num:
            raise NotImplementedError("class_labels / attention_mask / use_image_num are outside the MI355X path")
        if sample.dim() != 5:
            raise ValueError(f"Expected sample to have ndim=5 [b, c, f, h, w], got ndim={sample.dim()}")
        if encoder_hidden_states is None or encoder_hidden_states.dim() != 3:
            raise ValueError("encoder_hidden_states [b, n, cross_attention_dim] is required")
        b, c, f, h, w = sample.shape
        if c != self.cfg.in_channels or encoder_hidden_states.shape[0] != b \
                or encoder_hidden_states.shape[2] != self.cfg.cross_attention_dim:
            raise ValueError("sample / encoder_hidden_states shapes do not match the model configuration")
        handle = self._ensure_engine()
        dev = self.device
        n_ctx = encoder_hidden_states.shape[1]
        self.prepare(b, f, h, w, n_ctx)

        x = sample.to(device=dev, dtype=torch.float16).contiguous()
        ctx = encoder_hidden_states.to(device=dev, dtype=torch.float16).contiguous()
        if torch.is_tensor(timestep):
            t = timestep.to(device=dev, dtype=torch.float32).reshape(-1)
        else:
            t = torch.tensor([float(timestep)], dtype=torch.float32, device=dev)
        lib = _lib.load()
        if self._graph:
            io = self._graph_io.get((b, f, h, w))
            if io is None:
                io = (torch.empty(b, dtype=torch.float32, device=dev),
                      torch.empty(b, self.cfg.out_channels, f, h, w, dtype=torch.float16, device=dev))
                self._graph_io[(b, f, h, w)] = io
            io[0].copy_(t.expand(b))                       # unet.py:426; contents change, the address does not
            t, out = io
            entry, what = lib.lavie_unet_forward_graph, "lavie_unet_forward_graph"
        else:
            t = t.expand(b).contiguous()                   # unet.py:426
            out = torch.empty(b, self.cfg.out_channels, f, h, w, dtype=torch.float16, device=dev)
            entry, what = lib.lavie_unet_forward, "lavie_unet_forward"
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if mode:
                _lib.check(lib.lavie_unet_forward_cached(handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                                         ctypes.c_void_p(ctx.data_ptr()), None, ctypes.c_void_p(out.data_ptr()),
                                                         b, f, h, w, n_ctx, mode, stream), "lavie_unet_forward_cached")
            else:
                _lib.check(entry(handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(t.data_ptr()),
                                 ctypes.c_void_p(ctx.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                 b, f, h, w, n_ctx, stream), what)
        if not return_dict:
            return (out,)
        return UNet3DConditionOutput(sample=out)

    # ------------------------------------------------------------------ checkpoint contract (unet.py:540-588)
    @classmethod
    def from_pretrained_2d(cls, pretrained_model_path: str, subfolder: Optional[str] = None):
        """SD-1.x `unet/config.json` + `diffusion_pytorch_model.bin`; temporal ('_temp') tensors keep this
        model's own initialisation, exactly as the reference does before `lavie_base.pt` is loaded on top."""
        if subfolder is not None:
            pretrained_model_path = os.path.join(pretrained_model_path, subfolder)
        config_file = os.path.join(pretrained_model_path, "config.json")
        if not os.path.isfile(config_file):
            raise RuntimeError(f"{config_file} does not exist")
        with open(config_file, "r") as fh:
            config = json.load(fh)
        keep = ("sample_size", "in_channels", "out_channels", "block_out_channels", "layers_per_block",
                "norm_num_groups", "norm_eps", "cross_attention_dim", "attention_head_dim")
        model = cls(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in config.items() if k in keep})
        model_file = os.path.join(pretrained_model_path, "diffusion_pytorch_model.bin")
        if not os.path.isfile(model_file):
            raise RuntimeError(f"{model_file} does not exist")
        state = torch.load(model_file, map_location="cpu", weights_only=True)
        for k, v in model.state_dict().items():
            if "_temp" in k:
                state[k] = v
        model.load_state_dict(state)
        return model
