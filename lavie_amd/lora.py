"""LoRA adapters for the UNet engine: host-side key normalisation and loading (no GPU needed).

The fork fine-tunes the base UNet with a peft `LoraConfig(r=rank, lora_alpha=rank, target_modules=["to_k", "to_q", "to_v",
"to_out.0"])` (base/pipelines/fine_tuning.py:296-307) and saves the adapter with `save_lora_weights(..., safe_serialization=True)`
(:689-698).  `target_modules` matches on the name suffix, so every attn1 / attn2 / attn_temp projection of every transformer block
carries an adapter.  The engine serves it merged (`lavie_unet_lora_*`, `lavie_lora_merge_f16`): W = W0 + scale * B A with peft's
`scaling = lora_alpha / r`; up to `MAX_ADAPTERS` named adapters are blended in one fixed-order merge (`lavie_lora_merge_multi_f16`).

`normalize_lora_state_dict` maps the spellings in use to `{target weight name: (A [r, K], B [N, r], alpha or None)}` and refuses,
naming the key, what the engine could not serve exactly."""
import json
import os
import re
from typing import Dict, Mapping, Optional, Tuple

import torch

PREFIXES = ("base_model.model.", "unet.")
ADAPTER_FILES = ("pytorch_lora_weights.safetensors", "adapter_model.safetensors", "pytorch_lora_weights.bin", "adapter_model.bin")
MAX_RANK = 128
MAX_ADAPTERS = 8       # LAVIE_LORA_MAX_TERMS: the engine registry's slots

# <transformer>.transformer_blocks.0.<attn1 | attn2 | attn_temp | attn_temporal>.<to_q | to_k | to_v | to_out.0>
_TARGET = re.compile(r"^.+\.transformer_blocks\.0\.(attn1|attn2|attn_temp|attn_temporal)\.(to_q|to_k|to_v|to_out\.0)$")
# (module, role, adapter name) for the pair spellings; role A = down, B = up
_PAIR = (
    (re.compile(r"^(.+)\.lora_A(?:\.[^.]+)?\.weight$"), "A"),
    (re.compile(r"^(.+)\.lora_B(?:\.[^.]+)?\.weight$"), "B"),
    (re.compile(r"^(.+)\.lora\.down\.weight$"), "A"),
    (re.compile(r"^(.+)\.lora\.up\.weight$"), "B"),
    (re.compile(r"^(.+)\.lora_down\.weight$"), "A"),
    (re.compile(r"^(.+)\.lora_up\.weight$"), "B"),
)

LoraTensors = Dict[str, Tuple[torch.Tensor, torch.Tensor, Optional[float]]]


def is_target(weight_name: str) -> bool:
    """True for the state-dict name of a weight the engine can carry an adapter on (`....to_q.weight` etc.)."""
    return weight_name.endswith(".weight") and _TARGET.match(weight_name[: -len(".weight")]) is not None


def _strip(key: str) -> str:
    changed = True
    while changed:
        changed = False
        for p in PREFIXES:
            if key.startswith(p):
                key, changed = key[len(p):], True
    return key


def normalize_lora_state_dict(sd: Mapping[str, torch.Tensor], model_shapes: Optional[Mapping[str, tuple]] = None
                              ) -> LoraTensors:
    """{target weight name: (A fp32 [r, K], B fp32 [N, r], alpha or None)} from an adapter state dict in any of the spellings
    `lora_A[.<adapter>].weight` / `lora_B[...]`, `lora.down.weight` / `lora.up.weight`, `lora_down.weight` / `lora_up.weight`
    with an optional `<module>.alpha`, under an optional `unet.` / `base_model.model.` prefix.  `model_shapes` (state-dict name ->
    shape of the model the adapter goes on) turns on the module and shape checks.  Raises ValueError naming the offending key."""
    parts: Dict[str, Dict[str, Tuple[str, torch.Tensor]]] = {}
    alphas: Dict[str, Tuple[str, float]] = {}
    for key, value in sd.items():
        name = _strip(key)
        if name.endswith(".alpha"):
            module = name[: -len(".alpha")]
            alphas[module] = (key, float(torch.as_tensor(value).reshape(-1)[0]))
            continue
        for pattern, role in _PAIR:
            m = pattern.match(name)
            if m:
                slot = parts.setdefault(m.group(1), {})
                if role in slot:
                    raise ValueError(f"LoRA state dict: '{key}' repeats the {role} matrix of '{m.group(1)}' "
                                     f"(already given by '{slot[role][0]}'; several adapters at once are not supported)")
                slot[role] = (key, value)
                break
        else:
            raise ValueError(f"LoRA state dict: unknown key '{key}' (expected <module>.lora_A/lora_B[.<adapter>].weight, "
                             f"lora.down/lora.up.weight, lora_down/lora_up.weight or <module>.alpha)")
    out: LoraTensors = {}
    for module, slot in parts.items():
        if "A" not in slot or "B" not in slot:
            have, miss = ("A", "B") if "A" in slot else ("B", "A")
            raise ValueError(f"LoRA state dict: '{slot[have][0]}' has no {miss} (up/down) partner")
        key_a, a = slot["A"]
        key_b, b = slot["B"]
        target = module + ".weight"
        if model_shapes is not None and target not in model_shapes:
            raise ValueError(f"LoRA state dict: '{key_a}' names module '{module}', which the model does not have")
        if not is_target(target):
            raise ValueError(f"LoRA state dict: '{key_a}' is on '{module}', not a LoRA target "
                             f"(to_q / to_k / to_v / to_out.0 of attn1 / attn2 / attn_temp)")
        a = torch.as_tensor(a).detach()
        b = torch.as_tensor(b).detach()
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1]:
            raise ValueError(f"LoRA state dict: '{key_a}' {tuple(a.shape)} and '{key_b}' {tuple(b.shape)} are not a "
                             f"[r, K] / [N, r] pair")
        r = a.shape[0]
        if not 1 <= r <= MAX_RANK:
            raise ValueError(f"LoRA state dict: '{key_a}' has rank {r}; supported 1..{MAX_RANK}")
        if model_shapes is not None:
            n, k = tuple(model_shapes[target])[:2]
            if a.shape[1] != k or b.shape[0] != n:
                raise ValueError(f"LoRA state dict: '{key_a}' {tuple(a.shape)} / '{key_b}' {tuple(b.shape)} do not fit "
                                 f"'{target}' {tuple(model_shapes[target])}")
        alpha = alphas.pop(module, (None, None))[1]
        out[target] = (a.to(torch.float32).contiguous(), b.to(torch.float32).contiguous(), alpha)
    if alphas:
        key = next(iter(alphas.values()))[0]
        raise ValueError(f"LoRA state dict: '{key}' is an alpha without lora matrices")
    return out


_ADAPTER_KEY = re.compile(r"^.+\.lora_[AB]\.([^.]+)\.weight$")
_ADAPTER_ALPHA = re.compile(r"^(.+\.alpha)\.([^.]+)$")
DEFAULT_ADAPTER = "default"


def split_adapters(sd: Mapping[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """{adapter name: state dict} from a peft state dict that carries several adapters side by side
    (`<module>.lora_A.<adapter>.weight` / `lora_B.<adapter>.weight`, any prefix): each value goes through
    `normalize_lora_state_dict` on its own.  A per-adapter alpha is spelled `<module>.alpha.<adapter>` and comes out as
    `<module>.alpha`.  Keys without an adapter segment (`lora_A.weight`, `lora.down.weight`, `<module>.alpha`, ...) go under
    "default".  Adapters come out in the order of their first key; nothing is checked here."""
    out: Dict[str, Dict[str, torch.Tensor]] = {}
    for key, value in sd.items():
        m = _ADAPTER_KEY.match(key)
        if m:
            out.setdefault(m.group(1), {})[key] = value
            continue
        m = _ADAPTER_ALPHA.match(key)
        if m:
            out.setdefault(m.group(2), {})[m.group(1)] = value
            continue
        out.setdefault(DEFAULT_ADAPTER, {})[key] = value
    return out


def blend_factor(global_scale: float, weight: float, scale: float) -> float:
    """The factor the engine gives one adapter on one target: fp32, left to right, (global * weight) * scale."""
    import numpy as np
    return float(np.float32(np.float32(global_scale) * np.float32(weight)) * np.float32(scale))


def target_scales(lora: LoraTensors, alpha: Optional[float] = None) -> Dict[str, float]:
    """Per-target factor = peft's `scaling` = lora_alpha / r.  `alpha` (argument or adapter_config.json `lora_alpha`) overrides the
    per-module alphas; with neither it is 1.0, which is the fork's lora_alpha = r."""
    out = {}
    for name, (a, _, mod_alpha) in lora.items():
        use = alpha if alpha is not None else mod_alpha
        out[name] = 1.0 if use is None else float(use) / a.shape[0]
    return out


def split_peft_state_dict(sd: Mapping[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """`state_dict()` of a peft-wrapped UNet -> (base state dict under the model's own names, adapter state dict): the wrapped
    projections keep their weights under `<module>.base_layer.weight` / `.bias`, the adapter under `<module>.lora_A.<adapter>...`."""
    base: Dict[str, torch.Tensor] = {}
    lora: Dict[str, torch.Tensor] = {}
    for key, value in sd.items():
        name = _strip(key)
        if ".lora_" in name or name.endswith(".alpha"):
            lora[name] = value
        else:
            base[name.replace(".base_layer.", ".")] = value
    return base, lora


def load_lora_file(path: str) -> Tuple[Dict[str, torch.Tensor], Optional[float]]:
    """(adapter state dict, lora_alpha or None) from a `.safetensors` file, a `.bin` / `.pt` file (weights only), or a directory
    holding `pytorch_lora_weights.safetensors` (save_lora_weights) or `adapter_model.safetensors` (+ adapter_config.json)."""
    alpha = None
    if os.path.isdir(path):
        cfg = os.path.join(path, "adapter_config.json")
        if os.path.isfile(cfg):
            with open(cfg, "r") as fh:
                alpha = json.load(fh).get("lora_alpha")
        for f in ADAPTER_FILES:
            if os.path.isfile(os.path.join(path, f)):
                path = os.path.join(path, f)
                break
        else:
            raise FileNotFoundError(f"{path}: none of {', '.join(ADAPTER_FILES)}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path, device="cpu")
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    return dict(sd), (float(alpha) if alpha is not None else None)
