"""CPU: several named LoRA adapters — splitting a multi-adapter peft state dict, the blend factor, the model's adapter bookkeeping
without an engine, and the argument refusals of lavie_lora_merge_multi_f16 / lavie_unet_lora_*_slot* before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from lavie_amd import _lib, lora

BLK = "down_blocks.0.attentions.0.transformer_blocks.0"
SHAPES = {f"{BLK}.attn1.to_q.weight": (320, 320), f"{BLK}.attn2.to_k.weight": (320, 768)}
SMALL = dict(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
             down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"), up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"),
             init_weights=False)


def _pair(n, k, r, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, k, generator=g), torch.randn(n, r, generator=g)


@pytest.mark.parametrize("prefix", ["", "unet.", "base_model.model.", "base_model.model.unet."])
def test_split_adapters_two_peft_adapters(prefix):
    q, k = f"{BLK}.attn1.to_q", f"{BLK}.attn2.to_k"
    (aq1, bq1), (ak1, bk1), (aq2, bq2), (aq0, bq0) = _pair(320, 320, 4, 1), _pair(320, 768, 4, 2), _pair(320, 320, 8, 3), \
        _pair(320, 320, 2, 4)
    sd = {
        f"{prefix}{q}.lora_A.subject.weight": aq1, f"{prefix}{q}.lora_B.subject.weight": bq1,
        f"{prefix}{k}.lora_A.subject.weight": ak1, f"{prefix}{k}.lora_B.subject.weight": bk1,
        f"{prefix}{q}.lora_A.style.weight": aq2, f"{prefix}{q}.lora_B.style.weight": bq2,       # partial coverage: to_q only
        f"{prefix}{q}.alpha.style": torch.tensor(4.0),                                          # an alpha per adapter
        f"{prefix}{k}.alpha.subject": torch.tensor(2.0),
        f"{prefix}{q}.lora_A.weight": aq0, f"{prefix}{q}.lora_B.weight": bq0,                   # no adapter segment
    }
    with pytest.raises(ValueError, match="several adapters"):
        lora.normalize_lora_state_dict(sd, SHAPES)                   # unchanged: the whole dict is still refused
    parts = lora.split_adapters(sd)
    assert list(parts) == ["subject", "style", "default"]            # in the order of their first key
    got = {name: lora.normalize_lora_state_dict(part, SHAPES) for name, part in parts.items()}
    assert set(got["subject"]) == {q + ".weight", k + ".weight"}
    assert set(got["style"]) == set(got["default"]) == {q + ".weight"}
    assert torch.equal(got["subject"][k + ".weight"][0], ak1) and torch.equal(got["subject"][k + ".weight"][1], bk1)
    assert torch.equal(got["style"][q + ".weight"][0], aq2) and torch.equal(got["default"][q + ".weight"][1], bq0)
    assert got["subject"][k + ".weight"][2] == 2.0 and got["subject"][q + ".weight"][2] is None
    assert got["style"][q + ".weight"][2] == 4.0 and got["default"][q + ".weight"][2] is None
    assert lora.target_scales(got["style"])[q + ".weight"] == 4.0 / 8
    assert lora.target_scales(got["subject"]) == {q + ".weight": 1.0, k + ".weight": 2.0 / 4}


def test_split_adapters_one_adapter_and_other_spellings():
    q = f"{BLK}.attn1.to_q"
    a, b = _pair(320, 320, 4, 5)
    assert list(lora.split_adapters({f"{q}.lora_A.default.weight": a, f"{q}.lora_B.default.weight": b})) == ["default"]
    parts = lora.split_adapters({f"{q}.lora.down.weight": a, f"{q}.lora.up.weight": b, f"{q}.alpha": torch.tensor(8.0)})
    assert list(parts) == ["default"]
    assert lora.normalize_lora_state_dict(parts["default"], SHAPES)[q + ".weight"][2] == 8.0
    assert lora.split_adapters({}) == {}


def test_blend_factor_is_the_fp32_product_left_to_right():
    g, w, s = 1.5, 0.8, 1 / 3
    want = np.float32(np.float32(np.float32(g) * np.float32(w)) * np.float32(s))
    assert lora.blend_factor(g, w, s) == float(want)
    assert lora.blend_factor(g, 1.0, s) == float(np.float32(g) * np.float32(s))          # weight 1: the one-adapter product
    assert lora.blend_factor(g, 0.0, s) == 0.0 and lora.blend_factor(0.0, w, s) == 0.0


def _adapter(targets, r, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for t, (n, k) in targets.items():
        m = "unet." + t[: -len(".weight")]
        sd[m + ".lora_A.weight"] = torch.randn(r, k, generator=g)
        sd[m + ".lora_B.weight"] = torch.randn(n, r, generator=g)
    return sd


def test_adapter_bookkeeping_without_an_engine():
    from lavie_amd.unet import UNet3DConditionModel
    from lavie_amd.vsr.unet import UNet3DVSRModel
    net = UNet3DConditionModel(**SMALL)
    q, k = f"{BLK}.attn1.to_q.weight", f"{BLK}.attn2.to_k.weight"
    both, only_k = {q: (256, 256), k: (256, 128)}, {k: (256, 128)}
    assert net._lora == {} and net.get_list_adapters() == [] and net.get_active_adapters() == []
    net.load_lora(_adapter(both, 4, 1), adapter_name="a")
    net.load_lora(_adapter(only_k, 2, 2), scale=0.5, adapter_name="b")
    assert net.get_list_adapters() == net.get_active_adapters() == ["a", "b"]
    assert set(net._lora) == {q, k} and set(net._lora[q]) == {"a"} and set(net._lora[k]) == {"a", "b"}
    assert net._lora_slots() == [("a", 0, 1.0), ("b", 1, 0.5)] and net.lora_scale == 1.0      # a named load leaves the global scale
    net.set_adapters(["b", "a"], [0.25, -2.0])
    assert net._lora_slots() == [("a", 0, -2.0), ("b", 1, 0.25)]                              # blend order = slot order
    net.set_adapters("a")
    assert net.get_active_adapters() == ["a"] and net.get_list_adapters() == ["a", "b"]
    assert net._lora_slots() == [("a", 0, 1.0), ("b", 1, 0.0)]                                # resident, contributes nothing
    net.set_adapters([])
    assert net.get_active_adapters() == []
    net.set_adapters(["a", "b"], 0.5)
    assert net._lora_slots() == [("a", 0, 0.5), ("b", 1, 0.5)]
    # replacing keeps the slot; deleting frees it for the next new name
    net.load_lora(_adapter(only_k, 8, 3), adapter_name="a")
    assert net._lora_slots() == [("a", 0, 1.0), ("b", 1, 0.5)] and set(net._lora) == {k} and net._lora[k]["a"][0].shape[0] == 8
    net.delete_adapters("a")
    assert net.get_list_adapters() == ["b"] and set(net._lora[k]) == {"b"}
    net.load_lora(_adapter(both, 4, 4), adapter_name="c")
    assert net._lora_slots() == [("c", 0, 1.0), ("b", 1, 0.5)]
    for bad in ("nope", ["b", "nope"]):
        with pytest.raises(ValueError, match="nope"):
            net.set_adapters(bad)
        with pytest.raises(ValueError, match="nope"):
            net.delete_adapters(bad)
    with pytest.raises(ValueError, match="twice"):
        net.set_adapters(["b", "b"])
    with pytest.raises(ValueError, match="2 names, 1 weights"):
        net.set_adapters(["b", "c"], [1.0])
    for w in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="not finite"):
            net.set_adapters(["b", "c"], [1.0, w])
    assert net._lora_slots() == [("c", 0, 1.0), ("b", 1, 0.5)]                                # a refused call changes nothing
    # the limit: eight, and the ninth is refused by name of the limit, leaving the eight
    for i in range(6):
        net.load_lora(_adapter(only_k, 1, 10 + i), adapter_name=f"x{i}")
    assert len(net.get_list_adapters()) == 8 and [s for _, s, _ in net._lora_slots()] == list(range(8))
    with pytest.raises(ValueError, match="8 adapters"):
        net.load_lora(_adapter(only_k, 1, 20), adapter_name="ninth")
    assert len(net.get_list_adapters()) == 8 and "ninth" not in net._lora[k]
    net.load_lora(_adapter(only_k, 1, 21), adapter_name="x0")                                  # replacing one of the eight is fine
    # adapter_name=None replaces everything, as it always did
    net.load_lora(_adapter(both, 4, 5), scale=0.75)
    assert net.get_list_adapters() == ["default"] and net.lora_scale == 0.75 and set(net._lora) == {q, k}
    net.load_lora(_adapter(only_k, 4, 6), adapter_name="more")
    net.unload_lora()
    assert net._lora == {} and net.get_list_adapters() == [] and net.lora_scale == 1.0
    vsr = UNet3DVSRModel(init_weights=False, sample_size=8, block_out_channels=(256,), cross_attention_dim=1024,
                         layers_per_block=1, down_block_types=("CrossAttnDownBlock3D",), up_block_types=("CrossAttnUpBlock3D",),
                         only_cross_attention=(True,), num_class_embeds=None, down_temporal_idx=(), mid_temporal=False,
                         up_temporal_idx=())
    with pytest.raises(NotImplementedError):
        vsr.load_lora({}, adapter_name="a")


def test_abi_refusals_before_any_device_call():
    """The new entry points check their arguments on the host: fake pointers are never dereferenced, and a handle from
    lavie_unet_create (no GPU, not finalized) is enough for the slot calls."""
    from lavie_amd.unet import UNet3DConditionModel
    lib = _lib.load()
    fake, odd = 256, 256 + 4

    def refused(rc, text):
        assert rc != 0
        msg = lib.lavie_last_error().decode()
        assert text in msg, msg

    def terms(*ts):
        arr = (_lib.LoraTermC * max(1, len(ts)))()
        for i, (a, b, r, s) in enumerate(ts):
            arr[i].A, arr[i].B, arr[i].r, arr[i].scale = a, b, r, s
        return arr

    def merge(ts, n=None, w0=fake, out=fake, N=64, K=64):
        return lib.lavie_lora_merge_multi_f16(w0, terms(*ts), len(ts) if n is None else n, out, N, K, None)

    ok = (fake, fake, 4, 1.0)
    refused(merge([]), "0 terms outside 1..8")
    refused(merge([ok] * 9), "9 terms outside 1..8")
    refused(merge([ok, (fake, fake, 0, 1.0)]), "term 1: rank 0 outside 1..128")
    refused(merge([(fake, fake, 129, 1.0), ok]), "term 0: rank 129 outside 1..128")
    refused(merge([ok, ok], K=60), "multiple of 8")
    refused(merge([ok, (odd, fake, 4, 1.0)]), "term 1: A must be 16-byte aligned")
    refused(merge([ok], w0=odd), "W0 / out must be 16-byte aligned")
    refused(merge([ok, (None, fake, 4, 1.0)]), "term 1: null tensor")
    refused(merge([(fake, None, 4, 1.0)]), "term 0: null tensor")
    refused(merge([ok], w0=None), "null tensor")
    refused(merge([ok], out=None), "null tensor")
    refused(lib.lavie_lora_merge_multi_f16(fake, None, 1, fake, 64, 64, None), "null term list")
    refused(merge([ok, (fake, fake, 4, float("nan"))]), "term 1: scale is not finite")
    refused(merge([(fake, fake, 4, float("inf")), ok]), "term 0: scale is not finite")
    refused(merge([ok, (fake, fake, 200, 0.0)]), "term 1: rank 200")          # a zero-scale term is checked like any other

    net = UNet3DConditionModel(**SMALL)
    handle = ctypes.c_void_p()
    cfg = net._config_c()
    assert lib.lavie_unet_create(ctypes.byref(cfg), ctypes.byref(handle)) == 0
    good = f"{BLK}.attn1.to_q.weight".encode()
    try:
        for slot in (-1, 8):
            refused(lib.lavie_unet_lora_set_slot(handle, slot, good, fake, fake, fake, 4, 1.0, None), f"slot {slot} outside 0..7")
            refused(lib.lavie_unet_lora_clear_slot(handle, slot, None, None), f"slot {slot} outside 0..7")
            refused(lib.lavie_unet_lora_set_slot_weight(handle, slot, 1.0), f"slot {slot} outside 0..7")
        for w in (float("nan"), float("inf"), float("-inf")):
            refused(lib.lavie_unet_lora_set_slot_weight(handle, 3, w), "not finite")
        refused(lib.lavie_unet_lora_set_slot(handle, 7, f"{BLK}.ff.net.2.weight".encode(), fake, fake, fake, 4, 1.0, None),
                "not a LoRA target")
        refused(lib.lavie_unet_lora_set_slot(handle, 7, b"no.such.key.weight", fake, fake, fake, 4, 1.0, None), "unknown state-dict key")
        refused(lib.lavie_unet_lora_clear_slot(handle, 2, b"down_blocks.0.resnets.0.conv1.weight", None), "not a LoRA target")
        refused(lib.lavie_unet_lora_set_slot(handle, 1, good, fake, fake, fake, 0, 1.0, None), "rank 0 outside 1..128")
        refused(lib.lavie_unet_lora_set_slot(handle, 1, good, fake, fake, fake, 129, 1.0, None), "rank 129 outside 1..128")
        refused(lib.lavie_unet_lora_set_slot(handle, 1, good, fake, None, fake, 4, 1.0, None), "null argument")
        refused(lib.lavie_unet_lora_set_slot(handle, 1, good, fake, fake, fake, 4, float("nan"), None), "not finite")
        refused(lib.lavie_unet_lora_set_slot(handle, 1, good, fake, fake, fake, 4, 1.0, None), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_clear_slot(handle, 1, None, None), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_set_slot_weight(handle, 1, 0.5), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_set_slot(None, 1, good, fake, fake, fake, 4, 1.0, None), "null handle")
        refused(lib.lavie_unet_lora_clear_slot(None, 1, None, None), "null handle")
        refused(lib.lavie_unet_lora_set_slot_weight(None, 1, 0.5), "null handle")
    finally:
        lib.lavie_unet_destroy(handle)


def test_header_and_binding_agree_on_the_term_struct():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lavie_hip.h")).read()
    assert int(re.search(r"#define LAVIE_LORA_MAX_TERMS (\d+)", hdr).group(1)) == _lib.LORA_MAX_TERMS == lora.MAX_ADAPTERS == 8
    body = hdr[hdr.index("typedef struct lavie_lora_term {"):hdr.index("} lavie_lora_term;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [m.strip(" *") for m in re.findall(r"(?:const float\*|int|float)\s+([^;]+);", body)]
    assert names == [n for n, _ in _lib.LoraTermC._fields_]
    assert ctypes.sizeof(_lib.LoraTermC) == 24
