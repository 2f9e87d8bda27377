"""CPU: LoRA adapter host logic — key normalisation, peft state-dict split, file loading, and the C ABI's argument refusals."""
import ctypes
import json

import pytest
import torch

from lavie_amd import _lib, lora

BLK = "down_blocks.0.attentions.0.transformer_blocks.0"
SHAPES = {
    f"{BLK}.attn1.to_q.weight": (320, 320),
    f"{BLK}.attn2.to_k.weight": (320, 768),
    f"{BLK}.attn_temp.to_out.0.weight": (320, 320),
    f"{BLK}.attn_temp.to_out.0.bias": (320,),
    f"{BLK}.ff.net.2.weight": (320, 1280),
}


def _pair(n, k, r, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, k, generator=g), torch.randn(n, r, generator=g)


def _spellings():
    """(state dict, expected {target: (A, B, alpha)}) in every accepted spelling."""
    a1, b1 = _pair(320, 320, 4, 1)
    a2, b2 = _pair(320, 768, 8, 2)
    a3, b3 = _pair(320, 320, 16, 3)
    want = {f"{BLK}.attn1.to_q.weight": (a1, b1, None), f"{BLK}.attn2.to_k.weight": (a2, b2, 4.0),
            f"{BLK}.attn_temp.to_out.0.weight": (a3, b3, None)}
    mods = [f"{BLK}.attn1.to_q", f"{BLK}.attn2.to_k", f"{BLK}.attn_temp.to_out.0"]
    pairs = [(a1, b1), (a2, b2), (a3, b3)]
    forms = [
        ("unet.{m}.lora_A.weight", "unet.{m}.lora_B.weight"),                         # save_lora_weights (peft keys)
        ("base_model.model.{m}.lora_A.default.weight", "base_model.model.{m}.lora_B.default.weight"),   # peft model
        ("{m}.lora.down.weight", "{m}.lora.up.weight"),
        ("{m}.lora_down.weight", "{m}.lora_up.weight"),
        ("base_model.model.unet.{m}.lora_A.weight", "base_model.model.unet.{m}.lora_B.weight"),
    ]
    out = []
    for fa, fb in forms:
        sd = {}
        for m, (a, b) in zip(mods, pairs):
            sd[fa.format(m=m)] = a.half()
            sd[fb.format(m=m)] = b
        prefix = fa[: fa.index("{m}")]
        sd[f"{prefix}{mods[1]}.alpha"] = torch.tensor(4.0)
        out.append((sd, want))
    return out


@pytest.mark.parametrize("case", range(5))
def test_normalisation_round_trips_every_spelling(case):
    sd, want = _spellings()[case]
    got = lora.normalize_lora_state_dict(sd, SHAPES)
    assert set(got) == set(want)
    for name, (a, b, alpha) in want.items():
        ga, gb, galpha = got[name]
        assert ga.dtype == gb.dtype == torch.float32 and ga.is_contiguous() and gb.is_contiguous()
        assert torch.equal(ga, a.half().float()) and torch.equal(gb, b)
        assert galpha == alpha
    scales = lora.target_scales(got)
    assert scales[f"{BLK}.attn1.to_q.weight"] == 1.0                 # no alpha: the fork's lora_alpha = r
    assert scales[f"{BLK}.attn2.to_k.weight"] == 4.0 / 8             # peft scaling = alpha / r
    over = lora.target_scales(got, alpha=32)                          # adapter_config.json lora_alpha overrides
    assert over[f"{BLK}.attn_temp.to_out.0.weight"] == 2.0 and over[f"{BLK}.attn1.to_q.weight"] == 8.0


def test_normalisation_refuses_bad_adapters_by_name():
    a, b = _pair(320, 320, 4, 5)
    m = f"{BLK}.attn1.to_q"
    cases = [
        ({f"{m}.lora_A.weight": a, f"{m}.lora_B.weight": b, f"{m}.lora_C.weight": a}, f"{m}.lora_C.weight"),     # unknown key
        ({f"{m}.lora_A.weight": a}, f"{m}.lora_A.weight"),                                                      # unpaired
        ({f"{m}.lora_up.weight": b}, f"{m}.lora_up.weight"),
        ({f"{BLK}.ff.net.2.lora_A.weight": torch.zeros(4, 1280), f"{BLK}.ff.net.2.lora_B.weight": torch.zeros(320, 4)},
         f"{BLK}.ff.net.2.lora_A.weight"),                                                                       # not a target
        ({f"{BLK}.attn1.to_k.lora_A.weight": a, f"{BLK}.attn1.to_k.lora_B.weight": b}, f"{BLK}.attn1.to_k.lora_A.weight"),  # not in model
        ({f"{m}.lora_A.weight": torch.zeros(4, 768), f"{m}.lora_B.weight": b}, f"{m}.lora_A.weight"),           # K mismatch
        ({f"{m}.lora_A.weight": a, f"{m}.lora_B.weight": torch.zeros(640, 4)}, f"{m}.lora_A.weight"),          # N mismatch
        ({f"{m}.lora_A.weight": a, f"{m}.lora_B.weight": torch.zeros(320, 5)}, f"{m}.lora_A.weight"),          # rank mismatch
        ({f"{m}.lora_A.weight": torch.zeros(129, 320), f"{m}.lora_B.weight": torch.zeros(320, 129)}, f"{m}.lora_A.weight"),
        ({f"{m}.lora_A.weight": a, f"{m}.lora_B.weight": b, f"{BLK}.attn2.to_k.alpha": torch.tensor(1.0)},
         f"{BLK}.attn2.to_k.alpha"),                                                                             # orphan alpha
        ({f"{m}.lora_A.weight": a, f"{m}.lora_A.other.weight": a, f"{m}.lora_B.weight": b}, f"{m}.lora_A.other.weight"),  # two adapters
    ]
    for sd, key in cases:
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            lora.normalize_lora_state_dict(sd, SHAPES)


def test_is_target():
    assert lora.is_target(f"{BLK}.attn_temp.to_v.weight")
    assert lora.is_target("mid_block.attentions.0.transformer_blocks.0.attn2.to_out.0.weight")
    assert lora.is_target(f"{BLK}.attn_temporal.to_q.weight")        # the VSR model's spelling
    assert not lora.is_target(f"{BLK}.attn1.to_out.0.bias")
    assert not lora.is_target(f"{BLK}.ff.net.0.proj.weight")
    assert not lora.is_target("down_blocks.0.attentions.0.proj_in.weight")


def test_split_peft_state_dict():
    a, b = _pair(320, 320, 4, 7)
    w, bias, g = torch.randn(320, 320), torch.randn(320), torch.randn(320)
    sd = {
        f"base_model.model.{BLK}.attn1.to_q.base_layer.weight": w,
        f"base_model.model.{BLK}.attn1.to_q.lora_A.default.weight": a,
        f"base_model.model.{BLK}.attn1.to_q.lora_B.default.weight": b,
        f"base_model.model.{BLK}.attn1.to_out.0.base_layer.weight": w,
        f"base_model.model.{BLK}.attn1.to_out.0.base_layer.bias": bias,
        f"base_model.model.{BLK}.norm1.weight": g,
    }
    base, adapter = lora.split_peft_state_dict(sd)
    assert set(base) == {f"{BLK}.attn1.to_q.weight", f"{BLK}.attn1.to_out.0.weight", f"{BLK}.attn1.to_out.0.bias",
                         f"{BLK}.norm1.weight"}
    assert base[f"{BLK}.attn1.to_out.0.bias"] is bias and base[f"{BLK}.norm1.weight"] is g
    got = lora.normalize_lora_state_dict(adapter, SHAPES)
    assert list(got) == [f"{BLK}.attn1.to_q.weight"]
    assert torch.equal(got[f"{BLK}.attn1.to_q.weight"][0], a) and torch.equal(got[f"{BLK}.attn1.to_q.weight"][1], b)


def test_load_lora_file_formats(tmp_path):
    from safetensors.torch import save_file
    sd, want = _spellings()[0]
    sd = {k: v.contiguous() for k, v in sd.items()}
    save_file(sd, str(tmp_path / "a.safetensors"))
    torch.save(sd, str(tmp_path / "a.bin"))
    d = tmp_path / "dir"
    d.mkdir()
    save_file(sd, str(d / "pytorch_lora_weights.safetensors"))
    p = tmp_path / "peft"
    p.mkdir()
    save_file(sd, str(p / "adapter_model.safetensors"))
    (p / "adapter_config.json").write_text(json.dumps({"r": 8, "lora_alpha": 16}))
    for path, alpha in ((tmp_path / "a.safetensors", None), (tmp_path / "a.bin", None), (d, None), (p, 16.0)):
        got, got_alpha = lora.load_lora_file(str(path))
        assert got_alpha == alpha
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(FileNotFoundError):
        lora.load_lora_file(str(tmp_path))


def test_abi_refusals_before_any_device_call():
    """lavie_unet_lora_* check their arguments on the host: a handle from lavie_unet_create (no GPU, not finalized) is enough."""
    from lavie_amd.unet import UNet3DConditionModel
    lib = _lib.load()
    net = UNet3DConditionModel(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
                               down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
                               up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"), init_weights=False)
    handle = ctypes.c_void_p()
    cfg = net._config_c()
    assert lib.lavie_unet_create(ctypes.byref(cfg), ctypes.byref(handle)) == 0
    fake = ctypes.c_void_p(256)            # never dereferenced: every refusal comes before a HIP call
    good = f"{BLK}.attn1.to_q.weight".encode()

    def refused(rc, text):
        assert rc != 0
        msg = lib.lavie_last_error().decode()
        assert text in msg, msg

    try:
        refused(lib.lavie_unet_lora_set(handle, b"no.such.key.weight", fake, fake, fake, 4, 1.0, None), "unknown state-dict key")
        refused(lib.lavie_unet_lora_set(handle, f"{BLK}.ff.net.2.weight".encode(), fake, fake, fake, 4, 1.0, None),
                "not a LoRA target")
        refused(lib.lavie_unet_lora_set(handle, f"{BLK}.attn1.to_out.0.bias".encode(), fake, fake, fake, 4, 1.0, None),
                "not a LoRA target")
        refused(lib.lavie_unet_lora_set(handle, good, fake, fake, fake, 0, 1.0, None), "rank 0 outside 1..128")
        refused(lib.lavie_unet_lora_set(handle, good, fake, fake, fake, 129, 1.0, None), "rank 129 outside 1..128")
        refused(lib.lavie_unet_lora_set(handle, good, None, fake, fake, 4, 1.0, None), "null argument")
        refused(lib.lavie_unet_lora_set(handle, good, fake, None, fake, 4, 1.0, None), "null argument")
        refused(lib.lavie_unet_lora_set(handle, good, fake, fake, None, 4, 1.0, None), "null argument")
        refused(lib.lavie_unet_lora_set(handle, None, fake, fake, fake, 4, 1.0, None), "null argument")
        refused(lib.lavie_unet_lora_set(handle, good, fake, fake, fake, 4, float("nan"), None), "not finite")
        refused(lib.lavie_unet_lora_set(handle, good, fake, fake, fake, 4, float("inf"), None), "not finite")
        refused(lib.lavie_unet_lora_set(handle, good, fake, fake, fake, 4, 1.0, None), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_set(None, good, fake, fake, fake, 4, 1.0, None), "null handle")
        refused(lib.lavie_unet_lora_clear(handle, b"down_blocks.0.resnets.0.conv1.weight", None), "not a LoRA target")
        refused(lib.lavie_unet_lora_clear(handle, None, None), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_set_scale(handle, float("-inf")), "not finite")
        refused(lib.lavie_unet_lora_set_scale(handle, 0.5), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_apply(handle, None), "lavie_unet_finalize first")
        refused(lib.lavie_unet_lora_apply(None, None), "null handle")
        # the standalone merge operator refuses before launching
        refused(lib.lavie_lora_merge_f16(fake, fake, fake, fake, 64, 64, 0, 1.0, None), "rank 0")
        refused(lib.lavie_lora_merge_f16(fake, fake, fake, fake, 64, 60, 4, 1.0, None), "multiple of 8")
        refused(lib.lavie_lora_merge_f16(None, fake, fake, fake, 64, 64, 4, 1.0, None), "null tensor")
        refused(lib.lavie_lora_merge_f16(fake, fake, fake, fake, 64, 64, 4, float("nan"), None), "not finite")
    finally:
        lib.lavie_unet_destroy(handle)


def test_model_level_refusals_without_a_gpu():
    from lavie_amd.unet import UNet3DConditionModel
    from lavie_amd.vsr.unet import UNet3DVSRModel
    net = UNet3DConditionModel(sample_size=8, block_out_channels=(256, 512), cross_attention_dim=128,
                               down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
                               up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"), init_weights=False)
    blk = "down_blocks.0.attentions.0.transformer_blocks.0"
    a, b = _pair(256, 256, 4, 9)
    with pytest.raises(ValueError, match="attn1.to_q.lora_A.weight"):
        net.load_lora({f"{blk}.attn1.to_q.lora_A.weight": a, f"{blk}.attn1.to_q.lora_B.weight": torch.zeros(512, 4)})
    with pytest.raises(ValueError, match="not finite"):
        net.set_lora_scale(float("nan"))
    # no engine yet: the adapter is held on the host and registered at the first build
    net.load_lora({f"unet.{blk}.attn1.to_q.lora_A.weight": a, f"unet.{blk}.attn1.to_q.lora_B.weight": b}, scale=0.5)
    assert set(net._lora) == {f"{blk}.attn1.to_q.weight"} and net.lora_scale == 0.5
    net.set_lora_scale(0.25)
    assert net.lora_scale == 0.25
    net.unload_lora()
    assert net._lora == {} and net.lora_scale == 1.0
    vsr = UNet3DVSRModel(init_weights=False, sample_size=8, block_out_channels=(256,), cross_attention_dim=1024,
                         layers_per_block=1, down_block_types=("CrossAttnDownBlock3D",), up_block_types=("CrossAttnUpBlock3D",),
                         only_cross_attention=(True,), num_class_embeds=None, down_temporal_idx=(), mid_temporal=False,
                         up_temporal_idx=())
    with pytest.raises(NotImplementedError):
        vsr.load_lora({})
