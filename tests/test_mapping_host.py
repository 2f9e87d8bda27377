"""CPU: the image mapper (lavie_amd.mapping, the fork's base/pipelines/mapping.py:61-97) against the reference's recorded output,
its checkpoint loader, and how VideoGenPipeline widens the context with it (the denoiser stubbed: tests/test_gpu_image_cond.py runs
the loop)."""
import pytest
import torch

import golden_util as G
from lavie_amd import weights
from lavie_amd.mapping import MappingNetwork
from lavie_amd.scheduling_ddpm import DDPMScheduler

SAMPLE, STRIDE = 8192, 1_000_003


def sample(t):
    flat = t.reshape(-1)
    n = flat.numel()
    if n <= SAMPLE:
        return flat.clone()
    return flat[torch.arange(SAMPLE, dtype=torch.int64) * STRIDE % n].clone()


def rel_l2(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_parameter_names_and_shapes_are_the_reference_ones():
    fix = G.load("mapper.pt")
    sd = MappingNetwork().state_dict()
    assert list(sd) == fix["keys"]
    assert {k: list(v.shape) for k, v in sd.items()} == fix["shapes"]
    assert "text_proj.weight" in sd and "transformer_decoder.layers.11.norm3.bias" in sd


def test_forward_matches_the_reference():
    """Production configuration, seeded weights (synth_state_dict) and inputs, batch 2: the reference's fp32 output."""
    fix = G.load("mapper.pt")
    shapes = {k: tuple(v) for k, v in fix["shapes"].items()}
    net = MappingNetwork.from_checkpoint(weights.synth_state_dict(shapes, seed=fix["weight_seed"]))
    g = torch.Generator().manual_seed(fix["input_seed"])
    image = torch.randn(fix["batch"], 257, 1024, generator=g)
    text = torch.randn(fix["batch"], 77, 768, generator=g)
    with torch.no_grad():
        out = net(image, text)
    assert list(out.shape) == fix["out_shape"]
    assert rel_l2(sample(out), fix["out"]) <= 1e-5


def small_mapper(seed=0):
    torch.manual_seed(seed)
    return MappingNetwork(input_dim=32, output_dim=16, num_layers=2, num_heads=2, seq_len_in=9, seq_len_out=77)


def test_loader_strips_module_prefix_and_refuses_bad_keys(tmp_path):
    src = small_mapper(1)
    sd = {"module." + k: v.clone() for k, v in src.state_dict().items()}        # accelerate / DDP spelling
    path = str(tmp_path / "mapper.pt")
    torch.save(sd, path)
    for arg in (path, sd):
        net = MappingNetwork.from_checkpoint(arg, num_heads=2)
        assert not net.training
        assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), src.state_dict().values()))
    missing = {k: v for k, v in src.state_dict().items() if k != "transformer_decoder.layers.1.linear2.bias"}
    with pytest.raises(ValueError, match="layers.1.linear2.bias"):
        MappingNetwork.from_checkpoint(missing, num_heads=2)
    extra = dict(src.state_dict(), **{"mapper.extra": torch.zeros(1)})
    with pytest.raises(ValueError, match="mapper.extra"):
        MappingNetwork.from_checkpoint(extra, num_heads=2)


class _StubUNet:
    class config:
        in_channels, sample_size = 4, 64
    device = torch.device("cpu")

    def to(self, device):
        return self


def _pipe(monkeypatch, **kw):
    from lavie_amd.pipeline_videogen import VideoGenPipeline
    seen = {}

    def fake_denoise(self, latents, ctx, steps, scale, generator=None, callback=None, callback_steps=1, eta=0.0):
        seen["ctx"] = ctx.clone()
        return latents

    monkeypatch.setattr(VideoGenPipeline, "denoise", fake_denoise)
    return VideoGenPipeline(unet=_StubUNet(), scheduler=DDPMScheduler(), **kw), seen


def _call(pipe, **kw):
    return pipe(video_length=2, height=64, width=64, num_inference_steps=2, output_type="latent", **kw)


def test_pipeline_widens_the_context_from_image_embeds(monkeypatch):
    mapper = small_mapper(2)
    pipe, seen = _pipe(monkeypatch, mapper=mapper)
    g = torch.Generator().manual_seed(4)
    pe, ne = torch.randn(1, 77, 16, generator=g), torch.randn(1, 77, 16, generator=g)
    img = torch.randn(1, 9, 32, generator=g).half()                 # cast to the mapper's dtype on the way in
    _call(pipe, prompt_embeds=pe, negative_prompt_embeds=ne, image_embeds=img, guidance_scale=7.5)
    with torch.no_grad():
        want = torch.cat([torch.cat([ne, mapper(img.float(), ne)], 1), torch.cat([pe, mapper(img.float(), pe)], 1)]).half()
    assert seen["ctx"].shape == (2, 154, 16) and seen["ctx"].dtype == torch.float16
    assert torch.equal(seen["ctx"], want)                            # [uncond | cond], each [text | mapped image]
    _call(pipe, prompt_embeds=pe, image_embeds=img, guidance_scale=1.0)
    assert torch.equal(seen["ctx"], want[1:])                        # no guidance: the conditional half alone
    # two prompts, one image broadcast or one image each; num_images_per_prompt repeats each prompt's context
    pe2 = torch.randn(2, 77, 16, generator=g)
    img2 = torch.randn(2, 9, 32, generator=g)
    _call(pipe, prompt_embeds=pe2, image_embeds=img2, guidance_scale=1.0, num_images_per_prompt=2)
    with torch.no_grad():
        w2 = torch.cat([pe2, mapper(img2, pe2)], 1).half()
    assert torch.equal(seen["ctx"], w2.repeat_interleave(2, 0))
    _call(pipe, prompt_embeds=pe2, image_embeds=img2[:1], guidance_scale=1.0)
    with torch.no_grad():
        assert torch.equal(seen["ctx"], torch.cat([pe2, mapper(img2[:1].expand(2, -1, -1), pe2)], 1).half())
    with pytest.raises(ValueError):
        _call(pipe, prompt_embeds=pe2, image_embeds=torch.randn(3, 9, 32), guidance_scale=1.0)


def test_pipeline_without_mapper_ignores_the_image(monkeypatch):
    pipe, seen = _pipe(monkeypatch)
    pe, ne = torch.randn(1, 77, 16), torch.randn(1, 77, 16)
    _call(pipe, prompt_embeds=pe, negative_prompt_embeds=ne, image_tensor=torch.zeros(1, 3, 224, 224),
          image_embeds=torch.randn(1, 9, 32), guidance_scale=7.5)
    assert torch.equal(seen["ctx"], torch.cat([ne, pe]).half())


def test_pipeline_needs_clip_or_image_embeds_for_an_image(monkeypatch):
    pipe, _ = _pipe(monkeypatch, mapper=small_mapper())
    with pytest.raises(ValueError, match="clip_model"):
        _call(pipe, prompt_embeds=torch.randn(1, 77, 16), image_tensor=torch.zeros(1, 320, 512, 3, dtype=torch.uint8),
              guidance_scale=1.0)


def test_image_tensor_path_through_clip_vision_matches_image_embeds(monkeypatch):
    """A tiny random-init CLIPVisionModel + CLIPImageProcessor (built offline) on the fork's image layout, uint8 [1, 320, 512, 3]
    (load_and_transform_image): [1, 257, h] features, and the image_tensor path equals the image_embeds path."""
    import transformers
    torch.manual_seed(0)
    vcfg = transformers.CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                         image_size=224, patch_size=14)
    clip = transformers.CLIPVisionModel(vcfg).eval()
    proc = transformers.CLIPImageProcessor()
    image = torch.randint(0, 256, (1, 320, 512, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        tower = getattr(clip, "vision_model", clip)
        feats = tower(pixel_values=proc(images=image, return_tensors="pt").pixel_values).last_hidden_state
    assert feats.shape == (1, 257, 32)
    torch.manual_seed(5)
    mapper = MappingNetwork(input_dim=32, output_dim=16, num_layers=1, num_heads=2, seq_len_in=257, seq_len_out=77)
    pipe, seen = _pipe(monkeypatch, mapper=mapper, clip_model=clip, clip_processor=proc)
    pe, ne = torch.randn(1, 77, 16), torch.randn(1, 77, 16)
    _call(pipe, prompt_embeds=pe, negative_prompt_embeds=ne, image_tensor=image, guidance_scale=7.5)
    via_image = seen["ctx"]
    _call(pipe, prompt_embeds=pe, negative_prompt_embeds=ne, image_embeds=feats, guidance_scale=7.5)
    assert via_image.shape == (2, 154, 16)
    assert torch.equal(via_image, seen["ctx"])


def test_load_mapper_on_the_pipeline(monkeypatch, tmp_path):
    src = small_mapper(3)
    path = str(tmp_path / "mapper.pt")
    torch.save(src.state_dict(), path)
    pipe, _ = _pipe(monkeypatch)
    m = pipe.load_mapper(path, num_heads=2)
    assert pipe.mapper is m and not m.training
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), src.state_dict().values()))
