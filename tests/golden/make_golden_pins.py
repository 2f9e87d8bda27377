"""Generates tests/golden/oracle_pins_base.pt and oracle_pins_stages.pt: the reference outputs behind
tests/test_oracle_vs_reference.py, so that those pins run from the repository alone.  Needs the reference checkout (the same modules make_golden*.py import, under
tests/refshim).  Run from the repo root:  python tests/golden/make_golden_pins.py

Data only, as in make_golden.py: the reference's fp32 outputs and its state-dict shapes.  Weights are the fp32
`lavie_amd.weights.synth_state_dict(shapes, seed)` recipe and inputs come from seeded CPU generators; the test module
rebuilds both with the same recipes.  Outputs larger than SAMPLE elements are stored as the fixed spread of SAMPLE
elements that test_oracle_vs_reference.sample() picks (index arithmetic, no generator); smaller ones whole."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import refbuild  # noqa: E402
import refimport  # noqa: E402
from lavie_amd import weights  # noqa: E402
from make_golden import module_shapes, save  # noqa: E402
from test_oracle_vs_reference import SMALL, sample  # noqa: E402

REF_ROOT = os.path.dirname(os.path.dirname(refimport.REF))


def synth(shapes, seed):
    return weights.synth_state_dict(shapes, seed)


def load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@torch.no_grad()
def main():
    m = refimport.load()
    from rotary_embedding_torch import RotaryEmbedding
    out = {}

    # whole base UNet at a small width (refbuild: synth_state_dict(seed 3), fp32)
    net, _ = refbuild.reference_unet(SMALL, seed=3)
    out["small_unet_shapes"] = module_shapes(net)
    ys = {}
    for t in (980, 500, 0):
        g = torch.Generator().manual_seed(10 + t)
        x = torch.randn(2, 4, 16, 8, 8, generator=g)
        ctx = torch.randn(2, 77, SMALL.cross_attention_dim, generator=g)
        ys[t] = sample(net(x, torch.tensor(t), encoder_hidden_states=ctx).sample)
    out["small_unet"] = ys
    del net

    # ResnetBlock3D, Upsample3D, Downsample3D (resnet.py, direct import)
    cases = {}
    for cin, cout in ((64, 128), (64, 64)):
        blk = m.resnet.ResnetBlock3D(in_channels=cin, out_channels=cout, temb_channels=256, groups=32, eps=1e-5).eval()
        shapes = module_shapes(blk)
        blk.load_state_dict(synth(shapes, cin + cout))
        g = torch.Generator().manual_seed(cin + cout)
        x = torch.randn(2, cin, 4, 8, 8, generator=g) * torch.linspace(0.5, 2.0, 4).reshape(1, 1, 4, 1, 1)
        temb = torch.randn(2, 256, generator=g)
        cases[cin, cout] = dict(shapes=shapes, y=sample(blk(x, temb)))
    out["resnet"] = cases
    up = m.resnet.Upsample3D(64, use_conv=True, out_channels=64).eval()
    dn = m.resnet.Downsample3D(64, use_conv=True, out_channels=64, padding=1, name="op").eval()
    up_shapes, dn_shapes = module_shapes(up), module_shapes(dn)
    up.load_state_dict(synth(up_shapes, 1))
    dn.load_state_dict(synth(dn_shapes, 2))
    x = torch.randn(1, 64, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    out["sampler"] = dict(up_shapes=up_shapes, dn_shapes=dn_shapes, up=sample(up(x)), dn=sample(dn(x)))

    # TemporalAttention: 64 sequences per case
    cases = {}
    for c, frames in ((320, 16), (640, 16), (1280, 16), (320, 61)):
        att = m.attention.TemporalAttention(query_dim=c, heads=8, dim_head=c // 8, rotary_emb=RotaryEmbedding(32)).eval()
        shapes = module_shapes(att)
        att.load_state_dict(synth(shapes, c + frames))
        x = torch.randn(64, frames, c, generator=torch.Generator().manual_seed(c + frames))
        cases[c, frames] = dict(shapes=shapes, y=sample(att(x)))
    out["temporal_attention"] = cases

    # relative-position bucket tables
    tables = {}
    for n in (16, 61):
        q = torch.arange(n)
        rel = q.reshape(1, n) - q.reshape(n, 1)
        tables[n] = m.attention.RelativePositionBias._relative_position_bucket(rel, num_buckets=32, max_distance=32).to(torch.int8)
    out["rel_pos_buckets"] = tables

    # Transformer3DModel block order
    tr = m.attention.Transformer3DModel(8, 40, in_channels=320, num_layers=1, cross_attention_dim=768,
                                        norm_num_groups=32, rotary_emb=RotaryEmbedding(32)).eval()
    shapes = module_shapes(tr)
    tr.load_state_dict(synth(shapes, 5))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 320, 16, 8, 8, generator=g) * torch.linspace(0.5, 2.0, 16).reshape(1, 1, 16, 1, 1)
    ctx = torch.randn(2, 77, 768, generator=g)
    out["transformer3d"] = dict(shapes=shapes, y=sample(tr(x, encoder_hidden_states=ctx, use_image_num=0).sample))
    save("oracle_pins_base.pt", out)
    out = {}

    # the reference's vendored DDIMScheduler: timesteps and every step the test takes, in the test's order
    ddim = refimport.load_vsr_ddim()
    ref = ddim(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear", clip_sample=False,
               set_alpha_to_one=False, steps_offset=1)
    ref.set_timesteps(50)
    steps = {"timesteps": [int(t) for t in ref.timesteps]}
    g = torch.Generator().manual_seed(77)
    wants = []
    for t in steps["timesteps"][1::7]:
        x, eps, z = (torch.randn(2, 4, 3, 8, 8, generator=g) for _ in range(3))
        for eta in (0.0, 1.0):
            wants.append(ref.step(eps, t, x, eta=eta, variance_noise=z if eta > 0 else None).prev_sample)
    steps["epsilon"] = wants
    for kind in ("v_prediction", "sample"):
        pref = ddim(num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="linear", clip_sample=False,
                    set_alpha_to_one=False, steps_offset=1, prediction_type=kind)
        pref.set_timesteps(50)
        wants = []
        for t in [int(t) for t in pref.timesteps][1::7]:
            x, mm, z = (torch.randn(2, 4, 3, 8, 8, generator=g) for _ in range(3))
            for eta in (0.0, 1.0):
                wants.append(pref.step(mm, t, x, eta=eta, variance_noise=z if eta > 0 else None).prev_sample)
        steps[kind] = wants
    out["ddim"] = steps

    # frame-interpolation UNet at a small width (interpolation/models)
    mi = refimport.load("interpolation")
    net = mi.unet.UNet3DConditionModel(sample_size=8, in_channels=8, out_channels=4, block_out_channels=(64, 128),
                                       down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
                                       up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"), layers_per_block=1,
                                       cross_attention_dim=64, attention_head_dim=8, use_first_frame=True).eval()
    shapes = module_shapes(net)
    net.load_state_dict(synth(shapes, 8))
    g = torch.Generator().manual_seed(5)
    x, ctx = torch.randn(2, 8, 7, 8, 8, generator=g), torch.randn(2, 77, 64, generator=g)
    out["interp_unet"] = dict(shapes=shapes, y=sample(net(x, torch.tensor(500), encoder_hidden_states=ctx).sample))

    # the interpolation stage's in-tree diffusion package: respaced tables and a 10-step DDIM loop around a toy denoiser
    rd = refimport.load_interp_diffusion()
    from oracle import interp_ddim as D
    tables = {}
    for n in ("50", "25", "7"):
        r = rd.create_diffusion(n)
        tables[n] = dict(timestep_map=[int(v) for v in r.timestep_map],
                         alphas_cumprod=torch.from_numpy(np.asarray(r.alphas_cumprod, dtype=np.float64)))
    g = torch.Generator().manual_seed(0)
    W = torch.randn(4, 8, generator=g) * 0.05
    toy = lambda x, t, c: (torch.einsum("oc,bcfhw->bofhw", W, x) * (1 + t.float().reshape(-1, 1, 1, 1, 1) / 1000)
                           + 0.1 * c.mean(dim=(1, 2)).reshape(-1, 1, 1, 1, 1))

    def fwd_cfg(x, t, encoder_hidden_states=None, class_labels=None, cfg_scale=4.0):
        return D.forward_with_cfg(toy, x, t, encoder_hidden_states, cfg_scale)

    z = torch.cat([torch.randn(1, 4, 3, 4, 4, generator=g)] * 2)
    xs = torch.cat([torch.randn(1, 4, 3, 4, 4, generator=g)] * 2)
    ctx = torch.randn(2, 7, 5, generator=g)
    kw = dict(clip_denoised=False, model_kwargs=dict(encoder_hidden_states=ctx, class_labels=None), mask=None, x_start=xs,
              use_concat=True, copy_no_mask=True)
    loop = rd.create_diffusion("10").ddim_sample_loop(fwd_cfg, z.shape, z, progress=False, device="cpu", **kw)
    out["interp_diffusion"] = dict(tables=tables, loop=sample(loop))

    # VSR stage: ResnetBlock3DCNN (vsr/models/resnet.py, direct import)
    mv = load_file("ref_vsr_resnet", "vsr/models/resnet.py")
    g = torch.Generator().manual_seed(4)
    cases = []
    for c, kern, frames in ((64, (5, 1, 1), 7), (128, (3, 1, 1), 2)):
        blk = mv.ResnetBlock3DCNN(in_channels=c, out_channels=c, kernel=kern, temb_channels=96).eval()
        shapes = module_shapes(blk)
        blk.load_state_dict(synth(shapes, 5))
        x, temb = torch.randn(2, c, frames, 4, 6, generator=g), torch.randn(2, 96, generator=g)
        cases.append(dict(shapes=shapes, y=sample(blk(x, temb))))
    out["vsr_resnet"] = cases

    # VSR Transformer3DModel and whole UNet3DVSRModel at a small width (vsr/models, under the shim)
    mb = refimport.load_vsr_blocks()
    cases = {}
    for only_cross in (True, False):
        tr = mb.attention.Transformer3DModel(8, 32, in_channels=256, num_layers=1, cross_attention_dim=128, norm_num_groups=32,
                                             use_linear_projection=True, only_cross_attention=only_cross,
                                             rotary_emb=RotaryEmbedding(32)).eval()
        shapes = module_shapes(tr)
        tr.load_state_dict(synth(shapes, 7))
        g = torch.Generator().manual_seed(2)
        x, ctx = torch.randn(2, 256, 5, 4, 4, generator=g), torch.randn(2, 77, 128, generator=g)
        cases[only_cross] = dict(shapes=shapes, y=sample(tr(x, encoder_hidden_states=ctx).sample))
    out["vsr_transformer3d"] = cases
    net = mb.unet.UNet3DVSRModel(
        sample_size=8, in_channels=7, out_channels=4, block_out_channels=(64, 128),
        down_block_types=("DownBlock3D", "CrossAttnDownBlock3D"), up_block_types=("CrossAttnUpBlock3D", "UpBlock3D"),
        only_cross_attention=(True, False), layers_per_block=1, cross_attention_dim=64, attention_head_dim=4,
        use_linear_projection=True, num_class_embeds=1000, down_temporal_idx=(0, 1), mid_temporal=True,
        up_temporal_idx=(0, 1), video_condition=False, temporal_module_config=refimport.VSR_TEMPORAL_MODULE_CONFIG).eval()
    shapes = module_shapes(net)
    net.load_state_dict(synth(shapes, 9))
    g = torch.Generator().manual_seed(1)
    x, lr = torch.randn(2, 4, 5, 8, 8, generator=g), torch.randn(2, 3, 5, 8, 8, generator=g)
    ctx, labels = torch.randn(2, 77, 64, generator=g), torch.tensor([20, 250])
    out["vsr_unet"] = dict(shapes=shapes, y=sample(net(x, torch.tensor(500), lr, encoder_hidden_states=ctx, class_labels=labels).sample))

    # FeedForward / GEGLU as the reference holds them (vsr/models/diffusers_attention.py)
    cases = {}
    for dim in (320, 640):
        ff = mb.diffusers_attention.FeedForward(dim, dropout=0.0, activation_fn="geglu").eval()
        shapes = module_shapes(ff)
        ff.load_state_dict(synth(shapes, 21))
        x = torch.randn(3, 50, dim, generator=torch.Generator().manual_seed(dim)) * 2.0
        cases[dim] = dict(shapes=shapes, y=sample(ff(x)))
    out["geglu_ff"] = cases

    # the sinusoidal timestep embedding the reference holds in-tree (base/models/utils.py)
    mu = load_file("ref_base_utils", "base/models/utils.py")
    t = torch.cat([torch.arange(980, -1, -20, dtype=torch.float32), torch.tensor([999.0, 0.5, 123.456, 1.0])])
    out["timestep_embedding"] = {dim: mu.timestep_embedding(t, dim) for dim in (320, 256)}

    save("oracle_pins_stages.pt", out)


if __name__ == "__main__":
    main()
