"""Test-side references of the layer cache (DeepCache).  TEST INFRASTRUCTURE: nothing under lavie_amd/ imports it.

`full` restates oracle.unet_fp32.unet_forward out of the oracle's own block functions, step for step, and hands back the running
activation at cut B besides the output; `shallow` is the walk a reuse forward takes: the time embedding, conv_in, `depth` layers of down
level 0, then, on a given activation at B, the last `depth` + 1 layers of the last up block with the skips of THIS call in the order
the full walk pops them, conv_norm_out and conv_out.  tests/test_layercache_host.py holds `full` to the oracle bit for bit and
checks that the cases separate a right shallow output from a stale, wrong-cut or ignored cache.

Cuts for a depth d in 1..layers_per_block: A behind layer d - 1 of down level 0; B in front of layer layers_per_block - d of the last
up block (behind the upsampler into level 0)."""
import torch
import torch.nn.functional as F

import pagcases as P

WIDTHS, ATTN, BASE_KW, SEED = P.WIDTHS, P.ATTN, P.BASE_KW, P.SEED      # the reduced base structure of tests/pagcases.py
DEPTHS = (1, 2)
# B, F, h, w: the smallest shapes that still give more than one tile per workgroup at level 0, and an odd frame count
SHAPES = {"F4-16x16": (2, 4, 16, 16), "F3-24x40": (2, 3, 24, 40)}
T_OLD, T_NEW = 500, 321                                                # the refresh step's timestep, the reuse step's


def ocfg():
    return P.ocfg()


def base_weights():
    return P.base_weights()


def inputs(name):
    """(x_old, x_new, ctx): the latents of the refresh step, fresh latents for the reuse step, one context for both.  The two batch
    entries hold the same latents ([negative | prompt], as a guided loop feeds them: the shared CFG prefix applies)."""
    b, f, h, w = SHAPES[name]
    g = torch.Generator().manual_seed(4100 + f)
    old = torch.randn(1, 4, f, h, w, generator=g).half()
    new = torch.randn(1, 4, f, h, w, generator=g).half()
    ctx = torch.randn(b, 77, 128, generator=g).half()
    return torch.cat([old] * b).contiguous(), torch.cat([new] * b).contiguous(), ctx


def _front(sd, sample, timesteps, ctx, cfg, layers):
    """The time embedding, conv_in and the first `layers` layers of down level 0: (emb, x, skips)."""
    from oracle import unet_fp32 as O
    sample = sample.float()
    t = torch.as_tensor(timesteps).reshape(-1).expand(sample.shape[0])
    emb = O.time_embedding(sd, t, cfg)
    x = O.conv_frames(sample, sd["conv_in.weight"], sd["conv_in.bias"])
    skips = [x]
    for j in range(layers):
        x = O.resnet_block(sd, f"down_blocks.0.resnets.{j}.", x, emb, cfg)
        if cfg.attn_levels[0]:
            x = O.transformer3d(sd, f"down_blocks.0.attentions.{j}.", x, ctx, cfg)
        skips.append(x)
    return emb, x, skips


def _up_layer(sd, i, j, lvl, x, skips, emb, ctx, cfg):
    from oracle import unet_fp32 as O
    x = torch.cat([x, skips.pop()], dim=1)
    x = O.resnet_block(sd, f"up_blocks.{i}.resnets.{j}.", x, emb, cfg)
    if cfg.attn_levels[lvl]:
        x = O.transformer3d(sd, f"up_blocks.{i}.attentions.{j}.", x, ctx, cfg)
    return x


def _end(sd, x, cfg):
    from oracle import unet_fp32 as O
    x = F.silu(O.group_norm_video(x, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], cfg.norm_groups, cfg.norm_eps))
    return O.conv_frames(x, sd["conv_out.weight"], sd["conv_out.bias"])


def full(sd, x, t, ctx, cfg, depth):
    """(out, feature at B) of the whole forward; `out` is O.unet_forward's, operation for operation."""
    from oracle import unet_fp32 as O
    nlev, lpb = len(cfg.block_out_channels), cfg.layers_per_block
    assert 1 <= depth <= lpb and nlev >= 3
    ctx = ctx.float()
    emb, x, skips = _front(sd, x, t, ctx, cfg, lpb)
    for lvl in range(nlev):
        if lvl > 0:
            for j in range(lpb):
                x = O.resnet_block(sd, f"down_blocks.{lvl}.resnets.{j}.", x, emb, cfg)
                if cfg.attn_levels[lvl]:
                    x = O.transformer3d(sd, f"down_blocks.{lvl}.attentions.{j}.", x, ctx, cfg)
                skips.append(x)
        if lvl != nlev - 1:
            x = O.downsample(sd, f"down_blocks.{lvl}.downsamplers.0.", x)
            skips.append(x)
    x = O.resnet_block(sd, "mid_block.resnets.0.", x, emb, cfg)
    x = O.transformer3d(sd, "mid_block.attentions.0.", x, ctx, cfg)
    x = O.resnet_block(sd, "mid_block.resnets.1.", x, emb, cfg)
    feature = None
    for i in range(nlev):
        lvl = nlev - 1 - i
        for j in range(lpb + 1):
            if i == nlev - 1 and j == lpb - depth:
                feature = x                                            # cut B
            x = _up_layer(sd, i, j, lvl, x, skips, emb, ctx, cfg)
        if i != nlev - 1:
            x = O.upsample(sd, f"up_blocks.{i}.upsamplers.0.", x)
    return _end(sd, x, cfg), feature


def shallow(sd, x, t, ctx, cfg, depth, feature):
    """The output of the shallow walk at (x, t) on `feature`, the activation at B of some earlier full walk."""
    nlev, lpb = len(cfg.block_out_channels), cfg.layers_per_block
    assert 1 <= depth <= lpb and nlev >= 3
    ctx = ctx.float()
    emb, _, skips = _front(sd, x, t, ctx, cfg, depth)                  # depth + 1 skips: conv_in's and one per layer
    x = feature
    for j in range(lpb - depth, lpb + 1):
        x = _up_layer(sd, nlev - 1, j, 0, x, skips, emb, ctx, cfg)
    assert not skips
    return _end(sd, x, cfg)


_REFS = {}


def _sd():
    return _REFS.setdefault("sd", {k: v.float() for k, v in base_weights().items()})


def refs(name, depth):
    """The references of one case, computed once per process and left unchanged: dict(full_old, shallow) with
    full_old = full(x_old, T_OLD)[0] and shallow = shallow(x_new, T_NEW, feature at B of that walk)."""
    key = (name, depth)
    if key not in _REFS:
        x_old, x_new, ctx = inputs(name)
        out_old, feature = full(_sd(), x_old.float(), T_OLD, ctx.float(), ocfg(), depth)
        _REFS[key] = dict(full_old=out_old, shallow=shallow(_sd(), x_new.float(), T_NEW, ctx.float(), ocfg(), depth, feature))
    return _REFS[key]


def full_new(name):
    """full(x_new, T_NEW)[0]: what a forward that ignores the cache gives at the reuse step's input (once per process)."""
    if ("new", name) not in _REFS:
        _, x_new, ctx = inputs(name)
        _REFS["new", name] = full(_sd(), x_new.float(), T_NEW, ctx.float(), ocfg(), 1)[0]
    return _REFS["new", name]


def schedule(steps, interval):
    """The modes of `steps` executed steps at `cache_interval` = interval, restated: step k refreshes iff k % interval == 0."""
    if interval is None or interval <= 1:
        return [None] * steps
    return ["refresh" if k % interval == 0 else "reuse" for k in range(steps)]
