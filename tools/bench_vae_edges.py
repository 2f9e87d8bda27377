#!/usr/bin/env python3
"""The AutoencoderKL edge convolutions and stride-2 downsamplers on the engine (csrc/conv_edge.hip, lavie_conv3x3_down_f16)
against the stock `torch.nn.Conv2d` path they replace (MIOpen, with the layout copies and casts that path needs), and what the
switch does to a VAE decode and encode.  Three parts, each a child process under its own time limit; inside a part both arms run
in ONE process in A B B A order and report medians of device events:
  launches  each new launch in isolation at its production shape: conv_edge_out 128 -> 3 at 1 x 1280 x 2048 writing fp32 (the last
            convolution of the VSR decode; stock arm = permuted fp32 copy + Conv2d), conv_edge_in 4 -> 512 at 320 x 512 with
            post_quant_conv folded in (stock arm = the two Conv2d + cast + rows copy), and the three downsamplers of an 8-frame
            encode at 320 x 512 pixels (stock arm = rows -> NCHW -> F.pad + Conv2d -> rows);
  decode    `HipAutoencoderKL.decode` of one frame of 320 x 512 latents, VSR layout (128 / 256 / 512, fp32 weights), edges="engine"
            and "stock";
  encode    `HipAutoencoderKL.encode` of 16 frames of 320 x 512 pixels (fp16 weights, two calls of 8 as the cascade makes them).
  first     the FIRST decode / encode call at the production shape, each arm in a child process of its own (host clock around a
            synchronised call, after that arm ran once at a small shape so that code-object loading and weight packing are out of
            it): what is left is per-shape first-use cost, MIOpen's kernel search above all; the second call in the same child is
            reported beside it.
Prints one JSON line and writes it to --out.  Usage: python tools/bench_vae_edges.py [--out profiles/vae_edges.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out)


def abba(a, b, iters):
    """-> (median of arm a, median of arm b, the four medians in run order)"""
    a(), b()
    runs = [timed(f, iters) for f in (a, b, b, a)]
    return (runs[0] + runs[3]) / 2, (runs[1] + runs[2]) / 2, runs


def first_call(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def part_launches(iters):
    import torch
    import torch.nn.functional as F
    from lavie_amd import ops
    from lavie_amd.vae_hip import _rows, fold_post_quant_conv
    res = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")                                                       # noqa: E731

    # conv_edge_out: 128 -> 3 at 1 x 1280 x 2048, fp32 out
    n, h, w, c = 1, 1280, 2048, 128
    conv = torch.nn.Conv2d(c, 3, 3, padding=1).cuda().eval()
    x = rnd(n * h * w, c).half()
    wp, b = ops.pack_conv_edge_out(conv.weight.detach().half()), conv.bias.detach().float()
    eng = lambda: ops.conv_edge_out(x, wp, b, n, h, w, 3, torch.float32)                                                # noqa: E731
    with torch.no_grad():
        stk = lambda: conv(x.reshape(n, h, w, c).permute(0, 3, 1, 2).to(torch.float32))                                # noqa: E731
        stk_conv_only_in = x.reshape(n, h, w, c).permute(0, 3, 1, 2).to(torch.float32)
        r = rel(eng(), stk())
        e_ms, s_ms, runs = abba(eng, stk, iters)
        conv_only = timed(lambda: conv(stk_conv_only_in), iters)
    gb = (n * h * w * (2.0 * c + 4.0 * 3)) / 1e9
    res["conv_edge_out_128to3_1280x2048_f32"] = {"engine_ms": e_ms, "stock_ms": s_ms, "abba_ms": runs, "stock_conv_alone_ms": conv_only,
                                                 "engine_gb_per_s": gb / e_ms * 1e3, "engine_vs_stock_rel_l2": r, "iters": iters}
    del x, stk_conv_only_in, conv
    torch.cuda.empty_cache()

    # conv_edge_in: post_quant_conv (4 -> 4) + conv_in (4 -> 512) at 320 x 512, fp32 latent
    n, h, w, c = 1, 320, 512, 512
    pq, cin = torch.nn.Conv2d(4, 4, 1).cuda().eval(), torch.nn.Conv2d(4, c, 3, padding=1).cuda().eval()
    z = rnd(n, 4, h, w)
    wf, tap = fold_post_quant_conv(cin.weight.detach(), pq.weight.detach(), pq.bias.detach())
    wp, b = ops.pack_conv_edge_in(wf.half()), cin.bias.detach().float()
    eng = lambda: ops.conv_edge_in(z, wp, b, c, tap_bias=tap)                                                           # noqa: E731
    with torch.no_grad():
        stk = lambda: _rows(cin(pq(z)).to(torch.float16))                                                               # noqa: E731
        r = rel(eng(), stk())
        e_ms, s_ms, runs = abba(eng, stk, iters)
    res["conv_edge_in_4to512_320x512"] = {"engine_ms": e_ms, "stock_ms": s_ms, "abba_ms": runs, "engine_vs_stock_rel_l2": r, "iters": iters}
    del z
    torch.cuda.empty_cache()

    # the three downsamplers of an 8-frame encode at 320 x 512 pixels (fp16 weights)
    n = 8
    for c, h, w in ((128, 320, 512), (256, 160, 256), (512, 80, 128)):
        conv = torch.nn.Conv2d(c, c, 3, stride=2).cuda().half().eval()
        x = rnd(n * h * w, c).half()
        wp, b = ops.pack_conv3x3(conv.weight.detach()), conv.bias.detach().float()
        eng = lambda: ops.conv3x3(x, wp, b, n, h, w, stride=2, pad=(0, 1))                                              # noqa: E731
        with torch.no_grad():
            stk = lambda: _rows(conv(F.pad(x.reshape(n, h, w, c).permute(0, 3, 1, 2).to(torch.float16), (0, 1, 0, 1))).to(torch.float16))  # noqa: E731
            r = rel(eng(), stk())
            e_ms, s_ms, runs = abba(eng, stk, iters)
        res[f"downsampler_{c}_{n}x{h}x{w}"] = {"engine_ms": e_ms, "stock_ms": s_ms, "abba_ms": runs, "engine_vs_stock_rel_l2": r,
                                               "engine_tflops": 2.0 * n * (h // 2) * (w // 2) * c * 9 * c / e_ms / 1e9, "iters": iters}
        del x, conv
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    return res


def _two_arms(vae):
    from lavie_amd.vae_hip import HipAutoencoderKL
    return HipAutoencoderKL(vae, edges="engine"), HipAutoencoderKL(vae, edges="stock")


def part_decode(iters):
    import torch
    from lavie_amd.autoencoder_kl import AutoencoderKL
    torch.manual_seed(0)
    vae = AutoencoderKL(block_out_channels=(128, 256, 512), scaling_factor=0.08333).cuda().eval()          # fp32, as the VSR stage's
    eng, stk = _two_arms(vae)
    small = torch.randn(1, 4, 16, 16, device="cuda")
    eng.decode(small), stk.decode(small)
    z = torch.randn(1, 4, 320, 512, device="cuda")
    a, b = (lambda: eng.decode(z).sample), (lambda: stk.decode(z).sample)
    r = rel(a(), b())
    e_ms, s_ms, runs = abba(a, b, iters)
    return {"latents": [1, 4, 320, 512], "block_out_channels": [128, 256, 512], "weights": "fp32",
            "engine_ms": e_ms, "stock_ms": s_ms, "abba_ms": runs, "engine_vs_stock_rel_l2": r, "iters": iters,
            "clip_61_frames_s": {"engine": 61 * e_ms / 1e3, "stock": 61 * s_ms / 1e3}}


def part_encode(iters):
    import torch
    from lavie_amd.autoencoder_kl import AutoencoderKL
    torch.manual_seed(0)
    vae = AutoencoderKL().cuda().half().eval()
    eng, stk = _two_arms(vae)
    small = torch.rand(1, 3, 64, 64, device="cuda", dtype=torch.float16)
    eng.encode(small), stk.encode(small)
    x = torch.rand(16, 3, 320, 512, device="cuda", dtype=torch.float16) * 2 - 1
    enc = lambda m: torch.cat([m.encode(x[i:i + 8]).latent_dist.mean for i in (0, 8)])                                  # noqa: E731
    a, b = (lambda: enc(eng)), (lambda: enc(stk))
    r = rel(a(), b())
    e_ms, s_ms, runs = abba(a, b, iters)
    return {"pixels": [16, 3, 320, 512], "block_out_channels": [128, 256, 512, 512], "weights": "fp16", "calls": "2 x 8 frames",
            "engine_ms": e_ms, "stock_ms": s_ms, "abba_ms": runs, "engine_vs_stock_rel_l2_mean": r, "iters": iters}


def part_first(what, arm):
    """one arm alone in this process: small-shape call, then the first and the second call at the production shape (host ms)"""
    import torch
    from lavie_amd.autoencoder_kl import AutoencoderKL
    from lavie_amd.vae_hip import HipAutoencoderKL
    torch.manual_seed(0)
    if what == "decode":
        m = HipAutoencoderKL(AutoencoderKL(block_out_channels=(128, 256, 512), scaling_factor=0.08333).cuda().eval(), edges=arm)
        m.decode(torch.randn(1, 4, 16, 16, device="cuda"))
        z = torch.randn(1, 4, 320, 512, device="cuda")
        fn = lambda: m.decode(z).sample                                                                                # noqa: E731
    else:
        m = HipAutoencoderKL(AutoencoderKL().cuda().half().eval(), edges=arm)
        m.encode(torch.rand(1, 3, 64, 64, device="cuda", dtype=torch.float16))
        x = torch.rand(16, 3, 320, 512, device="cuda", dtype=torch.float16) * 2 - 1
        fn = lambda: [m.encode(x[i:i + 8]).latent_dist.mean for i in (0, 8)]                                            # noqa: E731
    return {"first_ms": first_call(fn), "second_ms": first_call(fn)}


def child(part, limit, extra=()):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"part {part} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "launches", "decode", "encode", "first"])
    ap.add_argument("--what", default="decode", choices=["decode", "encode"])
    ap.add_argument("--arm", default="engine", choices=["engine", "stock"])
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.part == "launches":
        print(json.dumps(part_launches(a.iters)))
        return
    if a.part == "decode":
        print(json.dumps(part_decode(max(3, a.iters // 3))))
        return
    if a.part == "encode":
        print(json.dumps(part_encode(max(3, a.iters // 3))))
        return
    if a.part == "first":
        print(json.dumps(part_first(a.what, a.arm)))
        return
    it = ["--iters", str(a.iters)]
    res = {"metric": "vae_edges", "launches": child("launches", 240, it), "decode_one_frame": child("decode", 240, it),
           "encode_16_frames": child("encode", 240, it)}
    res["first_call"] = {what: {arm: child("first", 200, ["--what", what, "--arm", arm]) for arm in ("engine", "stock")}
                         for what in ("decode", "encode")}
    at_or_below = [v["engine_ms"] <= v["stock_ms"] for k, v in res["launches"].items() if isinstance(v, dict)]
    at_or_below += [res["decode_one_frame"]["engine_ms"] <= res["decode_one_frame"]["stock_ms"],
                    res["encode_16_frames"]["engine_ms"] <= res["encode_16_frames"]["stock_ms"]]
    res["default"] = "engine" if all(at_or_below) else "stock"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
