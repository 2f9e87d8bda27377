#!/usr/bin/env python3
"""The AutoencoderKL mid block's attention product (one head, head dim 512) on the engine kernel (csrc/attention_wide.hip)
against stock `F.scaled_dot_product_attention`, and what it does to a VAE decode.  Three parts, each a child process under
its own time limit; inside a part both arms run in ONE process in A B B A order and report medians of device events:
  product  the product alone on the same fp16 tensors (q | k | v slices of one fused tensor, q scaled by 4) at
           NB 1 x L 163,840 (VSR decode of one 320x512 latent frame), NB 4 x L 2,560 (base decode), NB 8 x L 2,560
           (interpolation-stage encode): us and TFLOP/s (4 NB L^2 dh);
  decode   `HipAutoencoderKL.decode` of one frame of 320x512 latents with the VSR VAE configuration
           (block_out_channels 128 / 256 / 512), attention="engine" and "sdpa";
  pmc      `rocprofv3 --pmc FETCH_SIZE` (no tracing beside it) around two launches of the engine kernel at the production
           shape, folded by tools/pmc_by_grid.py: bytes fetched per launch against the 0.34 GB of K + V.
Prints one JSON line and writes it to --out.  Usage: python tools/bench_vae_attention.py [--out profiles/vae_attention.json]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("vsr_decode", 1, 163840), ("base_decode", 4, 2560), ("interp_encode", 8, 2560)]
DH = 512


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


def fused(nb, l, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(nb * l, 3 * DH, generator=g, device="cuda")
    x[:, :DH] *= 4.0
    return x.to(torch.float16)


def arms(nb, l, d):
    import torch.nn.functional as F
    from lavie_amd import ops
    t = d.reshape(nb, l, 3, DH)
    engine = lambda: ops.attention(d[:, :DH], d[:, DH:2 * DH], d[:, 2 * DH:], nb, l, l, 1)                       # noqa: E731
    sdpa = lambda: F.scaled_dot_product_attention(t[:, None, :, 0], t[:, None, :, 1], t[:, None, :, 2])         # noqa: E731
    return engine, sdpa


def abba(a, b, iters):
    """-> (median of arm a, median of arm b, the four medians in run order)"""
    a(), b()
    runs = [timed(f, iters) for f in (a, b, b, a)]
    return (runs[0] + runs[3]) / 2, (runs[1] + runs[2]) / 2, runs


def part_product(iters):
    import torch
    res = {}
    for name, nb, l in SHAPES:
        d = fused(nb, l)
        engine, sdpa = arms(nb, l, d)
        rel = ((engine().float() - sdpa()[:, 0].reshape(nb * l, DH).float()).norm() / sdpa().float().norm()).item()
        it = iters if l < 100000 else max(3, iters // 3)
        e_ms, s_ms, runs = abba(engine, sdpa, it)
        flop = 4.0 * nb * l * l * DH
        res[name] = {"nb": nb, "l": l, "dh": DH, "engine_us": e_ms * 1e3, "sdpa_us": s_ms * 1e3,
                     "engine_tflops": flop / e_ms / 1e9, "sdpa_tflops": flop / s_ms / 1e9,
                     "abba_ms": runs, "engine_vs_sdpa_rel_l2": rel, "iters": it}
        del d
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    return res


def part_decode(iters):
    import torch
    from lavie_amd.autoencoder_kl import AutoencoderKL
    from lavie_amd.vae_hip import HipAutoencoderKL
    torch.manual_seed(0)
    vae = AutoencoderKL(block_out_channels=(128, 256, 512), scaling_factor=0.08333).cuda().half().eval()
    z = torch.randn(1, 4, 320, 512, device="cuda", dtype=torch.float16)
    eng, sd = HipAutoencoderKL(vae, attention="engine"), HipAutoencoderKL(vae, attention="sdpa")
    a, b = (lambda: eng.decode(z).sample), (lambda: sd.decode(z).sample)
    ya, yb = a().float(), b().float()
    rel = ((ya - yb).norm() / yb.norm()).item()
    del ya, yb
    e_ms, s_ms, runs = abba(a, b, iters)
    return {"latents": [1, 4, 320, 512], "block_out_channels": [128, 256, 512], "engine_ms": e_ms, "sdpa_ms": s_ms,
            "abba_ms": runs, "engine_vs_sdpa_rel_l2": rel, "iters": iters,
            "clip_61_frames_s": {"engine": 61 * e_ms / 1e3, "sdpa": 61 * s_ms / 1e3}}


def part_pmc_target():
    import torch
    name, nb, l = SHAPES[0]
    engine, _ = arms(nb, l, fused(nb, l))
    engine(), engine()
    torch.cuda.synchronize()


def child(part, limit, extra=()):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"part {part} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().split("\n")[-1])


def run_pmc(limit, outdir):
    shutil.rmtree(outdir, ignore_errors=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--pmc", "FETCH_SIZE", "-d", outdir, "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--part", "pmc-target"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": f"rocprofv3 exited {r.returncode}", "stderr": r.stderr[-800:]}
    t = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_by_grid.py"), outdir, "attention_wide"],
                       capture_output=True, text=True).stdout
    m = re.search(r"attention_wide_kernel\S*\s+(\d+)\s+(\d+)\s+([\d.]+)\s+(\S+)", t)
    if not m:
        return {"error": "kernel not found in the counter output", "table": t[-800:]}
    read_gb = float(m.group(3)) / 1e3
    operands_gb = 2 * 163840 * DH * 2 / 1e9
    return {"grid": int(m.group(1)), "launches": int(m.group(2)), "fetch_gb_per_launch": read_gb, "kv_operand_gb": operands_gb,
            "fetch_over_kv": read_gb / operands_gb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["all", "product", "decode", "pmc-target"])
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--pmc-dir", default="", help="where rocprofv3 writes its counters (default: a temporary directory)")
    ap.add_argument("--no-pmc", action="store_true")
    a = ap.parse_args()
    if a.part == "product":
        print(json.dumps(part_product(a.iters)))
        return
    if a.part == "decode":
        print(json.dumps(part_decode(max(3, a.iters // 3))))
        return
    if a.part == "pmc-target":
        part_pmc_target()
        return
    res = {"metric": "vae_attention", "product": child("product", 240, ["--iters", str(a.iters)]),
           "decode_one_frame": child("decode", 240, ["--iters", str(a.iters)])}
    if not a.no_pmc:
        res["pmc"] = run_pmc(180, a.pmc_dir or tempfile.mkdtemp(prefix="pmc_vae_attention_"))
    p = res["product"]["vsr_decode"]
    res["default"] = "engine" if p["engine_us"] <= p["sdpa_us"] else "sdpa"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
