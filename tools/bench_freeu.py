"""What FreeU costs, measured in one process in the order A B B A:
  * the forward with FreeU off and on, base model at [2, 4, 16, 40 x 64] and VSR model at the chunk [2, ., 8, 320 x 512];
  * lavie_freeu_f16 alone at the four production shapes against the same thing composed from torch ops the way diffusers does it
    (permute to NCHW, torch.fft, permute back; the half-channel scale in place).
Writes profiles/freeu.json.  Weights are random: only times are read.   python tools/bench_freeu.py [--out profiles/freeu.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from lavie_amd import ops  # noqa: E402

FREEU = (0.9, 0.2, 1.2, 1.4)          # s1, s2, b1, b2: diffusers' suggestion for SD-1.4-sized UNets


def timeit(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def abba(a, b, n):
    """ms of a and b, each the mean of its two turns in the order a b b a"""
    for _ in range(2):
        a()
        b()
    ta1, tb1, tb2, ta2 = timeit(a, n), timeit(b, n), timeit(b, n), timeit(a, n)
    return dict(a_ms=[ta1, ta2], b_ms=[tb1, tb2], a_mean_ms=(ta1 + ta2) / 2, b_mean_ms=(tb1 + tb2) / 2)


def randomise(net):
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.ones_like(p) if name.endswith("weight") else torch.zeros_like(p))
            else:
                p.copy_((torch.randn(p.shape, generator=g, device="cuda") / p[0].numel() ** 0.5).to(p.dtype))
    net.refresh_engine()
    return net


def forward_cost(net, call, n):
    def off():
        net.disable_freeu()
        call()

    def on():
        net.enable_freeu(*FREEU)
        call()
    r = abba(off, on, n)
    net.disable_freeu()
    return dict(off_ms=r["a_mean_ms"], on_ms=r["b_mean_ms"], off_turns_ms=r["a_ms"], on_turns_ms=r["b_ms"],
                delta_ms=r["b_mean_ms"] - r["a_mean_ms"], delta_percent=100.0 * (r["b_mean_ms"] - r["a_mean_ms"]) / r["a_mean_ms"])


def torch_freeu(h, skip, ni, H, W, b, s):
    """diffusers' apply_freeu on the same row matrices: NCHW round trip, fp32 FFT, back to fp16 rows"""
    h = h.clone()
    h[:, :h.shape[1] // 2] *= b
    x = skip.reshape(ni, H, W, -1).permute(0, 3, 1, 2).float()
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones_like(X.real)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    x = torch.fft.ifftn(torch.fft.ifftshift(X * mask, dim=(-2, -1)), dim=(-2, -1)).real
    return h, x.to(skip.dtype).permute(0, 2, 3, 1).reshape(skip.shape).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/freeu.json")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-vsr", action="store_true")
    a = ap.parse_args()
    res = dict(freeu=dict(zip(("s1", "s2", "b1", "b2"), FREEU)), device=torch.cuda.get_device_name(0), order="A B B A, one process",
               forward={}, operator={})
    g = torch.Generator().manual_seed(0)

    ops_shapes = [("base 32 x 5x8 x 1280/1280", 32, 5, 8, 1280, 1280), ("base 32 x 10x16 x 1280/640", 32, 10, 16, 1280, 640),
                  ("vsr 16 x 40x64 x 1024/1024", 16, 40, 64, 1024, 1024), ("vsr 16 x 80x128 x 512/512", 16, 80, 128, 512, 512)]
    for name, ni, H, W, ch, c2 in ops_shapes:
        h = torch.randn(ni * H * W, ch, generator=g).half().cuda()
        skip = torch.randn(ni * H * W, c2, generator=g).half().cuda()
        ho, so = torch.empty_like(h), torch.empty_like(skip)
        r = abba(lambda: ops.freeu(h, skip, ni, H, W, 1.2, 0.9, out=(ho, so)), lambda: torch_freeu(h, skip, ni, H, W, 1.2, 0.9), 50)
        inpl = timeit(lambda: ops.freeu(h, skip, ni, H, W, 1.2, 0.9, out=(h, skip)), 50)
        res["operator"][name] = dict(kernel_us=1e3 * r["a_mean_ms"], kernel_in_place_us=1e3 * inpl, torch_us=1e3 * r["b_mean_ms"],
                                     kernel_turns_us=[1e3 * v for v in r["a_ms"]], torch_turns_us=[1e3 * v for v in r["b_ms"]])
        print(name, res["operator"][name], flush=True)

    from lavie_amd.unet import UNet3DConditionModel
    net = randomise(UNet3DConditionModel(init_weights=False, sample_size=64, cross_attention_dim=768).to("cuda", torch.float16))
    x = torch.randn(2, 4, 16, 40, 64, generator=g).half().cuda()
    ctx = torch.randn(2, 77, 768, generator=g).half().cuda()
    res["forward"]["base [2,4,16,40x64]"] = forward_cost(net, lambda: net(x, 500, encoder_hidden_states=ctx), a.steps)
    print("base", res["forward"]["base [2,4,16,40x64]"], flush=True)
    del net
    if not a.skip_vsr:
        from lavie_amd.vsr import UNet3DVSRModel
        vsr = randomise(UNet3DVSRModel(init_weights=False, sample_size=128, down_temporal_idx=(0, 1, 2, 3), mid_temporal=True,
                                       up_temporal_idx=(0, 1, 2, 3)).to("cuda", torch.float16))
        xv, low = torch.randn(2, 4, 8, 320, 512, generator=g).half().cuda(), torch.randn(2, 3, 8, 320, 512, generator=g).half().cuda()
        cv = torch.randn(2, 77, 1024, generator=g).half().cuda()
        labels = torch.tensor([150, 150])
        res["forward"]["vsr chunk [2,.,8,320x512]"] = forward_cost(
            vsr, lambda: vsr(xv, 500, low, encoder_hidden_states=cv, class_labels=labels), max(2, a.steps // 3))
        print("vsr", res["forward"]["vsr chunk [2,.,8,320x512]"], flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
