"""What perturbed-attention guidance costs, measured in one process in the order A B B A:
  * the base forward at [3, 4, 16, 40 x 64] with PAG on `mid_block` (one perturbed entry) against the same build's [2, 4, 16, 40 x 64]
    forward without it: the price of the third batch entry;
  * the fused PAG step (lavie_cfg_pag_sampler_step) at [1, 4, 16, 40 x 64] against the plain guided step (lavie_cfg_sampler_step) and
    against the same arithmetic composed from torch ops.
Writes profiles/pag.json.  Weights are random: only times are read.   python tools/bench_pag.py [--out profiles/pag.json]"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
from lavie_amd import ops  # noqa: E402

COEFFS = (1.0125, 0.1594, 0.0123, 0.9841, 0.0107)
GUIDANCE, PAG_SCALE = 7.5, 3.0


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


def torch_step(eps3, x, noise, model_in3):
    """the PAG step's arithmetic from torch ops, fp32, with the same outputs"""
    k_x, k_e, c_x0, c_xt, sigma = COEFFS
    eu, ec, ep = eps3.float().unbind(0)
    e = eu + GUIDANCE * (ec - eu) + PAG_SCALE * (ec - ep)
    x0 = k_x * x - k_e * e
    xn = c_x0 * x0 + c_xt * x + sigma * noise
    x.copy_(xn)
    model_in3.copy_(xn.half().expand_as(model_in3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pag.json")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), order="A B B A, one process", guidance=GUIDANCE, pag_scale=PAG_SCALE, forward={}, step={})
    g = torch.Generator().manual_seed(0)

    shape = (1, 4, 16, 40, 64)
    n = 4 * 16 * 40 * 64
    eps3 = torch.randn(3, n, generator=g).half().cuda()
    x, noise = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    m3, m2 = torch.empty(3, n, dtype=torch.float16, device="cuda"), torch.empty(2, n, dtype=torch.float16, device="cuda")
    eps2 = eps3[:2].contiguous()
    pag = lambda: ops.cfg_pag_sampler_step(eps3, x, noise, m3, GUIDANCE, PAG_SCALE, COEFFS, 1.0)
    plain = lambda: ops.cfg_ddpm_step(eps2, x, noise, m2, GUIDANCE, COEFFS, 1.0)
    xt = x.reshape(-1).clone()
    composed = lambda: torch_step(eps3, xt, noise.reshape(-1), m3)
    r1, r2 = abba(plain, pag, 200), abba(composed, pag, 200)
    res["step"]["[1,4,16,40x64]"] = dict(plain_guided_us=1e3 * r1["a_mean_ms"], pag_us=1e3 * r1["b_mean_ms"],
                                         plain_turns_us=[1e3 * v for v in r1["a_ms"]], pag_turns_us=[1e3 * v for v in r1["b_ms"]],
                                         torch_composed_us=1e3 * r2["a_mean_ms"], pag_beside_torch_us=1e3 * r2["b_mean_ms"],
                                         torch_turns_us=[1e3 * v for v in r2["a_ms"]])
    print("step", res["step"], flush=True)

    from lavie_amd.unet import UNet3DConditionModel
    net = randomise(UNet3DConditionModel(init_weights=False, sample_size=64, cross_attention_dim=768).to("cuda", torch.float16))
    x3 = torch.randn(1, 4, 16, 40, 64, generator=g).half().cuda().repeat(3, 1, 1, 1, 1).contiguous()
    c3 = torch.randn(3, 77, 768, generator=g).half().cuda()
    x2, c2 = x3[:2].contiguous(), c3[:2].contiguous()

    def off():
        net.disable_pag()
        net(x2, 500, encoder_hidden_states=c2)

    def on():
        net.set_pag(("mid_block",), 1)
        net(x3, 500, encoder_hidden_states=c3)

    def three():
        net.disable_pag()
        net(x3, 500, encoder_hidden_states=c3)
    r = abba(off, on, a.steps)
    r3 = abba(three, on, a.steps)
    net.disable_pag()
    res["forward"]["base, PAG on mid_block"] = dict(
        b2_off_ms=r["a_mean_ms"], b3_on_ms=r["b_mean_ms"], b2_off_turns_ms=r["a_ms"], b3_on_turns_ms=r["b_ms"],
        ratio_b3_on_to_b2_off=r["b_mean_ms"] / r["a_mean_ms"], b3_off_ms=r3["a_mean_ms"], b3_on_beside_b3_off_ms=r3["b_mean_ms"],
        b3_off_turns_ms=r3["a_ms"])
    print("forward", res["forward"], flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
