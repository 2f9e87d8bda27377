"""-m gpu: the 3-D convolution kernels of the FVD evaluator per element -- guarded operands, poisoned outputs, the
gemm_c(K) bound of the 2-D conv tests against float64 F.conv3d on the fp16-rounded operands -- for every geometry R3D-18 uses, at
shapes that cross a 64-row workgroup tile and end off it; mean_rows against a float64 mean; bit properties; refusals."""
import math

import pytest
import torch
import torch.nn.functional as F

import opcheck as oc

pytestmark = pytest.mark.gpu


def sync():
    torch.cuda.synchronize()


def loc_rows5(t, h, w, c):
    def loc(i):
        p, ch = divmod(i, c)
        n, p = divmod(p, t * h * w)
        return "(clip %d, t %d, y %d, x %d, channel %d)" % (n, p // (h * w), p // w % h, p % w, ch)
    return loc


def conv_operands(n, t, h, w, cin, cout, ksize, stride, residual, seed):
    g = torch.Generator().manual_seed(seed)
    k = ksize ** 3 * cin
    out_shape = (n,) + tuple((e - 1) // stride + 1 for e in (t, h, w)) + (cout,)
    ins = {"x": torch.randn(n, t, h, w, cin, generator=g).half(),
           "w": (torch.randn(cout, cin, ksize, ksize, ksize, generator=g) / math.sqrt(k)).half(),
           "bias": torch.randn(cout, generator=g) * 0.5}
    if residual:
        ins["res"] = torch.randn(out_shape, generator=g).half()
    return ins, out_shape


def conv_reference(ins, ksize, stride, relu):
    """float64 conv3d on the fp16 values, channels-last like the kernel's output, and the sum of the magnitudes added per element"""
    x = ins["x"].double().permute(0, 4, 1, 2, 3)
    w, b = ins["w"].double(), ins["bias"].double().view(1, -1, 1, 1, 1)
    pad = 1 if ksize == 3 else 0
    ref = F.conv3d(x, w, stride=stride, padding=pad) + b
    scale = F.conv3d(x.abs(), w.abs(), stride=stride, padding=pad) + b.abs()
    ref, scale = ref.permute(0, 2, 3, 4, 1), scale.permute(0, 2, 3, 4, 1)
    if "res" in ins:
        ref, scale = ref + ins["res"].double(), scale + ins["res"].double().abs()
    return (ref.clamp_min(0) if relu else ref), scale          # ReLU is 1-Lipschitz: the bound of the sum holds behind it


def run_conv(ins, out_shape, ksize, stride, relu):
    from lavie_amd import ops

    def fn(i, o):
        ops.conv3d(i["x"], ops.pack_conv3d(i["w"]), i["bias"], ksize=ksize, stride=stride, residual=i.get("res"), relu=relu, out=o["y"])
    return oc.run_guarded(fn, ins, {"y": (out_shape, torch.float16)}, sync=sync)["y"]


# (label, cin, cout, ksize, stride, residual, relu, [(T, H, W)])
CONV_CASES = [
    ("1: 64->64 s1", 64, 64, 3, 1, False, True, [(4, 12, 20), (1, 5, 7), (2, 3, 3)]),
    ("2: 64->128 s2", 64, 128, 3, 2, False, True, [(5, 9, 11), (4, 12, 20)]),
    ("3: 128->128 s1 +res", 128, 128, 3, 1, True, True, [(3, 6, 10)]),
    ("4: 256->512 s2", 256, 512, 3, 2, False, True, [(2, 4, 6)]),
    ("5: 64->128 1x1x1 s2", 64, 128, 1, 2, False, False, [(5, 9, 11)]),
]
CONV_PARAMS = [pytest.param(*c[:7], thw, id=f"{c[0]} {thw}") for c in CONV_CASES for thw in c[7]]


@pytest.mark.parametrize("label,cin,cout,ksize,stride,residual,relu,thw", CONV_PARAMS)
def test_conv3d_per_element(label, cin, cout, ksize, stride, residual, relu, thw):
    t, h, w = thw
    ins, out_shape = conv_operands(2, t, h, w, cin, cout, ksize, stride, residual, seed=cin + cout + t)
    got = run_conv(ins, out_shape, ksize, stride, relu)
    ref, scale = conv_reference(ins, ksize, stride, relu)
    oc.assert_elementwise(got, ref, scale, oc.gemm_c(ksize ** 3 * cin + 2), where=loc_rows5(*out_shape[1:]), label=f"conv3d {label} {thw}")
    if relu:
        assert float(got.min()) == 0.0 and float(got.max()) > 0.0


def stem_operands(n, t, h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(n, 3, t, h, w, generator=g).to(dtype)
    return {"px": px, "w": (torch.randn(64, 3, 3, 7, 7, generator=g) / 21.0).half(), "bias": torch.randn(64, generator=g) * 0.5}


def stem_reference(ins):
    x = ins["px"].half().double()                    # fp32 pixels are rounded to fp16 on the way into the product
    w, b = ins["w"].double(), ins["bias"].double().view(1, -1, 1, 1, 1)
    kw = dict(stride=(1, 2, 2), padding=(1, 3, 3))
    ref = (F.conv3d(x, w, **kw) + b).clamp_min(0)
    return ref.permute(0, 2, 3, 4, 1), (F.conv3d(x.abs(), w.abs(), **kw) + b.abs()).permute(0, 2, 3, 4, 1)


def run_stem(ins, layout="ncthw"):
    from lavie_amd import ops
    n, _, t, h, w = ins["px"].shape
    out_shape = (n, t, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64)
    feed = dict(ins)
    if layout == "ntchw":
        feed["px"] = ins["px"].permute(0, 2, 1, 3, 4).contiguous()

    def fn(i, o):
        ops.conv3d_stem(i["px"], ops.pack_conv3d(i["w"]), i["bias"], relu=True, layout=layout, out=o["y"])
    return oc.run_guarded(fn, feed, {"y": (out_shape, torch.float16)}, sync=sync)["y"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("thw", [(5, 18, 22), (1, 7, 9)])
def test_stem_per_element(thw, dtype):
    ins = stem_operands(2, *thw, dtype, seed=thw[1])
    got = run_stem(ins)
    ref, scale = stem_reference(ins)
    oc.assert_elementwise(got, ref, scale, oc.gemm_c(441 + 1), where=loc_rows5(*got.shape[1:]), label=f"stem {thw} {dtype}")
    oc.assert_bits(run_stem(ins, layout="ntchw"), got, label="stem: frames-major pixels give the bits of channels-first pixels")


@pytest.mark.parametrize("rows", [1, 392, 1000])
def test_mean_rows_per_element(rows):
    """four sequential fp32 partials of ceil(rows / 4) terms, two more additions, one division: (ceil(rows / 4) + 3) roundings of
    2^-24 against the sum of magnitudes, and the final rounding of the fp32 result"""
    from lavie_amd import ops
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(3, rows, 512, generator=g) + 0.5).half()
    got = oc.run_guarded(lambda i, o: ops.mean_rows(i["x"], out=o["y"]), {"x": x}, {"y": ((3, 512), torch.float32)}, sync=sync)["y"]
    c = (math.ceil(rows / 4) + 3) * 2.0 ** -24
    oc.assert_elementwise(got, x.double().mean(1), x.double().abs().mean(1), c, where=oc.loc_rows(512), label=f"mean_rows {rows}", u=oc.U32)


def test_mean_rows_narrow_and_ragged_channel_counts():
    from lavie_amd import ops
    x = torch.randn(2, 9, 70).half()
    got = oc.run_guarded(lambda i, o: ops.mean_rows(i["x"], out=o["y"]), {"x": x}, {"y": ((2, 70), torch.float32)}, sync=sync)["y"]
    oc.assert_elementwise(got, x.double().mean(1), x.double().abs().mean(1), 6 * 2.0 ** -24, label="mean_rows C=70", u=oc.U32)


# ------------------------------------------------------------------ bit properties
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def test_clip_of_a_batch_has_the_bits_of_its_single_clip_call():
    from lavie_amd import ops
    ins, _ = conv_operands(3, 3, 6, 10, 128, 128, 3, 1, True, seed=5)
    dev = {k: v.cuda() for k, v in ins.items()}
    wp = ops.pack_conv3d(dev["w"])
    for stride in (1, 2):
        res = dev["res"] if stride == 1 else None
        whole = ops.conv3d(dev["x"], wp, dev["bias"], stride=stride, residual=res, relu=True)
        again = ops.conv3d(dev["x"], wp, dev["bias"], stride=stride, residual=res, relu=True)
        assert torch.equal(bits(whole), bits(again))
        for i in range(3):
            one = ops.conv3d(dev["x"][i:i + 1], wp, dev["bias"], stride=stride, residual=None if res is None else res[i:i + 1], relu=True)
            assert torch.equal(bits(one[0]), bits(whole[i])), (stride, i)
    sins = stem_operands(3, 2, 7, 9, torch.float32, seed=6)
    px, swp, sb = sins["px"].cuda(), ops.pack_conv3d(sins["w"].cuda()), sins["bias"].cuda()
    whole = ops.conv3d_stem(px, swp, sb)
    assert torch.equal(bits(whole), bits(ops.conv3d_stem(px, swp, sb)))
    for i in range(3):
        assert torch.equal(bits(ops.conv3d_stem(px[i:i + 1], swp, sb)[0]), bits(whole[i])), i
    rows = whole.reshape(3, -1, 64)
    mean = ops.mean_rows(rows)
    assert torch.equal(bits(mean), bits(ops.mean_rows(rows)))
    for i in range(3):
        assert torch.equal(bits(ops.mean_rows(rows[i:i + 1])[0]), bits(mean[i])), i


def test_aliased_residual_gives_the_bits_of_a_separate_one():
    from lavie_amd import ops
    ins, _ = conv_operands(2, 3, 6, 10, 64, 64, 3, 1, True, seed=8)
    dev = {k: v.cuda() for k, v in ins.items()}
    wp = ops.pack_conv3d(dev["w"])
    want = ops.conv3d(dev["x"], wp, dev["bias"], residual=dev["res"], relu=True)
    buf = dev["res"].clone()
    ops.conv3d(dev["x"], wp, dev["bias"], residual=buf, relu=True, out=buf)
    assert torch.equal(bits(buf), bits(want))


# ------------------------------------------------------------------ refusals
def test_operands_of_the_wrong_kind_are_refused_not_misread():
    from lavie_amd import ops
    ins, _ = conv_operands(1, 2, 4, 6, 64, 64, 3, 1, False, seed=9)
    x, w, b = ins["x"].cuda(), ins["w"].cuda(), ins["bias"].cuda()
    wp = ops.pack_conv3d(w)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.conv3d(x[:, :, :, ::2], wp, b)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.conv3d(x.float(), wp, b)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.conv3d(x, wp, b.half())
    with pytest.raises(ValueError, match="do not belong"):
        ops.conv3d(x, wp, b, ksize=1, stride=2)
    with pytest.raises(ValueError, match="residual must be"):
        ops.conv3d(x, wp, b, residual=x[:, :1])
    with pytest.raises(RuntimeError, match=r"kernel \(3,3,3\) stride 3 is not built"):
        ops.conv3d(x, wp, b, stride=3)
    w96 = torch.zeros(96, 64, 3, 3, 3, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="Cin=64 Cout=96 must each be 64, 128, 256 or 512"):
        ops.conv3d(x, ops.pack_conv3d(w96), torch.zeros(96, device="cuda"))
    px = torch.randn(1, 3, 2, 8, 10, device="cuda")
    swp, sb = ops.pack_conv3d(torch.zeros(64, 3, 3, 7, 7, dtype=torch.float16, device="cuda")), torch.zeros(64, device="cuda")
    with pytest.raises(ValueError, match="planes of pixels must be contiguous"):
        ops.conv3d_stem(px[..., ::2], swp, sb)
    with pytest.raises(ValueError, match="fp16 or fp32"):
        ops.conv3d_stem(px.double(), swp, sb)
    with pytest.raises(ValueError, match="3 channels"):
        ops.conv3d_stem(px, swp, sb, layout="ntchw")
    with pytest.raises(ValueError, match=r"\[64, 448\]"):
        ops.conv3d_stem(px, wp, sb)
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.mean_rows(torch.zeros(2, 4, 64, device="cuda"))
    with pytest.raises(ValueError, match="contiguous fp16"):
        ops.mean_rows(torch.zeros(2, 4, 128, dtype=torch.float16, device="cuda")[:, :, ::2])
