"""-m gpu: lavie_freeu_f16 (lavie_amd/csrc/freeu.hip) per element: guarded, poisoned operands, two runs bit for bit (opcheck.run_guarded),
against the float64 torch.fft reference under the bound of tests/freeucases.py."""
import pytest
import torch

import freeucases as FC
import opcheck as oc

pytestmark = pytest.mark.gpu
f16 = torch.float16


@pytest.fixture(scope="module")
def ops():
    from lavie_amd import ops
    return ops


def run(ops, case):
    got = oc.run_guarded(lambda i, o: case.run(ops, i, o), case.inputs, case.outputs, alias=case.alias, sync=torch.cuda.synchronize)
    case.check(got)
    return got


CASES = FC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_freeu_per_element(ops, case):
    """s == 1: the skip comes back bit-equal; b == 1: h comes back bit-equal (freeucases.check_skip / check_h)"""
    run(ops, case)


IN_PLACE = FC.in_place_cases()


@pytest.mark.parametrize("case", IN_PLACE, ids=[c.name for c in IN_PLACE])
def test_freeu_in_place_gives_the_out_of_place_bits(ops, case):
    got = run(ops, case)
    twin = FC.case(case.NI, case.H, case.W, case.C_h, case.C2, case.b, case.s, case.data)
    i = {k: v.cuda() for k, v in twin.inputs.items()}
    h_out, skip_out = ops.freeu(i["h"], i["skip"], twin.NI, twin.H, twin.W, twin.b, twin.s)
    oc.assert_bits(got["h_out"], h_out.cpu(), label=case.name + ":h_out")
    oc.assert_bits(got["skip_out"], skip_out.cpu(), label=case.name + ":skip_out")


@pytest.mark.parametrize("shape", [(3, 10, 16, 1280, 640), (3, 37, 53, 32, 64), (2, 40, 64, 64, 64), (2, 1, 2, 32, 32)], ids=str)
def test_batch_entry_equals_its_single_image_call(ops, shape):
    NI, H, W, C_h, C2 = shape
    case = FC.case(*shape, 1.6, 0.2, "offset8")
    i = {k: v.cuda() for k, v in case.inputs.items()}
    h_all, skip_all = ops.freeu(i["h"], i["skip"], NI, H, W, case.b, case.s)
    P = H * W
    for n in range(NI):
        h_n, skip_n = ops.freeu(i["h"][n * P:(n + 1) * P].contiguous(), i["skip"][n * P:(n + 1) * P].contiguous(), 1, H, W, case.b, case.s)
        oc.assert_bits(h_all[n * P:(n + 1) * P], h_n.cpu(), label=f"image {n}: h")
        oc.assert_bits(skip_all[n * P:(n + 1) * P], skip_n.cpu(), label=f"image {n}: skip")


@pytest.mark.parametrize("C_h,C2,text", [(32, 12, "C2=12"), (24, 32, "C_h=24")])
def test_refused_shapes_leave_every_band_intact(ops, C_h, C2, text):
    """the kernel's own message, and nothing written: run_guarded checks every band of a refused call"""
    NI, H, W = 2, 2, 2
    g = torch.Generator().manual_seed(5)
    ins = {"h": torch.randn(NI * H * W, C_h, generator=g).to(f16), "skip": torch.randn(NI * H * W, C2, generator=g).to(f16)}
    outs = {"h_out": ((NI * H * W, C_h), f16), "skip_out": ((NI * H * W, C2), f16)}
    with pytest.raises(RuntimeError, match=text):
        oc.run_guarded(lambda i, o: ops.freeu(i["h"], i["skip"], NI, H, W, 1.2, 0.9, out=(o["h_out"], o["skip_out"])), ins, outs,
                       sync=torch.cuda.synchronize)


def test_out_checks(ops):
    h, skip = torch.zeros(8, 32, dtype=f16, device="cuda"), torch.zeros(8, 32, dtype=f16, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        ops.freeu(h, skip, 2, 2, 2, 1.2, 0.9, out=(torch.zeros(8, 16, dtype=f16, device="cuda"), None))
    with pytest.raises(ValueError):
        ops.freeu(h, skip, 2, 2, 2, 1.2, 0.9, out=(None, torch.zeros(8, 32, dtype=torch.float32, device="cuda")))
    with pytest.raises(ValueError, match="row matrices"):
        ops.freeu(h, skip, 3, 2, 2, 1.2, 0.9)
