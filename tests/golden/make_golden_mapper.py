"""Generates tests/golden/mapper.pt: the reference's image mapper (base/pipelines/mapping.py:61-97, `MappingNetwork`) at the
production configuration (1024 -> 768, 12 decoder layers of 12 heads, 257 image / 77 text tokens), run on seeded weights and
inputs.  The file holds the state-dict key list and shapes, the recipe (weight seed, input seed, batch) and the reference's
fp32 output as the fixed 8192-element spread (element i * 1000003 mod n); tests/test_mapping_host.py rebuilds weights and
inputs from the recipe and compares lavie_amd.mapping.MappingNetwork against it.

Needs the reference tree (build container only); mapping.py is imported under tests/refshim.  Its module-level imports of
torchvision (the `transforms` name, used only by its __main__ block), transformers and PIL are satisfied by the shim and the
installed packages; nothing of them runs.  Run from the repo root:  python tests/golden/make_golden_mapper.py"""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from lavie_amd import weights  # noqa: E402

REF = "/root/reference/base/pipelines/mapping.py"
SHIM = os.path.join(ROOT, "tests", "refshim")
OUT = os.path.join(HERE, "mapper.pt")
WEIGHT_SEED, INPUT_SEED, BATCH = 23, 5, 2
SAMPLE, STRIDE = 8192, 1_000_003


def sample(t):
    flat = t.reshape(-1)
    n = flat.numel()
    if n <= SAMPLE:
        return flat.clone()
    assert n % STRIDE, n
    return flat[torch.arange(SAMPLE, dtype=torch.int64) * STRIDE % n].clone()


def load_reference():
    # resolved before the shim is on the path: with a `torchvision` importable, transformers would pick its torchvision backend
    from transformers import CLIPModel, CLIPProcessor, CLIPTextModel, CLIPTokenizer  # noqa: F401
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import torchvision                       # the shim: give it the one name mapping.py imports from it
    if not hasattr(torchvision, "transforms"):
        torchvision.transforms = type(sys)("torchvision.transforms")
    spec = importlib.util.spec_from_file_location("ref_mapping", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    torch.manual_seed(0)
    net = ref.MappingNetwork()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = weights.synth_state_dict(shapes, seed=WEIGHT_SEED)
    net.load_state_dict(sd, strict=True)
    net.eval()
    g = torch.Generator().manual_seed(INPUT_SEED)
    image = torch.randn(BATCH, 257, 1024, generator=g)
    text = torch.randn(BATCH, 77, 768, generator=g)
    with torch.no_grad():
        out = net(image, text)
    blob = {"keys": list(shapes), "shapes": {k: list(v) for k, v in shapes.items()}, "weight_seed": WEIGHT_SEED,
            "input_seed": INPUT_SEED, "batch": BATCH, "out_shape": list(out.shape), "out": sample(out)}
    torch.save(blob, OUT)
    print(f"wrote {OUT}: {len(shapes)} tensors, output {tuple(out.shape)}")


if __name__ == "__main__":
    main()
