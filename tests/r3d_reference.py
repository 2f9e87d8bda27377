"""The reference of the FVD tests: R3D-18 (Tran et al. 2018) restated from its published description as a plain nn.Module that
carries the usual checkpoint key names (stem.0 / stem.1, layerL.B.conv1.{0,1}, layerL.B.conv2.{0,1}, layerL.0.downsample.{0,1}, fc),
with random weights and non-trivial BatchNorm running statistics, and Pillow as the reference of the video processor."""
import numpy as np
import torch
from torch import nn

WIDTHS = (64, 128, 256, 512)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _unit(cin, cout, kernel, stride, padding, relu):
    layers = [nn.Conv3d(cin, cout, kernel, stride=stride, padding=padding, bias=False), nn.BatchNorm3d(cout)]
    if relu:
        layers.append(nn.ReLU(inplace=False))
    return nn.Sequential(*layers)


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = _unit(cin, cout, 3, stride, 1, True)
        self.conv2 = _unit(cout, cout, 3, 1, 1, False)
        self.downsample = _unit(cin, cout, 1, stride, 0, False) if stride != 1 or cin != cout else None

    def forward(self, x):
        r = x if self.downsample is None else self.downsample(x)
        return torch.relu(self.conv2(self.conv1(x)) + r)


class R3D18(nn.Module):
    def __init__(self, num_classes=400):
        super().__init__()
        self.stem = _unit(3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), True)
        cin = 64
        for level, cout in enumerate(WIDTHS):
            stride = 1 if level == 0 else 2
            setattr(self, f"layer{level + 1}", nn.Sequential(BasicBlock(cin, cout, stride), BasicBlock(cout, cout, 1)))
            cin = cout
        self.avgpool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Linear(512, num_classes)

    def features(self, x):
        x = self.stem(x)
        for level in range(4):
            x = getattr(self, f"layer{level + 1}")(x)
        return self.avgpool(x).flatten(1)

    def forward(self, x):
        return self.fc(self.features(x))


def make_r3d18(seed=0):
    """eval-mode module, default conv init, BatchNorm: running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5), gamma ~ U(0.5, 1.5),
    beta ~ N(0, 0.1)"""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = R3D18().eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm3d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m


def sequential_state_dict(m):
    """the keys of nn.Sequential(*list(m.children())[:-1]).state_dict(): numeric prefixes, no fc"""
    return nn.Sequential(*list(m.children())[:-1]).state_dict()


def features64(m, x):
    with torch.no_grad():
        return m.double().features(x.double())


def features16_cpu(m, x):
    """the yardstick: the same module in fp16 through stock torch.nn on the CPU"""
    import copy
    with torch.no_grad():
        return copy.deepcopy(m).half().features(x.half()).float()


def centre_offset(n, crop):
    return int(round((n - crop) / 2.0))


def pil_video_frames(frames_u8, crop, size, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [F, H, W, 3] -> fp32 [F, 3, size, size]: Pillow's centre crop and bilinear resize, then (v / 255 - mean) / std in fp32"""
    from PIL import Image
    out = []
    for fr in np.asarray(frames_u8):
        im = Image.fromarray(fr)
        w, h = im.size
        top, left = centre_offset(h, crop), centre_offset(w, crop)
        im = im.crop((left, top, left + crop, top + crop)).resize((size, size), Image.BILINEAR)
        v = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).to(torch.float32) / 255.0
        m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
        s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
        out.append((v - m) / s)
    return torch.stack(out)


def apply_tables(row_u8, xmin, count, coeff):
    """one axis of Pillow's 8-bit resampling from its integer tables: clip((2^21 + sum_t u[xmin + t] k[t]) >> 22)"""
    row = np.asarray(row_u8, np.int64)
    out = np.empty(len(xmin), np.uint8)
    for i in range(len(xmin)):
        acc = (1 << 21) + int((row[xmin[i]:xmin[i] + count[i]] * coeff[i, :count[i]].astype(np.int64)).sum())
        out[i] = min(255, max(0, acc >> 22))
    return out
