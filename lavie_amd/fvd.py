"""FVD on the engine: R3D-18 features of video clips and the Fréchet distance between two sets of them.

`HipR3D18` is the 18-layer video ResNet of Tran et al. (2018) without its classifier, on the 3-D convolution kernels of the library:
`model(pixel_values [N, 3, T, H, W])` is fp32 `[N, 512]`.  `VideoProcessor` is the per-frame transform in front of it (centre crop,
Pillow's bilinear resize, 1 / 255, normalise) on the device, bit-equal to Pillow followed by the fp32 normalisation.
`frechet_distance` and `FrechetStats` are float64 host code; `FvdScorer` ties the three together.  Two calls agree bit for bit, and
a clip's features do not depend on the batch."""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._engine_object import _EngineObject, _load

IMAGENET_MEAN, IMAGENET_STD = ops.IMAGENET_MEAN, ops.IMAGENET_STD
BN_EPS = 1e-5
FEATURES = 512
_BN_PARTS = ("weight", "bias", "running_mean", "running_var")
_WIDTHS = (64, 128, 256, 512)


def r3d18_param_shapes():
    """name -> shape of every tensor HipR3D18 takes, in the module's own naming"""
    shapes = {}

    def unit(name, cout, cin, kernel):
        shapes[f"{name}.0.weight"] = (cout, cin) + kernel
        for part in _BN_PARTS:
            shapes[f"{name}.1.{part}"] = (cout,)

    unit("stem", 64, 3, (3, 7, 7))
    cin = 64
    for level, cout in enumerate(_WIDTHS):
        for b in range(2):
            p = f"layer{level + 1}.{b}"
            unit(f"{p}.conv1", cout, cin, (3, 3, 3))
            unit(f"{p}.conv2", cout, cout, (3, 3, 3))
            if level > 0 and b == 0:
                unit(f"{p}.downsample", cout, cin, (1, 1, 1))
            cin = cout
    return shapes


def canonical_key(key):
    """'0.0.weight' -> 'stem.0.weight', '3.1.conv2.1.bias' -> 'layer3.1.conv2.1.bias' (the numeric prefixes of
    nn.Sequential(*children[:-1])); the module's own names pass through"""
    head, dot, rest = key.partition(".")
    if dot and head in ("0", "1", "2", "3", "4"):
        return ("stem" if head == "0" else f"layer{head}") + "." + rest
    return key


def map_state_dict(sd):
    """The tensors HipR3D18 needs under their canonical names.  fc.* and *.num_batches_tracked are dropped; a missing key, an
    unexpected key and a wrong shape raise ValueError with the key's name."""
    shapes = r3d18_param_shapes()
    out = {}
    for key, value in sd.items():
        name = canonical_key(key)
        if name in ("fc.weight", "fc.bias") or name.endswith(".num_batches_tracked"):
            continue
        if name not in shapes:
            raise ValueError(f"HipR3D18: unexpected state-dict key '{key}'")
        if tuple(value.shape) != shapes[name]:
            raise ValueError(f"HipR3D18: '{key}' has shape {tuple(value.shape)}, expected {shapes[name]}")
        out[name] = value
    missing = [k for k in shapes if k not in out]
    if missing:
        raise ValueError(f"HipR3D18: the state dict lacks '{missing[0]}'" + (f" and {len(missing) - 1} more" if len(missing) > 1 else ""))
    return out


def fold_batchnorm(weight, gamma, beta, mean, var, eps=BN_EPS):
    """The fold the engine applies at finalize, on the host: scale = gamma / sqrt(var + eps) in float64; (fp16 weight * scale rounded
    once, fp32 shift = beta - mean * scale)."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    w = (weight.double() * scale.view(-1, *([1] * (weight.dim() - 1)))).to(torch.float16)
    return w, (beta.double() - mean.double() * scale).to(torch.float32)


class HipR3D18(_EngineObject):
    _destroy = "lavie_r3d_destroy"

    def __init__(self, state_dict, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("HipR3D18 lives on a HIP device")
        sd = map_state_dict(state_dict)
        lib = _lib.load()
        handle = ctypes.c_void_p()
        _lib.check(lib.lavie_r3d_create(ctypes.byref(handle)), "lavie_r3d_create")
        self._h = handle
        _load(lib, "lavie_r3d", handle, sd.keys(), sd, self.device, dtype=torch.float32)

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        return cls(sd, device=device)

    @classmethod
    def from_stock(cls, module, device=None):
        """a torchvision r3d_18, or the nn.Sequential of its children without fc"""
        dev = device or next(module.parameters()).device
        return cls(module.state_dict(), device=dev if torch.device(dev).type == "cuda" else "cuda")

    @torch.no_grad()
    def __call__(self, pixel_values, layout="ncthw"):
        """pixel_values fp16 or fp32 [N, 3, T, H, W] (or [N, T, 3, H, W] with layout='ntchw', the processor's frames-major order), read
        in place -> fp32 [N, 512]"""
        if not torch.is_tensor(pixel_values) or not pixel_values.is_cuda or self.device.index not in (None, pixel_values.device.index):
            raise ValueError(f"HipR3D18: pixel_values must be a tensor on {self.device}")
        n, t, h, w, sn, st, sc = ops._stem_strides(pixel_values, layout, "HipR3D18")
        lib = _lib.load()
        need = lib.lavie_r3d_workspace_bytes(self._h, n, t, h, w)
        if need < 0:
            _lib.check(-1, "lavie_r3d_workspace_bytes")
        with torch.cuda.device(self.device):
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            out = torch.empty((n, FEATURES), dtype=torch.float32, device=self.device)
            _lib.check(lib.lavie_r3d_features(self._h, ctypes.c_void_p(pixel_values.data_ptr()), int(pixel_values.dtype == torch.float32), sn, st,
                                              sc, n, t, h, w, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                              ops._stream()), "lavie_r3d_features")
        return out

    forward = __call__


class VideoProcessor:
    """uint8 [F, H, W, 3] or [P, F, H, W, 3] -> frames-major pixel values [P, F, 3, size, size] (P = 1 for one clip) on the device"""

    def __init__(self, crop=270, size=224, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD, dtype=torch.float32, device="cuda"):
        self.crop, self.size = int(crop), int(size)
        self.image_mean, self.image_std = tuple(float(v) for v in image_mean), tuple(float(v) for v in image_std)
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise ValueError("VideoProcessor: image_mean and image_std have three entries")
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"VideoProcessor: dtype {dtype} is not fp32 or fp16")
        self.dtype, self.device = dtype, torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("VideoProcessor lives on a HIP device")

    def _clips(self, video):
        if isinstance(video, (list, tuple)):
            if not video:
                raise ValueError("VideoProcessor: empty list of clips")
            arrays = [v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for v in video]
            if any(a.shape != arrays[0].shape for a in arrays):
                raise ValueError(f"VideoProcessor: mixed sizes {sorted({a.shape for a in arrays})[:3]} in one call are not built: call once "
                                 "per size")
            video = np.stack(arrays)
        if isinstance(video, np.ndarray):
            video = torch.from_numpy(np.ascontiguousarray(video))
        if not torch.is_tensor(video):
            raise ValueError(f"VideoProcessor: {type(video).__name__} is not a tensor, an array or a list of them")
        if video.dtype != torch.uint8:
            raise ValueError(f"VideoProcessor: {video.dtype} pixels are not built: pass uint8 (float frames would need the stock "
                             "transform's own rounding to bytes)")
        if video.dim() == 4:
            video = video[None]
        if video.dim() != 5 or video.shape[-1] != 3:
            raise ValueError(f"VideoProcessor: video must be [F, H, W, 3] or [P, F, H, W, 3], got {tuple(video.shape)}")
        if self.crop > min(video.shape[2], video.shape[3]):
            raise ValueError(f"VideoProcessor: crop={self.crop} is greater than the frame {video.shape[2]} x {video.shape[3]} (the stock "
                             "transform pads there: not built)")
        return video.to(self.device).contiguous()

    def __call__(self, video):
        v = self._clips(video)
        p, f = v.shape[:2]
        px = ops.video_preprocess(v.reshape(p * f, *v.shape[2:]), self.crop, self.size, self.image_mean, self.image_std, dtype=self.dtype)
        return px.view(p, f, 3, self.size, self.size)


def _sym_eigh(m):
    """eigenvalues (ascending) and eigenvectors of the symmetric part of m; eigenvalues below n eps max|w| -- the rounding noise of a
    singular matrix's null space, of either sign -- are set to 0"""
    w, v = np.linalg.eigh((m + m.T) * 0.5)
    floor = m.shape[0] * np.finfo(np.float64).eps * max(float(np.abs(w).max()), 0.0) if w.size else 0.0
    return np.where(w > floor, w, 0.0), v


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrt(S1 S2)) in float64 (Dowson & Landau 1982; Heusel et al. 2017).  tr sqrt(S1 S2) is the sum
    of the square roots of the eigenvalues of the symmetric form S1^(1/2) S2 S1^(1/2), which has the spectrum of S1 S2.  The form is
    taken on the range of S1 (its eigenvectors with a non-zero eigenvalue; on the null space the form is exactly 0), so singular
    covariances -- fewer samples than dimensions -- add no square roots of rounding noise."""
    mu1, mu2 = np.asarray(mu1, np.float64).reshape(-1), np.asarray(mu2, np.float64).reshape(-1)
    sigma1, sigma2 = np.asarray(sigma1, np.float64), np.asarray(sigma2, np.float64)
    d = mu1.shape[0]
    if mu2.shape[0] != d or sigma1.shape != (d, d) or sigma2.shape != (d, d):
        raise ValueError(f"frechet_distance: shapes {mu1.shape}, {sigma1.shape}, {mu2.shape}, {sigma2.shape} do not agree")
    w1, v1 = _sym_eigh(sigma1)
    keep = w1 > 0.0
    half = v1[:, keep] * np.sqrt(w1[keep])                   # S1^(1/2) = half half^T on S1's range
    eig, _ = _sym_eigh(half.T @ ((sigma2 + sigma2.T) * 0.5) @ half)
    cross = np.sqrt(eig).sum()
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(sigma1) + np.trace(sigma2) - 2.0 * cross)


class FrechetStats:
    """count, sum and outer-product sum of feature rows in float64; shards combine with merge()"""

    def __init__(self, dim=FEATURES):
        self.dim = int(dim)
        self.reset()

    def reset(self):
        self.n = 0
        self.total = np.zeros(self.dim, np.float64)
        self.outer = np.zeros((self.dim, self.dim), np.float64)

    def update(self, features):
        f = features.detach().cpu().numpy() if torch.is_tensor(features) else np.asarray(features)
        f = f.astype(np.float64).reshape(-1, f.shape[-1])
        if f.shape[1] != self.dim:
            raise ValueError(f"FrechetStats: features have {f.shape[1]} columns, expected {self.dim}")
        self.n += f.shape[0]
        self.total += f.sum(0)
        self.outer += f.T @ f
        return self

    def merge(self, other):
        if other.dim != self.dim:
            raise ValueError(f"FrechetStats: merging dim {other.dim} into dim {self.dim}")
        self.n += other.n
        self.total += other.total
        self.outer += other.outer
        return self

    @property
    def mean(self):
        if self.n < 1:
            raise ValueError("FrechetStats: no features yet")
        return self.total / self.n

    @property
    def cov(self):
        """np.cov(features, rowvar=False): the N - 1 normalisation"""
        if self.n < 2:
            raise ValueError("FrechetStats: a covariance needs at least two feature rows")
        m = self.mean
        return (self.outer - self.n * np.outer(m, m)) / (self.n - 1)


class FvdScorer:
    MAX_BATCH = 4             # clips per engine call (16 x 224 x 224: about 0.23 GB of workspace per call)

    def __init__(self, r3d, processor=None):
        self.r3d = r3d
        self.processor = processor or VideoProcessor(device=r3d.device)
        self.real, self.generated = FrechetStats(), FrechetStats()

    @torch.no_grad()
    def features(self, video_u8):
        """uint8 [F, H, W, 3] or [P, F, H, W, 3] -> fp32 [P, 512]"""
        v = self.processor._clips(video_u8)
        out = torch.empty((v.shape[0], FEATURES), dtype=torch.float32, device=self.r3d.device)
        for b0 in range(0, v.shape[0], self.MAX_BATCH):
            out[b0:b0 + self.MAX_BATCH] = self.r3d(self.processor(v[b0:b0 + self.MAX_BATCH]), layout="ntchw")
        return out

    def update_real(self, video_u8):
        f = self.features(video_u8)
        self.real.update(f)
        return f

    def update_generated(self, video_u8):
        f = self.features(video_u8)
        self.generated.update(f)
        return f

    def compute(self):
        return frechet_distance(self.real.mean, self.real.cov, self.generated.mean, self.generated.cov)

    def reset(self):
        self.real.reset()
        self.generated.reset()
