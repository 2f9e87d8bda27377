"""Test-side model of FreeInit's frequency mix, evaluated literally as published: the filter over the
fftshift-ed spectrum, two 3-D transforms, the blend, the inverse transform and `.real`.  torch.fft on the CPU, float64 unless a
test asks for the float32 yardstick.  Shares no code with lavie_amd/free_init.py."""
import torch

DIMS = (-3, -2, -1)


def published_filter(F, H, W, method, order, ds, dt):
    """float64 [F, H, W] over the SHIFTED spectrum (the centre holds frequency 0), as diffusers' get_3d_filter builds it."""
    out = torch.zeros(F, H, W, dtype=torch.float64)
    if ds == 0 or dt == 0:
        return out
    t = torch.arange(F, dtype=torch.float64).view(F, 1, 1)
    h = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    w = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    d2 = ((ds / dt) * (2 * t / F - 1)) ** 2 + (2 * h / H - 1) ** 2 + (2 * w / W - 1) ** 2
    if method == "butterworth":
        return 1 / (1 + (d2 / ds ** 2) ** order)
    if method == "gaussian":
        return torch.exp(-1 / (2 * ds ** 2) * d2)
    if method == "ideal":
        out[d2 <= (2 * ds) ** 2] = 1.0
        return out
    raise NotImplementedError(method)


def mix(x0, e0, z, a, s, r, lpf_shifted, dtype=torch.float64):
    """mixed = Re IFFT3(LPF .* FFT3(a x0 + s e0) + (1 - LPF) .* FFT3(r z)) over the last three axes, in `dtype`."""
    x0, e0, z, lpf = (t.to(dtype) for t in (x0, e0, z, lpf_shifted))
    z_t = a * x0 + s * e0
    zf = torch.fft.fftshift(torch.fft.fftn(z_t, dim=DIMS), dim=DIMS)
    nf = torch.fft.fftshift(torch.fft.fftn(r * z, dim=DIMS), dim=DIMS)
    mixed = zf * lpf + nf * (1 - lpf)
    return torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=DIMS), dim=DIMS)


def even_part_native(lpf_shifted):
    """The published filter in FFT-native order with its even part taken, (L(k) + L(-k)) / 2, by explicit index tables."""
    native = torch.fft.ifftshift(lpf_shifted, dim=DIMS)
    F, H, W = native.shape
    neg = [(-torch.arange(n)) % n for n in (F, H, W)]
    mirrored = native[neg[0]][:, neg[1]][:, :, neg[2]]
    return (native + mirrored) / 2
