"""numpy restatement of the seeded engine noise (lavie_amd/csrc/philox.h): Philox4x32-10 in uint64 arithmetic and the
normal transform in float64.  Nothing here calls the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# Random123's known-answer vectors for philox4x32_10 (kat_vectors): (counter[4], key[2], expected[4])
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(key, counter):
    """key [..., 2], counter [..., 4] (any integer arrays of 32-bit values) -> uint64 array [..., 4] of 32-bit words."""
    k = np.asarray(key, dtype=np.uint64)
    c = np.asarray(counter, dtype=np.uint64)
    k0, k1 = k[..., 0] & MASK, k[..., 1] & MASK
    c0, c1, c2, c3 = (c[..., i] & MASK for i in range(4))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # 32 x 32 -> 64: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def words(seed: int, draw: int, first: int, count: int):
    """(a, b, second): for elements first .. first + count - 1 of latent (seed, draw) the pair of words each comes from and whether it
    is the pair's second value (the sine)."""
    e = np.arange(first, first + count, dtype=np.uint64)
    block = e >> np.uint64(2)
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    counter = np.stack([block & MASK, block >> np.uint64(32), np.full_like(block, draw & 0xFFFFFFFF), np.full_like(block, draw >> 32)], axis=-1)
    w = philox4x32_10(np.broadcast_to(key, (count, 2)), counter)
    high = (e & np.uint64(2)) != 0
    a = np.where(high, w[:, 2], w[:, 0])
    b = np.where(high, w[:, 3], w[:, 1])
    return a, b, (e & np.uint64(1)) != 0


def uniforms(a, b):
    """u1 in (0, 1], u2 in [0, 1): multiples of 2^-24, exact in fp32 and float64."""
    return ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24, (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normal(seed: int, draw: int, first: int, count: int):
    """float64 normals of elements first .. first + count - 1 of latent (seed, draw)."""
    a, b, second = words(seed, draw, first, count)
    u1, u2 = uniforms(a, b)
    r = np.sqrt(-2.0 * np.log(u1))
    return np.where(second, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2))


def normal_fp32_formula(seed: int, draw: int, first: int, count: int):
    """The same formula evaluated in fp32 by torch on the CPU from the same words: sqrt(-2 log u1) cos / sin (fp32(2 pi) u2).  The
    yardstick of the device's error (same precision, another libm)."""
    import torch
    a, b, second = words(seed, draw, first, count)
    u1, u2 = uniforms(a, b)
    u1, u2 = torch.from_numpy(u1).float(), torch.from_numpy(u2).float()
    r = torch.sqrt(-2.0 * torch.log(u1))
    ang = torch.tensor(2.0 * np.pi, dtype=torch.float32) * u2
    return torch.where(torch.from_numpy(second), r * torch.sin(ang), r * torch.cos(ang)).numpy()
