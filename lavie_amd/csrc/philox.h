// Seeded engine noise: a standard normal as a pure function of (a latent's 64-bit seed, a 64-bit draw number, the element's flat
// index e inside ONE latent [C, F, h, w]).  No state in memory: a kernel makes the value in registers, and a latent gets the same
// noise alone, in any batch, on any rank, under any window split.
//   words = Philox4x32-10(key = (lo, hi of seed), counter = (lo, hi of e >> 2, lo, hi of draw))      (Salmon et al., SC'11)
//   elements 4 (e >> 2) + 0, 1 from the pair (w0, w1), + 2, 3 from (w2, w3); for a pair (a, b):
//   u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1), both exact in fp32
//   r = sqrt(-2 ln u1);  first = r cos(2 pi u2), second = r sin(2 pi u2)
// The integer part is plain C++ and also builds for the host (lavie_philox4x32_host, the CPU tests, `make asan`).  The transform is
// one __device__ __forceinline__ function, contraction off, in the style of sampler_element.h: logf, a correctly rounded sqrtf and
// sincospif of the exact 2 u2 (no rounded 2 pi u2 exists), then ONE fp32 multiply per value.  Every kernel calls this one function,
// so the materialised tensor (sampler_noise.hip) and a fused step (sampler_noise.hip, sampler_window.hip) hold the same bits.
// u1 == 1 gives ln = 0, r = -0 and the values +-0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LAVIE_HD __host__ __device__
#else
#define LAVIE_HD
#endif

namespace lavie {

constexpr int kNoiseMaxSeeds = 16;          // LAVIE_NOISE_MAX_SEEDS: latents of one seeded launch

// The key of a seeded launch, a kernel argument: no device-side table exists.  seed[p] = latent p's seed; `per` = elements of one latent.
struct NoiseKey {
    unsigned long long seed[kNoiseMaxSeeds];
    unsigned long long draw;
    long long per;
    int count;                                // 0: no key (the step reads its noise from `aux`)
};

LAVIE_HD inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&w)[4]) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the four words of block `block` = e >> 2 of (seed, draw)
LAVIE_HD inline void philox_block(unsigned long long seed, unsigned long long draw, unsigned long long block, uint32_t (&w)[4]) {
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)block, (uint32_t)(block >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), w);
}

#if defined(__HIPCC__)
// one pair of words -> two normals
__device__ __forceinline__ void philox_normal_pair(uint32_t a, uint32_t b, float& first, float& second) {
#pragma clang fp contract(off)
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(b >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(2.f * u2, &s, &c);
    first = r * c;
    second = r * s;
}

// The normals of elements e0 .. e0 + V - 1 of latent (seed, draw).  V == 8: e0 % 4 == 0, two blocks; V == 1: any e0, the element's
// pair alone, through the same function.
template <int V>
__device__ __forceinline__ void philox_normals(unsigned long long seed, unsigned long long draw, unsigned long long e0, float (&n)[V]) {
    static_assert(V == 8 || V == 1, "eight elements per lane or one");
    uint32_t w[4];
    if constexpr (V == 8) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            philox_block(seed, draw, (e0 >> 2) + b, w);
            philox_normal_pair(w[0], w[1], n[4 * b], n[4 * b + 1]);
            philox_normal_pair(w[2], w[3], n[4 * b + 2], n[4 * b + 3]);
        }
    } else {
        philox_block(seed, draw, e0 >> 2, w);
        const bool high = (e0 & 2) != 0;
        float first, second;
        philox_normal_pair(high ? w[2] : w[0], high ? w[3] : w[1], first, second);
        n[0] = (e0 & 1) ? second : first;
    }
}
#endif

}  // namespace lavie
