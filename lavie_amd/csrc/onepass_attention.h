// Device pieces of the one-pass attention kernels (text_encoder.hip: causal, L <= 128; image_encoder.hip: bidirectional, Lq, Lk <= 320):
// a head's whole K (row-major) and V (transposed) in LDS, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16, lane layout of
// attention_frag.h (lane (g = lane >> 4, li = lane & 15) holds keys 16 kt + 4 g + r of query li).  The two kernels differ in which
// keys a query sees; staging, the PV product and the store are the same code.  Inlined into the caller, compiled under its flags.
#pragma once
#include "attention_frag.h"

namespace lavie {

constexpr float kLog2e = 1.4426950408889634f;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// K rows [0, lpad) of one head into Ks (row pitch DH + 8 halfs) and V transposed into Vt (Vt[d][key], row pitch vpitch halfs); rows
// at and past L are ZEROS, never read from memory.  k0 / v0: the head's columns of key row 0; 256 threads.
template <int DH>
__device__ __forceinline__ void onepass_stage_kv(half_t* Ks, half_t* Vt, int vpitch, const half_t* __restrict__ k0, int ldk,
                                                 const half_t* __restrict__ v0, int ldv, int L, int lpad) {
    constexpr int KP = DH + 8, PIECES = DH / 8;
    for (int idx = threadIdx.x; idx < lpad * PIECES; idx += 256) {
        const int j = idx / PIECES, c8 = idx - j * PIECES;
        half8_t kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (j < L) {
            kv = *reinterpret_cast<const half8_t*>(k0 + (size_t)j * ldk + c8 * 8);
            vv = *reinterpret_cast<const half8_t*>(v0 + (size_t)j * ldv + c8 * 8);
        }
        *reinterpret_cast<half8_t*>(&Ks[j * KP + c8 * 8]) = kv;
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(c8 * 8 + e) * vpitch + j] = vv[e];
    }
}

// O^T = V^T P^T over the first `nch` 32-key chunks (of at most NCH), times inv, rounded once and stored (when `store`) as the DH
// columns at orow of query li.  pb[j] holds the lane's eight probabilities of chunk j in the order the two 8-byte reads deliver V.
template <int DH, int NCH>
__device__ __forceinline__ void onepass_pv_store(const half_t* Vt, int vpitch, const half8_t (&pb)[NCH], int nch, float inv, int g, int li,
                                                 half_t* orow, bool store) {
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NCH; ++j)
            if (j < nch) {
                const half_t* vrow = &Vt[(16 * dt + li) * vpitch + 32 * j + 4 * g];
                const half4_t v0 = *reinterpret_cast<const half4_t*>(vrow);
                const half4_t v1 = *reinterpret_cast<const half4_t*>(vrow + 16);
                const half8_t vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[j], acc, 0, 0, 0);
            }
        if (store) {
            half4_t out;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[r] = (half_t)(acc[r] * inv);
            *reinterpret_cast<half4_t*>(orow + 16 * dt + 4 * g) = out;
        }
    }
}

}  // namespace lavie
