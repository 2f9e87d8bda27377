// Device pieces of the online-softmax attention kernels (attention.hip, attention_wide.hip): one home for the arithmetic
// both files share.  Layout they all assume: S^T = K Q^T, so lane (g = lane >> 4, li = lane & 15) holds, for query li of a
// 16-query tile, the scores of keys 16 kt + 4 g + r (r = 0..3) in s[kt][qt][r]; the four lane groups of a query hold its
// whole key tile between them.  Every helper is inlined into its caller and compiled under that file's own flags.
#pragma once
#include "common.h"
#include "ops.h"

namespace lavie {

constexpr float RESCALE_THR = 8.0f;   // log2 units: running max moves only when a row grows by > 2^8

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));      // the operand of a paired fp32 -> fp16 conversion

// LDS reads at a compile-time offset, untracked by the compiler: in front of a compiler-issued LDS read hipcc drains every
// LDS-DMA in flight (s_waitcnt vmcnt(0)); the caller waits with its own lgkmcnt that the fragments pass through
template <int OFF>
__device__ __forceinline__ u32x2_t lds_read_tr16_asm(unsigned addr) {      // hardware-transposed 8 bytes
    u32x2_t r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}
template <int OFF>
__device__ __forceinline__ u32x2_t lds_read_b64_asm(unsigned addr) {
    u32x2_t r;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}
template <int OFF>
__device__ __forceinline__ u32x4_t lds_read_b128_asm(unsigned addr) {
    u32x4_t r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
    return r;
}

// ---- row of query q in Q, for the fragment loads; rows past Lq read row Lq - 1 (never stored)
__device__ __forceinline__ const half_t* att_q_row(const AttnParams& p, int qb, int head, int dh, int q) {
    q = q < p.Lq ? q : p.Lq - 1;
    return p.q + ((size_t)qb * p.Lq + q) * p.ldq + head * dh;
}

// ---- sparse-causal key/value addressing (AttnParams::sc_frames): key j of batch entry qb = (b, f) is token j % D of frame
// (b, 0) for j < D and of frame (b, max(f - 1, 0)) for j >= D; row(j) is its row in the per-frame K / V tensors
template <bool SC>
struct AttScRows {
    int D, row0, row1;      // first token row of the two key segments; the row of key j >= D is row1 + j
    __device__ __forceinline__ AttScRows(const AttnParams& p, int qb) {
        D = p.Lk >> 1;
        const int f = SC ? qb % p.sc_frames : 0;
        row0 = (qb - f) * D;
        row1 = (qb - (f > 0 ? 1 : 0)) * D - D;
    }
    __device__ __forceinline__ size_t row(int j) const { return (size_t)(j < D ? row0 + j : row1 + j); }
};

// ---- four probabilities of key block `slot` into the P^T operand, rounded to fp16 in pairs: slot 2 j + i fills elements
// 4 i .. 4 i + 3 of the j-th half8_t (pb = that half8_t; at 32-key tiles j = 0)
__device__ __forceinline__ void att_pack4(half8_t& pb, int slot, float e0, float e1, float e2, float e3) {
    const half2_t h0 = __builtin_convertvector((f32x2){e0, e1}, half2_t);
    const half2_t h1 = __builtin_convertvector((f32x2){e2, e3}, half2_t);
    pb[(slot & 1) * 4 + 0] = h0[0];
    pb[(slot & 1) * 4 + 1] = h0[1];
    pb[(slot & 1) * 4 + 2] = h1[0];
    pb[(slot & 1) * 4 + 3] = h1[1];
}

// ---- maximum of the lane's 4 KT scores of query tile qt: a chain of three-input maxima (v_max3_f32: 8 slots for 16 scores;
// the pairwise tree takes 13).  TREE: the pairwise tree, which the register-staged kernel was scheduled around
template <bool TREE, int KT, int QT>
__device__ __forceinline__ float att_lane_max(const f32x4 (&s)[KT][QT], int qt) {
    if constexpr (TREE) {
        float mx = fmaxf(fmaxf(s[0][qt][0], s[0][qt][1]), fmaxf(s[0][qt][2], s[0][qt][3]));
#pragma unroll
        for (int kt = 1; kt < KT; ++kt)
            mx = fmaxf(mx, fmaxf(fmaxf(s[kt][qt][0], s[kt][qt][1]), fmaxf(s[kt][qt][2], s[kt][qt][3])));
        return mx;
    } else {
        float mx = fmaxf(fmaxf(s[0][qt][0], s[0][qt][1]), s[0][qt][2]);
#pragma unroll
        for (int kt = 1; kt < KT; ++kt) {
            mx = fmaxf(fmaxf(mx, s[kt - 1][qt][3]), s[kt][qt][0]);
            mx = fmaxf(fmaxf(mx, s[kt][qt][1]), s[kt][qt][2]);
        }
        return fmaxf(mx, s[KT - 1][qt][3]);
    }
}
// max over the four 16-lane groups holding the same query: two half-swaps instead of ds_bpermute
__device__ __forceinline__ float att_group_max(float mx) {
    const unsigned u = __float_as_uint(mx);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    mx = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned v = __float_as_uint(mx);
    const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// ---- row sum of query li from the lanes' partial sums: reduced over the four lane groups
__device__ __forceinline__ float att_sum_groups(float l) {
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    return l;
}
}  // namespace lavie
