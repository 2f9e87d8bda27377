// The three operators a CLIP text transformer needs beyond the engine's LayerNorm and Linear:
//   launch_causal_attention   o = softmax_causal(scale q k^T) v over packed q | k | v rows, 1 <= L <= 128, head dim 32 / 64
//   launch_token_embed        out = fp16(float(tok[id]) + float(pos[i])), one rounding
//   launch_act                x <- quick_gelu(x) = x sigmoid(1.702 x) or erf-GELU(x), in place, fp32 with one rounding
//
// Causal attention.  One workgroup of four waves per (batch entry, head); the head's whole K and V live in LDS (128 keys x 64 dims x
// 2 tensors x 2 bytes = 32 KiB, plus row padding), so a query tile is finished in ONE pass: no running maximum, no rescale.  Wave w
// takes the 16-query tiles w, w + 4.  As in attention.hip the products are S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16:
// lane (g = lane >> 4, li = lane & 15) then holds, for ONE query li of the tile, the scores of keys 16 kt + 4 g + r (r = 0..3) of
// every key tile kt, and the four lane groups of a query hold its whole row between them (two shuffles reduce it).
//   * K is staged row-major (row pitch dh + 8 halfs: 16-byte rows, the A operand of a tile is one 16-byte read per 32 dims);
//   * V is staged TRANSPOSED (Vt[d][key], pitch 136 halfs): the A operand of O^T for 32 keys is two 8-byte reads, of keys
//     32 j + 4 g .. + 3 and 32 j + 16 + 4 g .. + 3 -- the order in which the lane's own probabilities sit in the B operand, so P never
//     moves between lanes;
//   * keys past L inside a tile are ZEROS in LDS (never read from memory), so a probability of 0 never meets a NaN or an infinity.
// Masking.  Key j is visible to query i when j <= i and j < L.  A masked score takes no part in the row maximum or the row sum and
// its probability is the constant 0: it is never pushed through exp as -inf (no inf - inf, no 0 inf).  Key tiles past the query tile
// are not multiplied at all.  Every query has key 0, so the maximum is a finite score.
// Rounding points of an output element: P to fp16 in front of the PV product (the row sum is taken over the ROUNDED values, so that
// numerator and denominator agree) and the store: n = 2.  Scores, exponentials, sums and the normalisation are fp32.
// Determinism: a row's sum is its lane's 4 x (key tiles) terms in ascending key order, then lane groups 16 apart, then 32 apart; the
// matrix pipe adds in a fixed order; no atomics.  Nothing depends on the batch entry's index or on NB: an entry has the bits of its
// single-entry call.
// Rows past L inside a query tile compute on row L - 1's values and are never stored.
#include <math.h>

#include "common.h"
#include "onepass_attention.h"
#include "ops.h"

namespace lavie {

namespace {

constexpr int kCaKeys = kCausalMaxL;          // keys (and queries) a workgroup can hold
constexpr int kCaVPitch = kCaKeys + 8;        // row pitch of V^T in halfs: 272 bytes, 8-byte reads at 8-byte offsets

template <int DH>
__global__ __launch_bounds__(256) void causal_attention_kernel(const half_t* __restrict__ qkv, int ld, half_t* __restrict__ o, int ldo,
                                                               int L, int heads, float scale_log2) {
    constexpr int KP = DH + 8;                // K row pitch in halfs: 144 / 80 bytes, 16-byte aligned rows
    constexpr int DC = DH / 32;               // 32-dim chunks of the QK^T contraction
    __shared__ __attribute__((aligned(16))) half_t Ks[kCaKeys * KP];
    __shared__ __attribute__((aligned(16))) half_t Vt[DH * kCaVPitch];

    const int b = blockIdx.x / heads, head = blockIdx.x - b * heads;
    const int C = heads * DH;
    const half_t* base = qkv + (size_t)b * L * ld + head * DH;      // q of row 0; k at + C, v at + 2 C
    const int nqt = cdiv(L, 16);
    const int lpad = cdiv(L, 32) * 32;        // the PV product walks whole 32-key chunks

    onepass_stage_kv<DH>(Ks, Vt, kCaVPitch, base + C, ld, base + 2 * C, ld, L, lpad);
    __syncthreads();

    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int qt = wave; qt < nqt; qt += 4) {
        const int i = 16 * qt + li;                                  // this lane's query
        const half_t* qrow = base + (size_t)(i < L ? i : L - 1) * ld;
        half8_t qf[DC];
#pragma unroll
        for (int c = 0; c < DC; ++c) qf[c] = *reinterpret_cast<const half8_t*>(qrow + 32 * c + 8 * g);

        // scores of the key tiles 0 .. qt, in log2 units
        f32x4 s[8];
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
            s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (kt <= qt) {
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    const half8_t kf = *reinterpret_cast<const half8_t*>(&Ks[(16 * kt + li) * KP + 32 * c + 8 * g]);
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[c], s[kt], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) s[kt][r] *= scale_log2;
            }
        }
        // the true row maximum over the visible keys
        float mx = -3.0e38f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
            if (kt <= qt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * kt + 4 * g + r;
                    if (j <= i && j < L) mx = fmaxf(mx, s[kt][r]);
                }
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // probabilities, rounded once; the row sum over the rounded values
        half8_t pb[4];
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * kt + 4 * g + r;
                half_t ph = (half_t)0.f;
                if (kt <= qt && j <= i && j < L) {
                    ph = (half_t)__builtin_amdgcn_exp2f(s[kt][r] - mx);
                    l += (float)ph;
                }
                pb[kt >> 1][(kt & 1) * 4 + r] = ph;
            }
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;                                  // l >= 1: the maximum's own term
        // O^T = V^T P^T over the 32-key chunks 0 .. qt / 2
        onepass_pv_store<DH, 4>(Vt, kCaVPitch, pb, qt / 2 + 1, inv, g, li, o + ((size_t)b * L + (i < L ? i : L - 1)) * ldo + head * DH, i < L);
    }
}

__global__ __launch_bounds__(256) void token_embed_kernel(const int* __restrict__ ids, const half_t* __restrict__ tok,
                                                          const half_t* __restrict__ pos, half_t* __restrict__ out, int rows, int L, int C,
                                                          int V) {
    const int nvec = C >> 3;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)rows * nvec) return;
    const int row = (int)(idx / nvec), c8 = (int)(idx - (long)row * nvec);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);                        // no id reads outside the table (the callers validate; see ops.h)
    const half8_t t = *reinterpret_cast<const half8_t*>(tok + (size_t)id * C + c8 * 8);
    const half8_t p = *reinterpret_cast<const half8_t*>(pos + (size_t)(row % L) * C + c8 * 8);
    half8_t r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (half_t)((float)t[e] + (float)p[e]);
    *reinterpret_cast<half8_t*>(out + (size_t)row * C + c8 * 8) = r;
}

template <int KIND>
__device__ __forceinline__ half_t act_one(half_t h) {
    const float x = (float)h;
    if constexpr (KIND == 0) return (half_t)(x / (1.0f + __expf(-1.702f * x)));
    else return (half_t)gelu_erf_f(x);
}

// VEC: x is 16-byte aligned, a thread takes eight elements; the last, partial group and an unaligned tensor go element by element
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void act_kernel(half_t* __restrict__ x, long n) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (VEC && i0 + 8 <= n) {
        half8_t v = *reinterpret_cast<half8_t*>(x + i0);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = act_one<KIND>(v[e]);
        *reinterpret_cast<half8_t*>(x + i0) = v;
    } else {
        const long end = i0 + 8 < n ? i0 + 8 : n;
        for (long i = i0; i < end; ++i) x[i] = act_one<KIND>(x[i]);
    }
}

}  // namespace

int launch_causal_attention(const half_t* qkv, int ld, half_t* o, int ldo, int NB, int L, int heads, int dh, float scale,
                            hipStream_t stream) {
    LAVIE_CHECK(qkv && o, "causal_attention: null tensor");
    LAVIE_CHECK(L >= 1 && L <= kCausalMaxL, "causal_attention: L=%d must be 1..%d", L, kCausalMaxL);
    LAVIE_CHECK(dh == 32 || dh == 64, "causal_attention: dh=%d must be 32 or 64", dh);
    LAVIE_CHECK(NB >= 1 && heads >= 1 && (long)NB * heads <= 0x7fffffffL, "causal_attention: NB=%d heads=%d", NB, heads);
    LAVIE_CHECK(ld >= 3 * heads * dh && ld % 8 == 0, "causal_attention: ld=%d must be a multiple of 8 and at least 3 heads dh = %d", ld,
                3 * heads * dh);
    LAVIE_CHECK(ldo >= heads * dh && ldo % 8 == 0, "causal_attention: ldo=%d must be a multiple of 8 and at least heads dh = %d", ldo,
                heads * dh);
    LAVIE_CHECK(aligned16(qkv) && aligned16(o), "causal_attention: qkv and o must be 16-byte aligned");
    LAVIE_CHECK(isfinite(scale), "causal_attention: scale must be finite");
    const float sl2 = scale * kLog2e;
    const dim3 grid((unsigned)(NB * heads));
    if (dh == 64) hipLaunchKernelGGL(causal_attention_kernel<64>, grid, dim3(256), 0, stream, qkv, ld, o, ldo, L, heads, sl2);
    else hipLaunchKernelGGL(causal_attention_kernel<32>, grid, dim3(256), 0, stream, qkv, ld, o, ldo, L, heads, sl2);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_token_embed(const int* ids, const half_t* tok, const half_t* pos, half_t* out, int B, int L, int C, int V, hipStream_t stream) {
    LAVIE_CHECK(ids && tok && pos && out, "token_embed: null tensor");
    LAVIE_CHECK(B >= 1 && L >= 1 && (long)B * L <= 0x7fffffffL / 256, "token_embed: B=%d L=%d", B, L);
    LAVIE_CHECK(C >= 8 && C % 8 == 0, "token_embed: C=%d must be a multiple of 8", C);
    LAVIE_CHECK(V >= 1, "token_embed: V=%d", V);
    LAVIE_CHECK(aligned16(tok) && aligned16(pos) && aligned16(out), "token_embed: the tables and out must be 16-byte aligned");
    const long work = (long)B * L * (C / 8);
    hipLaunchKernelGGL(token_embed_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, ids, tok, pos, out, B * L, L, C, V);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_act(half_t* x, int64_t n, int kind, hipStream_t stream) {
    LAVIE_CHECK(x, "act: null tensor");
    LAVIE_CHECK(n >= 1 && n <= (int64_t)0x7fffffff * 256, "act: n=%lld", (long long)n);
    LAVIE_CHECK(kind == 0 || kind == 1, "act: kind=%d is neither 0 (quick_gelu) nor 1 (gelu)", kind);
    const dim3 grid((unsigned)((n + 2047) / 2048));
    const bool vec = aligned16(x);
    if (kind == 0) {
        if (vec) hipLaunchKernelGGL((act_kernel<0, true>), grid, dim3(256), 0, stream, x, (long)n);
        else hipLaunchKernelGGL((act_kernel<0, false>), grid, dim3(256), 0, stream, x, (long)n);
    } else {
        if (vec) hipLaunchKernelGGL((act_kernel<1, true>), grid, dim3(256), 0, stream, x, (long)n);
        else hipLaunchKernelGGL((act_kernel<1, false>), grid, dim3(256), 0, stream, x, (long)n);
    }
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
