// What the CLIP vision tower and the fork's image mapper need beyond the text encoder's operators:
//   launch_short_attention   o = softmax(scale q k^T) v, bidirectional, separate query and key lengths 1 .. 320, head dim 32 / 64,
//                            q, k, v three pointers with their own pitches
//   launch_patch_embed       CLIPVisionEmbeddings: P x P stride-P conv of an NCHW image (no bias) + class row + positions
//   launch_add_rows          out[b, i] = fp16(float(x[b, i]) + float(pos[i])), one rounding (the mapper's target rows)
//   launch_relu              x <- max(x, 0) in place, exact
//
// Short attention follows causal_attention_kernel (text_encoder.hip) and shares its staging and PV code (onepass_attention.h): the
// head's whole K (row-major, pitch dh + 8) and V (transposed, pitch 328 halfs) sit in LDS -- at 320 keys and dh 64 that is 46080 +
// 41984 bytes -- and a 16-query tile is finished in ONE pass by one wave: 20 key tiles = 80 fp32 scores per lane, the true row
// maximum, no running rescale.  The grid is (entry x head, groups of four query tiles): every workgroup stages the head's K and V and
// its wave w takes query tile 4 y + w, so the 257 tokens of ViT-L/14 spread over 5 workgroups per head.  A query's arithmetic does
// not know which workgroup or wave runs it, so the bits do not depend on that choice.
// Masking.  Keys >= Lk inside the last 32-key chunk are ZEROS in LDS (never read from memory), take no part in the maximum or the sum,
// and their probability is the constant 0; key tiles past Lk are not multiplied.  Lk >= 1, so the maximum is a finite score.  Query
// rows past Lq compute on row Lq - 1 and are never stored.
// Rounding points of an output element: P to fp16 in front of PV (the row sum is taken over the rounded P) and the store: n = 2.
// Determinism: a row's sum is its lane's terms in ascending key order, then lane groups 16 apart, then 32 apart; the matrix pipe adds in a
// fixed order; no atomics.  Nothing depends on the entry's index or on NB.
//
// Patch embedding: a gather writes the patches as rows [B G^2, Kp] fp16 (K = 3 P^2 in (channel, y, x) order, the flattening of the conv
// weight, zero-padded to Kp = a multiple of 64) and the class rows fp16(class + position 0); then one pinned GEMM per image adds
// position 1 + g as its residual operand in fp32.  Rounding points of a patch element: the pixel to fp16 (none for fp16 pixels) and the
// store; of a class element: the store.  Per-image launches, row-by-row kernels: an image's rows do not depend on B.
#include <math.h>

#include "common.h"
#include "onepass_attention.h"
#include "ops.h"
#include "pinned_linear.h"

namespace lavie {

namespace {

constexpr int kSaTiles = kShortMaxL / 16;      // key tiles a lane holds scores of
constexpr int kSaChunks = kShortMaxL / 32;     // 32-key chunks of the PV product
constexpr int kSaVPitch = kShortMaxL + 8;      // row pitch of V^T in halfs: 656 bytes, 8-byte reads at 8-byte offsets

template <int DH>
constexpr int sa_lds_bytes() { return (kShortMaxL * (DH + 8) + DH * kSaVPitch) * (int)sizeof(half_t); }

template <int DH>
__global__ __launch_bounds__(256) void short_attention_kernel(const half_t* __restrict__ q, int ldq, const half_t* __restrict__ k, int ldk,
                                                              const half_t* __restrict__ v, int ldv, half_t* __restrict__ o, int ldo, int Lq,
                                                              int Lk, int heads, int kv_shared, float scale_log2) {
    constexpr int KP = DH + 8;                // K row pitch in halfs: 144 / 80 bytes, 16-byte aligned rows
    constexpr int DC = DH / 32;               // 32-dim chunks of the QK^T contraction
    extern __shared__ __attribute__((aligned(16))) half_t sa_smem[];
    half_t* Ks = sa_smem;
    half_t* Vt = sa_smem + kShortMaxL * KP;

    const int b = blockIdx.x / heads, head = blockIdx.x - b * heads;
    const int kb = kv_shared ? 0 : b;          // one memory read by every entry (the mapper's single image)
    const int lpad = cdiv(Lk, 32) * 32;        // the PV product walks whole 32-key chunks
    onepass_stage_kv<DH>(Ks, Vt, kSaVPitch, k + (size_t)kb * Lk * ldk + head * DH, ldk, v + (size_t)kb * Lk * ldv + head * DH, ldv, Lk, lpad);
    __syncthreads();

    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qt = 4 * blockIdx.y + wave;
    if (qt >= cdiv(Lq, 16)) return;
    const int nkt = cdiv(Lk, 16);
    const int i = 16 * qt + li;                                      // this lane's query
    const int ic = i < Lq ? i : Lq - 1;
    const half_t* qrow = q + ((size_t)b * Lq + ic) * ldq + head * DH;
    half8_t qf[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) qf[c] = *reinterpret_cast<const half8_t*>(qrow + 32 * c + 8 * g);

    // scores of every key tile, in log2 units
    f32x4 s[kSaTiles];
#pragma unroll
    for (int kt = 0; kt < kSaTiles; ++kt) {
        s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (kt < nkt) {
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                const half8_t kf = *reinterpret_cast<const half8_t*>(&Ks[(16 * kt + li) * KP + 32 * c + 8 * g]);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[c], s[kt], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] *= scale_log2;
        }
    }
    // the true row maximum over the keys < Lk
    float mx = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < kSaTiles; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * kt + 4 * g + r < Lk) mx = fmaxf(mx, s[kt][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // probabilities, rounded once; the row sum over the rounded values
    half8_t pb[kSaChunks];
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < kSaTiles; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            half_t ph = (half_t)0.f;
            if (16 * kt + 4 * g + r < Lk) {
                ph = (half_t)__builtin_amdgcn_exp2f(s[kt][r] - mx);
                l += (float)ph;
            }
            pb[kt >> 1][(kt & 1) * 4 + r] = ph;
        }
    }
    l = att_sum_groups(l);
    const float inv = 1.0f / l;                                      // l >= 1: the maximum's own term
    onepass_pv_store<DH, kSaChunks>(Vt, kSaVPitch, pb, lpad >> 5, inv, g, li, o + ((size_t)b * Lq + ic) * ldo + head * DH, i < Lq);
}

// rows [0, B G^2): thread = eight columns of one patch row; rows [B G^2, B G^2 + B): the class rows of out
template <typename T>
__global__ __launch_bounds__(256) void patch_gather_kernel(const T* __restrict__ px, half_t* __restrict__ cols, const half_t* __restrict__ cls,
                                                           const half_t* __restrict__ pos, half_t* __restrict__ out, int B, int S, int P,
                                                           int G, int Kp, int C) {
    const int kvec = Kp >> 3, cvec = C >> 3;
    const long npatch = (long)B * G * G * kvec;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < npatch) {
        const int m = (int)(idx / kvec), k8 = (int)(idx - (long)m * kvec) * 8;
        const int b = m / (G * G), gi = m - b * G * G, gy = gi / G, gx = gi - gy * G;
        const int pp = P * P, K = 3 * pp;
        half8_t r;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = k8 + e;
            half_t h = (half_t)0.f;
            if (kk < K) {
                const int c = kk / pp, rem = kk - c * pp, py = rem / P, pxx = rem - py * P;
                h = (half_t)px[(((size_t)b * 3 + c) * S + gy * P + py) * S + gx * P + pxx];
            }
            r[e] = h;
        }
        *reinterpret_cast<half8_t*>(cols + (size_t)m * Kp + k8) = r;
    } else if (idx < npatch + (long)B * cvec) {
        const long j = idx - npatch;
        const int b = (int)(j / cvec), c8 = (int)(j - (long)b * cvec) * 8;
        const half8_t a = *reinterpret_cast<const half8_t*>(cls + c8);
        const half8_t p = *reinterpret_cast<const half8_t*>(pos + c8);
        half8_t r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (half_t)((float)a[e] + (float)p[e]);
        *reinterpret_cast<half8_t*>(out + (size_t)b * (1 + G * G) * C + c8) = r;
    }
}

// w [C, K] -> out [C, Kp], columns K .. Kp - 1 zero
__global__ __launch_bounds__(256) void pack_patch_kernel(const half_t* __restrict__ w, half_t* __restrict__ out, int C, int K, int Kp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * Kp) return;
    const int n = (int)(idx / Kp), kk = (int)(idx - (long)n * Kp);
    out[idx] = kk < K ? w[(size_t)n * K + kk] : (half_t)0.f;
}

__global__ __launch_bounds__(256) void add_rows_kernel(const half_t* __restrict__ x, const half_t* __restrict__ pos, half_t* __restrict__ out,
                                                       int rows, int L, int C) {
    const int nvec = C >> 3;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)rows * nvec) return;
    const int row = (int)(idx / nvec), c8 = (int)(idx - (long)row * nvec) * 8;
    const half8_t a = *reinterpret_cast<const half8_t*>(x + (size_t)row * C + c8);
    const half8_t p = *reinterpret_cast<const half8_t*>(pos + (size_t)(row % L) * C + c8);
    half8_t r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (half_t)((float)a[e] + (float)p[e]);
    *reinterpret_cast<half8_t*>(out + (size_t)row * C + c8) = r;
}

// torch.relu: a negative value becomes +0, everything else (-0, NaN included) keeps its bits
__device__ __forceinline__ half_t relu_one(half_t h) { return h < (half_t)0.f ? (half_t)0.f : h; }

template <bool VEC>
__global__ __launch_bounds__(256) void relu_kernel(half_t* __restrict__ x, long n) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (VEC && i0 + 8 <= n) {
        half8_t v = *reinterpret_cast<half8_t*>(x + i0);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = relu_one(v[e]);
        *reinterpret_cast<half8_t*>(x + i0) = v;
    } else {
        const long end = i0 + 8 < n ? i0 + 8 : n;
        for (long i = i0; i < end; ++i) x[i] = relu_one(x[i]);
    }
}

template <int DH>
int run_short_attention(dim3 grid, hipStream_t stream, const half_t* q, int ldq, const half_t* k, int ldk, const half_t* v, int ldv, half_t* o,
                        int ldo, int Lq, int Lk, int heads, int kv_shared, float sl2) {
    auto kern = short_attention_kernel<DH>;
    constexpr int lds = sa_lds_bytes<DH>();
    static_assert(lds <= 160 * 1024, "K and V of a head do not fit LDS");
    static bool attr_set = false;      // one per instantiation
    if (!attr_set) {
        LAVIE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, q, ldq, k, ldk, v, ldv, o, ldo, Lq, Lk, heads, kv_shared, sl2);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_short_attention(const half_t* q, int ldq, const half_t* k, int ldk, const half_t* v, int ldv, half_t* o, int ldo, int NB, int Lq,
                           int Lk, int heads, int dh, float scale, bool kv_shared, hipStream_t stream) {
    LAVIE_CHECK(q && k && v && o, "short_attention: null tensor");
    LAVIE_CHECK(Lq >= 1 && Lq <= kShortMaxL, "short_attention: Lq=%d must be 1..%d", Lq, kShortMaxL);
    LAVIE_CHECK(Lk >= 1 && Lk <= kShortMaxL, "short_attention: Lk=%d must be 1..%d", Lk, kShortMaxL);
    LAVIE_CHECK(dh == 32 || dh == 64, "short_attention: dh=%d must be 32 or 64", dh);
    LAVIE_CHECK(NB >= 1 && heads >= 1 && (long)NB * heads <= 0x7fffffffL, "short_attention: NB=%d heads=%d", NB, heads);
    const int c = heads * dh;
    LAVIE_CHECK(ldq >= c && ldq % 8 == 0, "short_attention: ldq=%d must be a multiple of 8 and at least heads dh = %d", ldq, c);
    LAVIE_CHECK(ldk >= c && ldk % 8 == 0, "short_attention: ldk=%d must be a multiple of 8 and at least heads dh = %d", ldk, c);
    LAVIE_CHECK(ldv >= c && ldv % 8 == 0, "short_attention: ldv=%d must be a multiple of 8 and at least heads dh = %d", ldv, c);
    LAVIE_CHECK(ldo >= c && ldo % 8 == 0, "short_attention: ldo=%d must be a multiple of 8 and at least heads dh = %d", ldo, c);
    LAVIE_CHECK(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o), "short_attention: q, k, v and o must be 16-byte aligned");
    LAVIE_CHECK(isfinite(scale), "short_attention: scale must be finite");
    const float sl2 = scale * kLog2e;
    const dim3 grid((unsigned)(NB * heads), (unsigned)cdiv(cdiv(Lq, 16), 4));
    if (dh == 64) return run_short_attention<64>(grid, stream, q, ldq, k, ldk, v, ldv, o, ldo, Lq, Lk, heads, kv_shared ? 1 : 0, sl2);
    return run_short_attention<32>(grid, stream, q, ldq, k, ldk, v, ldv, o, ldo, Lq, Lk, heads, kv_shared ? 1 : 0, sl2);
}

int patch_embed_k(int P) { return (3 * P * P + IGEMM_BK - 1) / IGEMM_BK * IGEMM_BK; }

static int check_patch(const char* who, int S, int P, int C) {
    LAVIE_CHECK(P >= 1 && P <= 64, "%s: P=%d must be 1..64", who, P);
    LAVIE_CHECK(S >= P && S % P == 0 && S <= 1024, "%s: S=%d must be a multiple of P=%d up to 1024", who, S, P);
    LAVIE_CHECK(C >= kPinBn && C % kPinBn == 0 && C <= 2048, "%s: C=%d must be a multiple of %d up to 2048", who, C, kPinBn);
    return 0;
}

long long patch_embed_workspace_bytes(int B, int S, int P) {
    if (B < 1 || P < 1 || S < P || S % P != 0) return -1;
    return (long long)up256((size_t)B * (S / P) * (S / P) * patch_embed_k(P) * sizeof(half_t));
}

int launch_pack_patch_embed(const half_t* w, half_t* out, int C, int P, hipStream_t stream) {
    LAVIE_CHECK(w && out, "pack_patch_embed: null tensor");
    if (int rc = check_patch("pack_patch_embed", P, P, C)) return rc;
    const int K = 3 * P * P, Kp = patch_embed_k(P);
    hipLaunchKernelGGL(pack_patch_kernel, dim3((unsigned)(((long)C * Kp + 255) / 256)), dim3(256), 0, stream, w, out, C, K, Kp);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_patch_embed(const void* px, bool px_f32, const half_t* wp, const half_t* cls, const half_t* pos, half_t* out, half_t* cols, int B,
                       int S, int P, int C, hipStream_t stream) {
    LAVIE_CHECK(px && wp && cls && pos && out && cols, "patch_embed: null tensor");
    LAVIE_CHECK(B >= 1 && B <= 1024, "patch_embed: B=%d must be 1..1024", B);
    if (int rc = check_patch("patch_embed", S, P, C)) return rc;
    LAVIE_CHECK(aligned16(wp) && aligned16(cls) && aligned16(pos) && aligned16(out) && aligned16(cols),
                "patch_embed: the weights, tables, workspace and out must be 16-byte aligned");
    const int G = S / P, Kp = patch_embed_k(P), T = 1 + G * G;
    const long work = (long)B * G * G * (Kp / 8) + (long)B * (C / 8);
    const dim3 grid((unsigned)((work + 255) / 256));
    if (px_f32) hipLaunchKernelGGL(patch_gather_kernel<float>, grid, dim3(256), 0, stream, (const float*)px, cols, cls, pos, out, B, S, P, G, Kp, C);
    else hipLaunchKernelGGL(patch_gather_kernel<half_t>, grid, dim3(256), 0, stream, (const half_t*)px, cols, cls, pos, out, B, S, P, G, Kp, C);
    LAVIE_HIP(hipGetLastError());
    for (int b = 0; b < B; ++b)          // rows 1 .. G^2 of image b: patches W^T + position 1 + g, summed in fp32, one rounding
        if (int rc = pinned_linear(cols + (size_t)b * G * G * Kp, Kp, wp, nullptr, pos + C, C, out + ((size_t)b * T + 1) * C, C, G * G, C, Kp, stream))
            return rc;
    return 0;
}

int launch_add_rows(const half_t* x, const half_t* pos, half_t* out, int B, int L, int C, hipStream_t stream) {
    LAVIE_CHECK(x && pos && out, "add_rows: null tensor");
    LAVIE_CHECK(B >= 1 && L >= 1 && (long)B * L <= 0x7fffffffL / 256, "add_rows: B=%d L=%d", B, L);
    LAVIE_CHECK(C >= 8 && C % 8 == 0, "add_rows: C=%d must be a multiple of 8", C);
    LAVIE_CHECK(aligned16(x) && aligned16(pos) && aligned16(out), "add_rows: the tensors must be 16-byte aligned");
    const long work = (long)B * L * (C / 8);
    hipLaunchKernelGGL(add_rows_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, x, pos, out, B * L, L, C);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_relu(half_t* x, int64_t n, hipStream_t stream) {
    LAVIE_CHECK(x, "relu: null tensor");
    LAVIE_CHECK(n >= 1 && n <= (int64_t)0x7fffffff * 256, "relu: n=%lld", (long long)n);
    const dim3 grid((unsigned)((n + 2047) / 2048));
    if (aligned16(x)) hipLaunchKernelGGL(relu_kernel<true>, grid, dim3(256), 0, stream, x, (long)n);
    else hipLaunchKernelGGL(relu_kernel<false>, grid, dim3(256), 0, stream, x, (long)n);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
