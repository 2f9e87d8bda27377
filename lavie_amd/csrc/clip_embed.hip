// CLIPModel's feature heads and the CLIPSIM reduction.
//   clip_embed_kernel        out[b, :] = normalise?(W LN?(x[b, row_b, :])), fp32: the pooled row of a tower's hidden states through
//                            post_layernorm (vision) and visual_projection / text_projection, then the L2 normalisation
//   clip_similarity_kernel   logits[n, p] = s <img_n, txt_p>, or clipsim[p] = (100 / F) sum_f <img_{p F + f}, txt_p>
// One workgroup of four waves per item, so an item's bits do not know B or its position.
// Row choice (CLIPTextTransformer's pooling): eos_token_id == 2 -> the first maximum of the ids (the legacy rule), otherwise the first
// position equal to eos_token_id and row 0 when there is none; without ids the fixed row.
// Order of every sum.  LayerNorm: a lane adds its elements c = tid, tid + 256, ... ascending, then the xor butterfly of wave_sum,
// then the four waves' sums in wave order; the mean first, then the squares of x - mean (two passes, fp32, nothing rounded to fp16).
// Projection: output d belongs to one wave; lane l multiplies columns 128 i + 2 l and + 1 for i ascending (two fmaf per step), then
// wave_sum.  Norm: as the LayerNorm sums, over d.  Rounding points are counted for the bound in DESIGN.md 7.19.
// Similarity: one wave per dot product, lane l takes d = l, l + 64, ... ascending, then wave_sum; the grouped form adds its F dot
// products in frame order in one wave and multiplies by 100.0f / F once.  No atomics anywhere.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "ops.h"

namespace lavie {

namespace {

// the four waves' values of `v` (already summed inside each wave), added in wave order; every thread gets the same bits
__device__ __forceinline__ float block_sum4(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                   // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void clip_embed_kernel(const half_t* __restrict__ x, int L, int C, int D, const int* __restrict__ ids, int eos,
                                                         int fixed_row, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         const half_t* __restrict__ W, int normalize, float* __restrict__ out) {
    __shared__ float xs[kClipEmbedMaxWidth];
    __shared__ float ys[kClipEmbedMaxWidth];
    __shared__ float red[4];
    __shared__ int sv[256], si[256];
    __shared__ int srow;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;

    int row = fixed_row;
    if (ids != nullptr) {
        const int* id = ids + (size_t)b * L;
        int bv = INT_MIN, bi = INT_MAX;
        for (int i = tid; i < L; i += 256) {
            const int v = id[i];
            if (eos == 2) {
                if (v > bv) { bv = v; bi = i; }
            } else if (v == eos && bi == INT_MAX) {
                bi = i;
            }
        }
        sv[tid] = bv;
        si[tid] = bi;
        __syncthreads();
        if (tid == 0) {
            int best = INT_MIN, at = INT_MAX;
            for (int t = 0; t < 256; ++t) {
                if (eos == 2) {
                    if (si[t] != INT_MAX && (sv[t] > best || (sv[t] == best && si[t] < at))) { best = sv[t]; at = si[t]; }
                } else if (si[t] < at) {
                    at = si[t];
                }
            }
            srow = at == INT_MAX ? 0 : at;
        }
        __syncthreads();
        row = srow;
    }
    row = row < 0 ? 0 : (row >= L ? L - 1 : row);

    const half_t* xr = x + ((size_t)b * L + row) * C;
    for (int c = tid; c < C; c += 256) xs[c] = (float)xr[c];
    if (gamma != nullptr) {
        float s = 0.f;
        for (int c = tid; c < C; c += 256) s += (float)xr[c];
        const float mean = block_sum4(s, red) / (float)C;
        float q = 0.f;
        for (int c = tid; c < C; c += 256) {
            const float d = (float)xr[c] - mean;
            q = fmaf(d, d, q);
        }
        const float var = block_sum4(q, red) / (float)C;
        const float rstd = 1.0f / sqrtf(var + eps);
        for (int c = tid; c < C; c += 256) xs[c] = ((float)xr[c] - mean) * rstd * gamma[c] + beta[c];
    }
    __syncthreads();

    const int per = D >> 2;                            // D % 128 == 0: a wave's share is a multiple of 32
    for (int d0 = wave * per; d0 < (wave + 1) * per; d0 += 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < C; i += 128) {
            const float x0 = xs[i + 2 * lane], x1 = xs[i + 2 * lane + 1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const half2_t w = *reinterpret_cast<const half2_t*>(W + (size_t)(d0 + q) * C + i + 2 * lane);
                acc[q] = fmaf((float)w[0], x0, acc[q]);
                acc[q] = fmaf((float)w[1], x1, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float y = wave_sum(acc[q]);
            if (lane == 0) ys[d0 + q] = y;
        }
    }
    __syncthreads();

    float* o = out + (size_t)b * D;
    if (normalize) {
        float s = 0.f;
        for (int d = tid; d < D; d += 256) s = fmaf(ys[d], ys[d], s);
        const float nrm = sqrtf(block_sum4(s, red));
        for (int d = tid; d < D; d += 256) o[d] = ys[d] / nrm;
    } else {
        for (int d = tid; d < D; d += 256) o[d] = ys[d];
    }
}

__device__ __forceinline__ float wave_dot(const float* __restrict__ a, const float* __restrict__ b, int D, int lane) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(a[d], b[d], s);
    return wave_sum(s);
}

// frames == 0: wave = one (n, p) pair of the matrix; frames >= 1: wave = one prompt p, its F images in order
__global__ __launch_bounds__(256) void clip_similarity_kernel(const float* __restrict__ img, const float* __restrict__ txt, float* __restrict__ out,
                                                              int N, int P, int D, int frames, float scale) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (frames == 0) {
        if (w >= (long)N * P) return;
        const int n = (int)(w / P), p = (int)(w - (long)n * P);
        const float v = scale * wave_dot(img + (size_t)n * D, txt + (size_t)p * D, D, lane);
        if (lane == 0) out[w] = v;
    } else {
        if (w >= P) return;
        const float* t = txt + (size_t)w * D;
        float s = wave_dot(img + (size_t)w * frames * D, t, D, lane);
        for (int f = 1; f < frames; ++f) s += wave_dot(img + ((size_t)w * frames + f) * D, t, D, lane);
        if (lane == 0) out[w] = (100.0f / (float)frames) * s;
    }
}

}  // namespace

int launch_clip_embed(const half_t* x, int B, int L, int C, const int* ids_dev, int eos_token_id, int row, const float* gamma, const float* beta,
                      float eps, const half_t* W, int D, bool normalize, float* out, hipStream_t stream) {
    const char* who = "clip_embed";
    LAVIE_CHECK(x && W && out, "%s: null tensor", who);
    LAVIE_CHECK(B >= 1 && B <= 0x7fffffff / 256, "%s: B=%d must be at least 1", who, B);
    LAVIE_CHECK(L >= 1, "%s: L=%d must be at least 1", who, L);
    LAVIE_CHECK(C >= 128 && C % 128 == 0 && C <= kClipEmbedMaxWidth, "%s: C=%d must be a multiple of 128 up to %d", who, C, kClipEmbedMaxWidth);
    LAVIE_CHECK(D >= 128 && D % 128 == 0 && D <= kClipEmbedMaxWidth, "%s: D=%d must be a multiple of 128 up to %d", who, D, kClipEmbedMaxWidth);
    LAVIE_CHECK(ids_dev != nullptr || (row >= 0 && row < L), "%s: row=%d outside [0, L=%d)", who, row, L);
    LAVIE_CHECK((gamma == nullptr) == (beta == nullptr), "%s: the LayerNorm takes both ln_weight and ln_bias or neither", who);
    LAVIE_CHECK(gamma == nullptr || (isfinite(eps) && eps >= 0.f), "%s: eps must be finite and not negative", who);
    LAVIE_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)W & 3) == 0 && ((uintptr_t)out & 3) == 0, "%s: x, w and out must be 4-byte aligned", who);
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)B), dim3(256), 0, stream, x, L, C, D, ids_dev, eos_token_id, row, gamma, beta, eps, W,
                       normalize ? 1 : 0, out);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_clip_similarity(const float* img, const float* txt, float* out, int N, int P, int D, int frames, float scale, hipStream_t stream) {
    const char* who = "clip_similarity";
    LAVIE_CHECK(img && txt && out, "%s: null tensor", who);
    LAVIE_CHECK(N >= 1 && P >= 1 && (long)N * P <= 0x7fffffffL, "%s: N=%d P=%d must be at least 1", who, N, P);
    LAVIE_CHECK(D >= 1, "%s: D=%d must be at least 1", who, D);
    LAVIE_CHECK(frames >= 0, "%s: frames=%d must not be negative", who, frames);
    LAVIE_CHECK(frames == 0 || (long)P * frames == N, "%s: the grouped form needs N = P frames, got N=%d P=%d frames=%d", who, N, P, frames);
    LAVIE_CHECK(frames != 0 || isfinite(scale), "%s: scale must be finite", who);
    LAVIE_CHECK(((uintptr_t)img & 3) == 0 && ((uintptr_t)txt & 3) == 0 && ((uintptr_t)out & 3) == 0, "%s: the tensors must be 4-byte aligned", who);
    const long waves = frames == 0 ? (long)N * P : (long)P;
    hipLaunchKernelGGL(clip_similarity_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, img, txt, out, N, P, D, frames, scale);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
