// The two ends of the denoising objective evaluated forward: the noised model input in front of the UNet and the mean
// squared error against the regenerated target behind it.  The noise is the function of philox.h at (seed[p], draw, e), made in
// registers on both sides: no noise tensor, no fp32 noisy tensor, no target and no squared difference is ever written.
//
// Per latent p (a = sqrt(abar_t), s = sqrt(1 - abar_t) of the latent's timestep, fp32 kernel arguments), per element e, all fp32:
//   n     = philox_normals(seed[p], draw, e)
//   n     = fma(coef, m, n)   with offset noise: m = the normal of element e / hw of (seed[p], draw_offset), one value per (channel, frame)
//   noisy_latents_kernel:    v = s != 0 ? fma(s, n, a x0) : a x0;  model_in = once_rounded_f16(v, 1)
//   denoising_loss_kernel:   target = n (epsilon) | fma(a, n, -(s x0)) (v_prediction) | x0 (sample);  d = pred - target;  sum += d d
// Contraction is off and every fused multiply-add is spelled out (sampler_element.h), so both kernels hold the same n and the
// eight-element and one-element forms hold the same bits.
// blockIdx.y = the latent: seed, levels and row base are block-uniform.  per % 8 == 0 and 16-byte aligned tensors: eight elements per
// lane, 16-byte accesses; otherwise one element per access.
// The loss sums in a fixed order, as sampler_guidance.hip does: a block owns kLossChunk elements of one latent whatever the grid or P;
// lane t adds the squares of elements 8 t .. 8 t + 7 of the chunk in ascending order (one fma each, in both forms), a 6-level
// butterfly in the wave, the four waves added in wave order: summation depth 8 + 6 + 3 = 17.  partials[latent][chunk].
// denoising_loss_fold_kernel, its own launch, one workgroup per latent: lane t adds chunks t, t + 256, ... in ascending order, then
// a fixed 8-level tree over the lanes, all in double; out[p] = fp32(sum / per).  No atomics, no allocation: capture-safe; a latent's
// value reads that latent only.
#include "common.h"
#include "ops.h"
#include "philox.h"
#include "sampler_element.h"

namespace lavie {

// elements j0 .. j0 + V - 1 of latent p's noise, the offset term included
template <int V>
__device__ __forceinline__ void training_noise(const NoiseKey& key, int p, const OffsetNoise& off, long j0, float (&n)[V]) {
#pragma clang fp contract(off)
    philox_normals<V>(key.seed[p], key.draw, (unsigned long long)j0, n);
    if (off.hw == 0) return;
    float m[1];
    if (V == 8 && off.hw % 8 == 0) {        // the eight elements lie in one (channel, frame) plane
        philox_normals<1>(key.seed[p], off.draw, (unsigned long long)(j0 / off.hw), m);
#pragma unroll
        for (int j = 0; j < V; ++j) n[j] = __builtin_fmaf(off.coef, m[0], n[j]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            philox_normals<1>(key.seed[p], off.draw, (unsigned long long)((j0 + j) / off.hw), m);
            n[j] = __builtin_fmaf(off.coef, m[0], n[j]);
        }
    }
}

template <bool X32, int V> __device__ __forceinline__ void load_x0(const void* x0, long i, float (&v)[V]) {
    if constexpr (X32) load_f32<V>(static_cast<const float*>(x0) + i, v);
    else load_f16<V>(static_cast<const half_t*>(x0) + i, v);
}

__device__ __forceinline__ float noised_element(float x0, float n, float a, float s) {
#pragma clang fp contract(off)
    const float ax = a * x0;
    return s != 0.f ? __builtin_fmaf(s, n, ax) : ax;
}

__device__ __forceinline__ float loss_target(int kind, float x0, float n, float a, float s) {
#pragma clang fp contract(off)
    if (kind == kLossEpsilon) return n;
    if (kind == kLossVPrediction) return __builtin_fmaf(a, n, -(s * x0));
    return x0;
}

template <bool X32, int V>
__global__ __launch_bounds__(256) void noisy_latents_kernel(const void* __restrict__ x0, half_t* __restrict__ model_in, NoiseKey key,
                                                            NoiseLevels lv, OffsetNoise off) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= key.per) return;
    const int p = blockIdx.y;
    const float a = lv.a[p], s = lv.s[p];
    const long i = (long)p * key.per + j0;
    float x[V], n[V];
    half_t h[V];
    load_x0<X32, V>(x0, i, x);
    if (s != 0.f) training_noise<V>(key, p, off, j0, n);
#pragma unroll
    for (int j = 0; j < V; ++j) h[j] = once_rounded_f16(noised_element(x[j], s != 0.f ? n[j] : 0.f, a, s), 1.f);
    store_f16<V>(model_in + i, h);
}

// V = 8: one 16-byte load of pred and x0 per lane; V = 1: the same eight elements of the lane, one at a time: the same adds per lane.
template <bool X32, int V>
__global__ __launch_bounds__(256) void denoising_loss_kernel(const half_t* __restrict__ pred, const void* __restrict__ x0, NoiseKey key,
                                                             NoiseLevels lv, OffsetNoise off, int kind, int chunks,
                                                             float* __restrict__ partials) {
    __shared__ float red[4];
    const int p = blockIdx.y;
    const float a = lv.a[p], s = lv.s[p];
    const long base = (long)p * key.per;
    const long j0 = (long)blockIdx.x * kLossChunk + (long)threadIdx.x * 8;
    const bool noise = kind != kLossSample;
    float sum = 0.f;
    if constexpr (V == 8) {
        if (j0 < key.per) {
            float pr[8], x[8], n[8];
            load_f16<8>(pred + base + j0, pr);
            load_x0<X32, 8>(x0, base + j0, x);
            if (noise) training_noise<8>(key, p, off, j0, n);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float d = pr[k] - loss_target(kind, x[k], noise ? n[k] : 0.f, a, s);
                sum = __builtin_fmaf(d, d, sum);
            }
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < 8; ++k) {
            const long j = j0 + k;
            if (j < key.per) {
                float pr[1], x[1], n[1];
                load_f16<1>(pred + base + j, pr);
                load_x0<X32, 1>(x0, base + j, x);
                if (noise) training_noise<1>(key, p, off, j, n);
                const float d = pr[0] - loss_target(kind, x[0], noise ? n[0] : 0.f, a, s);
                sum = __builtin_fmaf(d, d, sum);
            }
        }
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long)p * chunks + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void denoising_loss_fold_kernel(const float* __restrict__ partials, long per, int chunks,
                                                                  float* __restrict__ out) {
    __shared__ double red[256];
    const int p = blockIdx.x;
    double s = 0.;
    for (int c = threadIdx.x; c < chunks; c += 256) s += (double)partials[(long)p * chunks + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[p] = (float)(red[0] / (double)per);
}

int64_t denoising_loss_chunks(int64_t per) { return (per + kLossChunk - 1) / kLossChunk; }

static int check_common(const char* who, const NoiseKey& key, const OffsetNoise& off) {
    LAVIE_CHECK(key.count >= 1 && key.count <= kNoiseMaxSeeds, "%s: P=%d outside 1..%d", who, key.count, kNoiseMaxSeeds);
    LAVIE_CHECK(key.per >= 1, "%s: per=%lld must be >= 1", who, key.per);
    LAVIE_CHECK(off.hw >= 0 && (off.hw == 0 || key.per % off.hw == 0), "%s: offset hw=%lld does not divide per=%lld", who, off.hw, key.per);
    return 0;
}

int launch_noisy_latents(const void* x0, bool x0_f32, half_t* model_in, const NoiseKey& key, const NoiseLevels& lv, const OffsetNoise& off,
                         hipStream_t stream) {
    if (int rc = check_common("noisy_latents", key, off)) return rc;
    const bool vec = key.per % 8 == 0 && (((uintptr_t)x0 | (uintptr_t)model_in) & 15) == 0;
    const int64_t blocks = ((vec ? key.per / 8 : key.per) + 255) / 256;
    LAVIE_CHECK(blocks >= 1 && blocks <= 0x7fffffff, "noisy_latents: per=%lld does not fit one launch", key.per);
    auto kern = x0_f32 ? (vec ? noisy_latents_kernel<true, 8> : noisy_latents_kernel<true, 1>)
                       : (vec ? noisy_latents_kernel<false, 8> : noisy_latents_kernel<false, 1>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)key.count), dim3(256), 0, stream, x0, model_in, key, lv, off);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_denoising_loss(const half_t* pred, const void* x0, bool x0_f32, const NoiseKey& key, const NoiseLevels& lv, const OffsetNoise& off,
                          int kind, float* partials, float* out, hipStream_t stream) {
    if (int rc = check_common("denoising_loss", key, off)) return rc;
    LAVIE_CHECK(kind == kLossEpsilon || kind == kLossVPrediction || kind == kLossSample, "denoising_loss: kind=%d outside 0..2", kind);
    const int64_t chunks = denoising_loss_chunks(key.per);
    LAVIE_CHECK(chunks >= 1 && chunks <= 0x7fffffff, "denoising_loss: per=%lld does not fit one launch", key.per);
    const bool vec = key.per % 8 == 0 && (((uintptr_t)x0 | (uintptr_t)pred) & 15) == 0;
    auto kern = x0_f32 ? (vec ? denoising_loss_kernel<true, 8> : denoising_loss_kernel<true, 1>)
                       : (vec ? denoising_loss_kernel<false, 8> : denoising_loss_kernel<false, 1>);
    hipLaunchKernelGGL(kern, dim3((unsigned)chunks, (unsigned)key.count), dim3(256), 0, stream, pred, x0, key, lv, off, kind, (int)chunks,
                       partials);
    LAVIE_HIP(hipGetLastError());
    hipLaunchKernelGGL(denoising_loss_fold_kernel, dim3((unsigned)key.count), dim3(256), 0, stream, partials, (long)key.per, (int)chunks, out);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
