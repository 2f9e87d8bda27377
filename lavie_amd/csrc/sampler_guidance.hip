// Guidance from a per-latent table: a guidance scale of its own for every latent of a batched call, and guidance rescale (Lin et al.,
// "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4), inside the fused step, with no host synchronisation.
//
// eps2 = [negative | prompt] holds the fp16 model outputs of P latents of `per` elements each.  For latent p, fp32 unless said:
//   e_i   = fma(g_p, ec_i - eu_i, eu_i)                      guided_eps<true> (sampler_element.h): the value the step itself uses
//   s_t   = std(ec), s_e = std(e) over the latent            unbiased (per - 1), from sums kept in double
//   f_p   = phi s_t / s_e + (1 - phi)                        double, stored as fp32; s_e == 0 gives f_p = 1; a NaN sum gives NaN
//   eps_i = f_p e_i                                          one fp32 multiply, then the family's *_from_eps unchanged
// Three kernels:
//   guidance_moments_kernel   grid (chunks, latents), a chunk = kGuidanceChunk elements whatever the grid or P.  Per lane four fp32
//                             sums (ec, ec^2, e, e^2) over eight elements in ascending order, a 6-level butterfly in the wave,
//                             the four waves added in wave order: summation depth 8 + 6 + 3 = 17.  partials[latent][chunk][4].
//   guidance_fold_kernel      one workgroup per latent, its own launch.  Lane t adds chunks t, t + 256, ... in ascending order, then
//                             a fixed 8-level tree over the lanes, all in double; both variances as (Sxx - Sx^2 / per) / (per - 1);
//                             table[latent] = (g_p, f_p), optionally moments[latent] = the four double sums.
//   scaled_step_kernel        the guided five-coefficient and multistep steps with (g, f) read from table[blockIdx.y]; the forms
//                             around known latents and over frame windows live beside their plain forms (sampler_known.hip,
//                             sampler_window.hip) behind a template parameter.
// With f == 1 the multiply is exact, so a table of (g, 1) gives the bits of the plain kernel of the family.  No atomics, no
// allocation, fixed order of additions: capture-safe, and two runs agree bit for bit.  A latent's sums read that latent only.
#include "common.h"
#include "ops.h"
#include "sampler_element.h"

namespace lavie {

struct GuidanceSources { const half_t* eps[kWindowMaxWindows]; };      // one [2 P, per] prediction per window (one without windows)

__device__ __forceinline__ void moments_add(float eu, float ec, float g, float (&s)[4]) {
#pragma clang fp contract(off)
    const float e = guided_eps<true>(eu, ec, g);
    s[0] += ec;
    s[1] = __builtin_fmaf(ec, ec, s[1]);
    s[2] += e;
    s[3] = __builtin_fmaf(e, e, s[3]);
}

// V = 8: one 16-byte load of each half per lane (per % 8 == 0); V = 1: eight strided elements per lane, the same adds per lane.
template <int V>
__global__ __launch_bounds__(256) void guidance_moments_kernel(GuidanceSources src, const float* __restrict__ guidance_dev,
                                                               float guidance, int P, long per, int chunks,
                                                               float* __restrict__ partials) {
    __shared__ float red[4][4];
    const int lat = blockIdx.y, w = lat / P, p = lat - w * P;
    const half_t* eu_p = src.eps[w] + (long)p * per;
    const half_t* ec_p = eu_p + (long)P * per;
    const float g = guidance_dev ? guidance_dev[p] : guidance;
    const long base = (long)blockIdx.x * kGuidanceChunk;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (V == 8) {
        const long j = base + (long)threadIdx.x * 8;
        if (j < per) {
            float eu[8], ec[8];
            load_f16<8>(eu_p + j, eu);
            load_f16<8>(ec_p + j, ec);
#pragma unroll
            for (int k = 0; k < 8; ++k) moments_add(eu[k], ec[k], g, s);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kGuidanceChunk / 256; ++k) {
            const long j = base + k * 256 + threadIdx.x;
            if (j < per) moments_add((float)eu_p[j], (float)ec_p[j], g, s);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = s[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        partials[((long)lat * chunks + blockIdx.x) * 4 + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    }
}

// partials == nullptr (phi == 0): f = 1 without any statistics.
__global__ __launch_bounds__(256) void guidance_fold_kernel(const float* __restrict__ partials, const float* __restrict__ guidance_dev,
                                                            float guidance, float phi, int P, long per, int chunks,
                                                            float* __restrict__ table, double* __restrict__ moments) {
    __shared__ double red[4][256];
    const int lat = blockIdx.x, p = lat % P;
    double s[4] = {0., 0., 0., 0.};
    if (partials)
        for (int c = threadIdx.x; c < chunks; c += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(partials + ((long)lat * chunks + c) * 4);
            for (int k = 0; k < 4; ++k) s[k] += (double)v[k];
        }
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float f = 1.f;
    if (partials) {
        const double n = (double)per;
        const double var_t = (red[1][0] - red[0][0] * red[0][0] / n) / (n - 1.), var_e = (red[3][0] - red[2][0] * red[2][0] / n) / (n - 1.);
        if (var_t != var_t || var_e != var_e) f = __builtin_nanf("");
        else if (var_e > 0.) f = (float)((double)phi * (sqrt(var_t > 0. ? var_t : 0.) / sqrt(var_e)) + (1. - (double)phi));
    }
    table[2 * lat] = guidance_dev ? guidance_dev[p] : guidance;
    table[2 * lat + 1] = f;
    if (moments)
        for (int k = 0; k < 4; ++k) moments[4 * (long)lat + k] = red[k][0];
}

int64_t guidance_chunks(int64_t per) { return (per + kGuidanceChunk - 1) / kGuidanceChunk; }

int launch_guidance_table(const half_t* const* eps, int W, int P, int64_t per, const float* guidance_dev, float guidance, float phi,
                          float* partials, float* table, double* moments, hipStream_t stream) {
    const int64_t latents = (int64_t)W * P, chunks = guidance_chunks(per);
    LAVIE_CHECK(W >= 1 && W <= kWindowMaxWindows, "guidance table: W=%d outside 1..%d", W, kWindowMaxWindows);
    LAVIE_CHECK(latents >= 1 && latents <= 65535, "guidance table: %lld latents do not fit one launch", (long long)latents);
    LAVIE_CHECK(chunks >= 1 && chunks <= 0x7fffffff, "guidance table: per=%lld does not fit one launch", (long long)per);
    if (phi != 0.f) {
        GuidanceSources src{};
        for (int w = 0; w < W; ++w) src.eps[w] = eps[w];
        auto kern = per % 8 == 0 ? guidance_moments_kernel<8> : guidance_moments_kernel<1>;
        hipLaunchKernelGGL(kern, dim3((unsigned)chunks, (unsigned)latents), dim3(256), 0, stream, src, guidance_dev, guidance, P,
                           (long)per, (int)chunks, partials);
        LAVIE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(guidance_fold_kernel, dim3((unsigned)latents), dim3(256), 0, stream, phi != 0.f ? partials : nullptr,
                       guidance_dev, guidance, phi, P, (long)per, (int)chunks, table, moments);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

// FAM 0: five-coefficient family (aux = the step's noise, read when c4 != 0); FAM 1: multistep family (aux = x0_prev, read when
// HIST, always written).  blockIdx.y = the latent, so its (g, f) pair is block-uniform; V = elements per lane.
template <int FAM, bool HIST, int V>
__global__ __launch_bounds__(256) void scaled_step_kernel(const half_t* __restrict__ eps2, float* __restrict__ x,
                                                          float* __restrict__ aux, half_t* __restrict__ model_in2, long n, long per,
                                                          const float* __restrict__ table, StepCoef c, float in_scale) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= per) return;
    const float g = table[2 * blockIdx.y], f = table[2 * blockIdx.y + 1];
    const long i = (long)blockIdx.y * per + j0;
    float xt[V], eu[V], ec[V], ax[V], xn[V], hist[V];
    half_t h[V];
    load_f32<V>(x + i, xt);
    load_f16<V>(eps2 + i, eu);
    load_f16<V>(eps2 + n + i, ec);
    if (FAM == 0 ? c.c4 != 0.f : HIST) load_f32<V>(aux + i, ax);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float eps = scaled_guided_eps(eu[j], ec[j], g, f);
        if (FAM == 0) xn[j] = five_coefficient_from_eps(eps, xt[j], c.c4 != 0.f ? ax[j] : 0.f, c);
        else multistep_from_eps<HIST>(eps, xt[j], HIST ? ax[j] : 0.f, c, hist[j], xn[j]);
        h[j] = FAM == 1 ? twice_rounded_f16(xn[j], in_scale) : once_rounded_f16(xn[j], in_scale);
    }
    if (FAM == 1) store_f32<V>(aux + i, hist);
    store_f32<V>(x + i, xn);
    store_f16<V>(model_in2 + i, h);
    store_f16<V>(model_in2 + n + i, h);
}

template <int FAM, bool HIST>
static int launch_scaled(const StepArgs& a, hipStream_t stream) {
    const int64_t latents = a.n / a.per;
    LAVIE_CHECK(latents >= 1 && latents <= 65535, "scaled step: %lld latents do not fit one launch", (long long)latents);
    const bool vec = a.per % 8 == 0;
    const int64_t blocks = ((vec ? a.per / 8 : a.per) + 255) / 256;
    LAVIE_CHECK(blocks <= 0x7fffffff, "scaled step: per=%lld does not fit one launch", (long long)a.per);
    auto kern = vec ? scaled_step_kernel<FAM, HIST, 8> : scaled_step_kernel<FAM, HIST, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)latents), dim3(256), 0, stream, a.eps, a.x, a.aux, a.model_in, (long)a.n,
                       (long)a.per, a.table, a.c, a.in_scale);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_step_scaled(const StepArgs& a, hipStream_t stream) {
    if (!a.multistep) return launch_scaled<0, false>(a, stream);
    return a.c.c4 != 0.f ? launch_scaled<1, true>(a, stream) : launch_scaled<1, false>(a, stream);
}

}  // namespace lavie
