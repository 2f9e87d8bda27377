// Sampler steps around known latents: the fused guidance + scheduler step of elementwise.hip with the known-region replacement
// of the legacy inpaint / img2img loop folded in, one launch per denoising step, plus the blend that starts such a run.
//
// Operands beside those of the plain step (all fp32, read-only, none may alias x / x0_prev / model_in):
//   known [P, C, inner]   the clean latents to keep                     (inner = frames * height * width)
//   mask  [P, 1, inner]   in [0, 1], broadcast over channels: 1 keep known, 0 free, between: a linear blend
//   noise_known [P, C, inner]   the run's one noise tensor, not read when s_next == 0
//   a_next, s_next        the noise level of the timestep this step lands on
// Per element, fp32:
//   xm = the plain step's x'                      (rounding points of the kernel of the same family, restated below)
//   xk = s_next != 0 ? fma(s_next, noise_known, a_next known) : a_next known
//   x' = m == 0 ? xm : m == 1 ? xk : fma(m, xk - xm, xm)
//   model_in = fp16(x' in_scale), rounded as the kernel of the same family rounds it, one value for both guidance halves
//   multistep family: x0_prev <- m == 0 ? x0 : m == 1 ? known : fma(m, known - x0, x0)   (a pinned element's x0 is known)
// The two selects are exact: m == 0 returns the plain step's bits whatever known / noise_known hold (NaN included), m == 1
// returns xk whatever the model predicted.  Contraction is off and every fused multiply-add is spelled out, as in
// multistep_element (elementwise.hip): the compiler cannot move a rounding point.
//
// Launch shape: blockIdx.y = the (video, channel) plane, blockIdx.x * 256 + lane = the position inside the plane, so the mask
// index needs one scalar division per block and none per lane.  HBM-bound: with inner % 8 == 0 every lane takes eight elements
// with 16-byte accesses (an 8-group cannot straddle a plane, one 32-byte mask read serves it, and n % 8 == 0 keeps the cond
// halves of eps2 / model_in2 aligned); otherwise one element per lane, same arithmetic.  No atomics, no host synchronisation,
// no allocation: capture-safe and bit-reproducible.
#include "common.h"
#include "ops.h"

namespace lavie {

struct StepCoef { float guidance, kx, ke, c0, ct, c4; };     // c4: sigma (five-coefficient family) or c_prev (multistep family)
struct KnownOperands { const float* known; const float* mask; const float* noise; float a, s; };

// The instructions sampler_step_kernel (elementwise.hip) compiles to, spelled out: eps and x0 one fma each, x' the sum of two
// rounded products, then one fma for the step's own noise.  tests/test_gpu_known_region.py holds m == 0 bit-equal to that kernel.
template <bool CFG>
__device__ __forceinline__ float five_coefficient_element(float eu, float ec, float xt, float nz, const StepCoef& c) {
#pragma clang fp contract(off)
    const float eps = CFG ? __builtin_fmaf(c.guidance, ec - eu, eu) : eu;
    const float x0 = __builtin_fmaf(-c.ke, eps, c.kx * xt);
    const float xn = c.ct * xt + c.c0 * x0;
    return c.c4 != 0.f ? __builtin_fmaf(c.c4, nz, xn) : xn;
}

// multistep_element of elementwise.hip, restated (same test).
template <bool CFG, bool HIST>
__device__ __forceinline__ void multistep_known_element(float eu, float ec, float xt, float x0p, const StepCoef& c, float& x0,
                                                        float& xn) {
#pragma clang fp contract(off)
    const float eps = CFG ? __builtin_fmaf(c.guidance, ec - eu, eu) : eu;
    x0 = __builtin_fmaf(-c.ke, eps, c.kx * xt);
    const float d = HIST ? __builtin_fmaf(c.c4, x0 - x0p, x0) : x0;
    xn = c.ct * xt + c.c0 * d;
}

__device__ __forceinline__ float known_select(float m, float free_v, float pinned_v) {
#pragma clang fp contract(off)
    return m == 0.f ? free_v : m == 1.f ? pinned_v : __builtin_fmaf(m, pinned_v - free_v, free_v);
}

// fp16 of the exact product v s, rounded once: the v_fma_mixlo_f16 that sampler_step_kernel and f32_to_f16_kernel compile to.
// Written as the instruction itself because the compiler forms it from (half)(v * s) in some code shapes only (elementwise.hip,
// scaled_f16), and the two forms of this kernel must agree with each other and with those kernels.
__device__ __forceinline__ half_t once_rounded_f16(float v, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned r = 0;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(r) : "v"(s), "v"(v));
    return __builtin_bit_cast(half_t, (unsigned short)r);
#else
    return (half_t)(v * s);
#endif
}

// fp16(fp32(v s)): what multistep_step_kernel writes (scaled_f16 of elementwise.hip).
__device__ __forceinline__ half_t twice_rounded_f16(float v, float s) {
    float p = v * s;
    asm("" : "+v"(p));
    return (half_t)p;
}

template <int W> __device__ __forceinline__ void load_f32(const float* p, float (&v)[W]) {
    if constexpr (W == 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    } else {
        v[0] = p[0];
    }
}
template <int W> __device__ __forceinline__ void store_f32(float* p, const float (&v)[W]) {
    if constexpr (W == 8) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
        p[0] = v[0];
    }
}
template <int W> __device__ __forceinline__ void load_f16(const half_t* p, float (&v)[W]) {
    if constexpr (W == 8) {
        const half8_t h = *reinterpret_cast<const half8_t*>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
    } else {
        v[0] = (float)p[0];
    }
}
template <int W> __device__ __forceinline__ void store_f16(half_t* p, const half_t (&v)[W]) {
    if constexpr (W == 8) {
        half8_t h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = v[j];
        *reinterpret_cast<half8_t*>(p) = h;
    } else {
        p[0] = v[0];
    }
}

// FAM 0: five-coefficient family (aux = the step's noise, read when c4 != 0); FAM 1: multistep family (aux = x0_prev, read when
// HIST, always written); FAM 2: the start blend (no eps, xm = x; CFG = write the model input twice).  W = elements per lane.
template <int FAM, bool CFG, bool HIST, int W>
__global__ __launch_bounds__(256) void known_step_kernel(const half_t* __restrict__ eps2, float* __restrict__ x,
                                                         float* __restrict__ aux, half_t* __restrict__ model_in2, long n,
                                                         int channels, long inner, StepCoef c, KnownOperands k, float in_scale) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * W;
    if (j0 >= inner) return;
    const long i = (long)blockIdx.y * inner + j0;                       // element in [P, C, inner]
    const long mi = (long)(blockIdx.y / (unsigned)channels) * inner + j0;     // its mask element in [P, 1, inner]
    float xt[W], eu[W], ec[W], ax[W], kn[W], nk[W], m[W], xn[W], hist[W];
    half_t h[W];
    load_f32<W>(x + i, xt);
    load_f32<W>(k.known + i, kn);
    if (k.s != 0.f) load_f32<W>(k.noise + i, nk);
    if (k.mask) load_f32<W>(k.mask + mi, m);
    if (FAM != 2) {
        load_f16<W>(eps2 + i, eu);
        if (CFG) load_f16<W>(eps2 + n + i, ec);
    }
    if (FAM == 0 ? c.c4 != 0.f : (FAM == 1 && HIST)) load_f32<W>(aux + i, ax);
#pragma unroll
    for (int j = 0; j < W; ++j) {
#pragma clang fp contract(off)
        const float mj = k.mask ? m[j] : 1.f;
        float x0 = 0.f, xm;
        if (FAM == 0) xm = five_coefficient_element<CFG>(eu[j], CFG ? ec[j] : 0.f, xt[j], c.c4 != 0.f ? ax[j] : 0.f, c);
        else if (FAM == 1) multistep_known_element<CFG, HIST>(eu[j], CFG ? ec[j] : 0.f, xt[j], HIST ? ax[j] : 0.f, c, x0, xm);
        else xm = xt[j];
        const float xk = k.s != 0.f ? __builtin_fmaf(k.s, nk[j], k.a * kn[j]) : k.a * kn[j];
        xn[j] = known_select(mj, xm, xk);
        if (FAM == 1) hist[j] = known_select(mj, x0, kn[j]);
        h[j] = FAM == 1 ? twice_rounded_f16(xn[j], in_scale) : once_rounded_f16(xn[j], in_scale);
    }
    if (FAM == 1) store_f32<W>(aux + i, hist);
    store_f32<W>(x + i, xn);
    store_f16<W>(model_in2 + i, h);
    if (CFG) store_f16<W>(model_in2 + n + i, h);
}

template <int FAM, bool CFG, bool HIST>
static int launch_known(const half_t* eps2, float* x, float* aux, half_t* model_in2, int64_t n, const StepCoef& c,
                        const KnownOperands& k, int channels, int64_t inner, float in_scale, hipStream_t stream) {
    const int64_t planes = n / inner;
    LAVIE_CHECK(planes >= 1 && planes <= 65535, "known-region step: %lld (video, channel) planes do not fit one launch",
                (long long)planes);
    const bool vec = inner % 8 == 0;
    const int64_t blocks = ((vec ? inner / 8 : inner) + 255) / 256;
    LAVIE_CHECK(blocks <= 0x7fffffff, "known-region step: inner=%lld does not fit one launch", (long long)inner);
    auto kern = vec ? known_step_kernel<FAM, CFG, HIST, 8> : known_step_kernel<FAM, CFG, HIST, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)planes), dim3(256), 0, stream, eps2, x, aux, model_in2, (long)n,
                       channels, (long)inner, c, k, in_scale);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_sampler_step_known(bool cfg, const half_t* eps2, float* x, const float* noise, half_t* model_in2, int64_t n,
                              float guidance, float kx, float ke, float c0, float ct, float sigma, float in_scale,
                              const float* known, const float* mask, const float* noise_known, int channels, int64_t inner,
                              float a_next, float s_next, hipStream_t stream) {
    const StepCoef c{guidance, kx, ke, c0, ct, sigma};
    const KnownOperands k{known, mask, noise_known, a_next, s_next};
    float* aux = const_cast<float*>(noise);              // FAM 0 only reads it
    return cfg ? launch_known<0, true, false>(eps2, x, aux, model_in2, n, c, k, channels, inner, in_scale, stream)
               : launch_known<0, false, false>(eps2, x, aux, model_in2, n, c, k, channels, inner, in_scale, stream);
}

int launch_multistep_step_known(bool cfg, const half_t* eps2, float* x, float* x0_prev, half_t* model_in2, int64_t n,
                                float guidance, float kx, float ke, float c0, float ct, float cp, float in_scale,
                                const float* known, const float* mask, const float* noise_known, int channels, int64_t inner,
                                float a_next, float s_next, hipStream_t stream) {
    const StepCoef c{guidance, kx, ke, c0, ct, cp};
    const KnownOperands k{known, mask, noise_known, a_next, s_next};
    if (cfg)
        return cp != 0.f ? launch_known<1, true, true>(eps2, x, x0_prev, model_in2, n, c, k, channels, inner, in_scale, stream)
                         : launch_known<1, true, false>(eps2, x, x0_prev, model_in2, n, c, k, channels, inner, in_scale, stream);
    return cp != 0.f ? launch_known<1, false, true>(eps2, x, x0_prev, model_in2, n, c, k, channels, inner, in_scale, stream)
                     : launch_known<1, false, false>(eps2, x, x0_prev, model_in2, n, c, k, channels, inner, in_scale, stream);
}

int launch_known_blend(float* x, half_t* model_in, bool dup, int64_t n, float in_scale, const float* known, const float* mask,
                       const float* noise_known, int channels, int64_t inner, float a_next, float s_next, hipStream_t stream) {
    const StepCoef c{};
    const KnownOperands k{known, mask, noise_known, a_next, s_next};
    return dup ? launch_known<2, true, false>(nullptr, x, nullptr, model_in, n, c, k, channels, inner, in_scale, stream)
               : launch_known<2, false, false>(nullptr, x, nullptr, model_in, n, c, k, channels, inner, in_scale, stream);
}

}  // namespace lavie
