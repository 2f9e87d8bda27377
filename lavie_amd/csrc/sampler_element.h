// Per-element arithmetic and vector accesses shared by the step kernels that restate the plain sampler steps of elementwise.hip
// with something folded in (sampler_known.hip: the known-region replacement; sampler_window.hip: the fusion of overlapping frame
// windows; sampler_guidance.hip: guidance scale and rescale factor per latent from a table).  Contraction is off and every fused
// multiply-add is spelled out, as in multistep_element (elementwise.hip): the compiler cannot move a rounding point, so a kernel
// built from these pieces gives the plain kernel's bits wherever its own addition is the identity.
#pragma once
#include "common.h"
#include "ops.h"      // StepCoef

namespace lavie {

// eps = eps_u + g (eps_c - eps_u) as one fma; without guidance eps_u itself
template <bool CFG> __device__ __forceinline__ float guided_eps(float eu, float ec, float guidance) {
#pragma clang fp contract(off)
    return CFG ? __builtin_fmaf(guidance, ec - eu, eu) : eu;
}

// The guided eps of a latent whose (guidance, factor) pair comes from a table (sampler_guidance.hip): guided_eps<true> times the
// latent's rescale factor, one fp32 multiply.  f == 1 returns guided_eps<true>'s bits.
__device__ __forceinline__ float scaled_guided_eps(float eu, float ec, float guidance, float f) {
#pragma clang fp contract(off)
    return f * guided_eps<true>(eu, ec, guidance);
}

// The instructions sampler_step_kernel (elementwise.hip) compiles to, spelled out, from eps on: x0 one fma, x' the sum of two
// rounded products, then one fma for the step's own noise.
__device__ __forceinline__ float five_coefficient_from_eps(float eps, float xt, float nz, const StepCoef& c) {
#pragma clang fp contract(off)
    const float x0 = __builtin_fmaf(-c.ke, eps, c.kx * xt);
    const float xn = c.ct * xt + c.c0 * x0;
    return c.c4 != 0.f ? __builtin_fmaf(c.c4, nz, xn) : xn;
}

// multistep_element of elementwise.hip from eps on.
template <bool HIST>
__device__ __forceinline__ void multistep_from_eps(float eps, float xt, float x0p, const StepCoef& c, float& x0, float& xn) {
#pragma clang fp contract(off)
    x0 = __builtin_fmaf(-c.ke, eps, c.kx * xt);
    const float d = HIST ? __builtin_fmaf(c.c4, x0 - x0p, x0) : x0;
    xn = c.ct * xt + c.c0 * d;
}

// The whole element of each family.  tests/test_gpu_known_region.py holds m == 0 bit-equal to the plain kernels.
template <bool CFG>
__device__ __forceinline__ float five_coefficient_element(float eu, float ec, float xt, float nz, const StepCoef& c) {
    return five_coefficient_from_eps(guided_eps<CFG>(eu, ec, c.guidance), xt, nz, c);
}
template <bool CFG, bool HIST>
__device__ __forceinline__ void multistep_known_element(float eu, float ec, float xt, float x0p, const StepCoef& c, float& x0,
                                                        float& xn) {
    multistep_from_eps<HIST>(guided_eps<CFG>(eu, ec, c.guidance), xt, x0p, c, x0, xn);
}

// fp16 of the exact product v s, rounded once: the v_fma_mixlo_f16 that sampler_step_kernel and f32_to_f16_kernel compile to.
// Written as the instruction itself because the compiler forms it from (half)(v * s) in some code shapes only (elementwise.hip,
// scaled_f16), and the two forms of a kernel must agree with each other and with those kernels.
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

}  // namespace lavie
