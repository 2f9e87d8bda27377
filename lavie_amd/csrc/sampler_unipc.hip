// UniPC (Zhao et al., "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models", arXiv:2302.04867)
// as one fused launch per denoising step: guidance, the x0 prediction, the corrector that recomputes the sample the model was just
// evaluated at, the predictor to the next timestep, the three history writes and the next fp16 model input
// (lavie_amd/scheduling_unipc_multistep.py derives the scalars).  Per element, fp32, contraction off, in this order:
//   eps = eu | fma(g, ec - eu, eu) | f fma(g, ec - eu, eu)          no guidance | scalar guidance | (g, f) from table[latent]
//   m   = fma(-k_eps, eps, round(k_x x))                            multistep_from_eps (sampler_element.h), the same instructions
//   xc  = corr ? fma(c_2, m2, fma(c_1, m1, fma(c_0, m, round(c_l x_last)))) : x        a fused multiply-add whose coefficient is
//                                                                                       zero is skipped, not multiplied by zero
//   x'  = round(p_x xc) + round(p_0 m);   p_1 != 0:  x' = fma(p_1, m1, x')
//   x_last <- xc;  m2 <- m1 (m1 read) or m (m1 not read);  m1 <- m;  x <- x';  model_in <- fp16(fp32(x' in_scale))
// A history buffer is loaded only when a coefficient that multiplies it is non-zero (x_last: corr and c_l; m1: corr and c_1, or
// p_1; m2: corr and c_2): the decision is a launch argument, uniform over the grid, so an unread buffer may hold anything, NaN
// included.  When m1 is not read, m2 receives m instead of a copy of m1: the value is defined, and no step can need it, because a
// step that reads m2 follows a second-order predictor, which read m1.
// With corr == 0 and p_1 == 0 the arithmetic from eps to x' is multistep_from_eps<false> with (c_xt, c_x0) = (p_x, p_0): the
// second-order term is added last, by a fused multiply-add of its own, so leaving it out leaves exactly those instructions, and
// the fp16 conversion is the same twice_rounded_f16: x and model_in have the bits of lavie_multistep_step with c_prev = 0.
// HBM-bound: eight elements per lane with 16-byte accesses when the latent's element count is a multiple of 8 (every tensor is
// then 16-byte aligned, the cond half under guidance included), else one element per lane with the same arithmetic.  No atomics,
// no noise, no allocation, no host synchronisation: bit-reproducible and safe in a stream capture.
#include "common.h"
#include "ops.h"
#include "sampler_element.h"

namespace lavie {

// GM 0: no guidance; 1: scalar guidance; 2: (g, f) per latent from the table (blockIdx.y = the latent)
template <int GM>
__device__ __forceinline__ void unipc_element(float eu, float ec, float g, float f, float xt, float xl, float h1, float h2,
                                              const UnipcCoef& c, float& m, float& xc, float& xn) {
#pragma clang fp contract(off)
    const float eps = GM == 0 ? eu : GM == 1 ? guided_eps<true>(eu, ec, g) : scaled_guided_eps(eu, ec, g, f);
    m = __builtin_fmaf(-c.ke, eps, c.kx * xt);
    xc = xt;
    if (c.corr) {
        float acc = c.cl * xl;
        acc = __builtin_fmaf(c.c0, m, acc);
        if (c.c1 != 0.f) acc = __builtin_fmaf(c.c1, h1, acc);
        if (c.c2 != 0.f) acc = __builtin_fmaf(c.c2, h2, acc);
        xc = acc;
    }
    xn = c.px * xc + c.p0 * m;
    if (c.p1 != 0.f) xn = __builtin_fmaf(c.p1, h1, xn);
}

template <int GM, int V>
__global__ __launch_bounds__(256) void unipc_step_kernel(const half_t* __restrict__ eps2, float* __restrict__ x,
                                                         float* __restrict__ x_last, float* __restrict__ m1, float* __restrict__ m2,
                                                         half_t* __restrict__ model_in2, long n, long per,
                                                         const float* __restrict__ table, UnipcCoef c) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= per) return;
    float g = c.guidance, f = 1.f;
    if (GM == 2) { g = table[2 * blockIdx.y]; f = table[2 * blockIdx.y + 1]; }
    const long i = (long)blockIdx.y * per + j0;
    const bool read_last = c.corr && c.cl != 0.f, read_m1 = (c.corr && c.c1 != 0.f) || c.p1 != 0.f, read_m2 = c.corr && c.c2 != 0.f;
    float xt[V], eu[V], ec[V], xl[V], h1[V], h2[V], m[V], xc[V], xn[V];
    half_t h[V];
    load_f32<V>(x + i, xt);
    load_f16<V>(eps2 + i, eu);
    if (GM != 0) load_f16<V>(eps2 + n + i, ec);
    if (read_last) load_f32<V>(x_last + i, xl);
    if (read_m1) load_f32<V>(m1 + i, h1);
    if (read_m2) load_f32<V>(m2 + i, h2);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        unipc_element<GM>(eu[j], GM != 0 ? ec[j] : 0.f, g, f, xt[j], read_last ? xl[j] : 0.f, read_m1 ? h1[j] : 0.f,
                          read_m2 ? h2[j] : 0.f, c, m[j], xc[j], xn[j]);
        h[j] = twice_rounded_f16(xn[j], c.in_scale);
        if (!read_m1) h1[j] = m[j];
    }
    store_f32<V>(x_last + i, xc);
    store_f32<V>(m2 + i, h1);
    store_f32<V>(m1 + i, m);
    store_f32<V>(x + i, xn);
    store_f16<V>(model_in2 + i, h);
    if (GM != 0) store_f16<V>(model_in2 + n + i, h);
}

template <int GM>
static int launch_unipc(const UnipcArgs& a, hipStream_t stream) {
    const int64_t per = GM == 2 ? a.per : a.n, latents = a.n / per;
    LAVIE_CHECK(latents >= 1 && latents <= 65535 && latents * per == a.n, "unipc step: n=%lld is not 1..65535 latents of per=%lld",
                (long long)a.n, (long long)per);
    const bool vec = per % 8 == 0;
    const int64_t blocks = ((vec ? per / 8 : per) + 255) / 256;
    LAVIE_CHECK(blocks <= 0x7fffffff, "unipc step: per=%lld does not fit one launch", (long long)per);
    auto kern = vec ? unipc_step_kernel<GM, 8> : unipc_step_kernel<GM, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)latents), dim3(256), 0, stream, a.eps, a.x, a.x_last, a.m1, a.m2,
                       a.model_in, (long)a.n, (long)per, a.table, a.c);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_unipc_step(const UnipcArgs& a, hipStream_t stream) {
    if (a.table) return launch_unipc<2>(a, stream);
    return a.cfg ? launch_unipc<1>(a, stream) : launch_unipc<0>(a, stream);
}

}  // namespace lavie
