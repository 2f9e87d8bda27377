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
// returns xk whatever the model predicted.  Contraction is off and every fused multiply-add is spelled out (sampler_element.h, shared
// with sampler_window.hip): the compiler cannot move a rounding point.
//
// Launch shape: blockIdx.y = the (video, channel) plane, blockIdx.x * 256 + lane = the position inside the plane, so the mask
// index needs one scalar division per block and none per lane.  HBM-bound: with inner % 8 == 0 every lane takes eight elements
// with 16-byte accesses (an 8-group cannot straddle a plane, one 32-byte mask read serves it, and n % 8 == 0 keeps the cond
// halves of eps2 / model_in2 aligned); otherwise one element per lane, same arithmetic.  No atomics, no host synchronisation,
// no allocation: capture-safe and bit-reproducible.
#include "common.h"
#include "ops.h"
#include "sampler_element.h"

namespace lavie {

__device__ __forceinline__ float known_select(float m, float free_v, float pinned_v) {
#pragma clang fp contract(off)
    return m == 0.f ? free_v : m == 1.f ? pinned_v : __builtin_fmaf(m, pinned_v - free_v, free_v);
}

// FAM 0: five-coefficient family (aux = the step's noise, read when c4 != 0); FAM 1: multistep family (aux = x0_prev, read when
// HIST, always written); FAM 2: the start blend (no eps, xm = x; CFG = write the model input twice).  W = elements per lane.
// TAB: the latent's guidance scale and rescale factor come from table[latent] = (g, f) (sampler_guidance.hip) and eps = f e;
// `table` is the LAST kernel argument, so the forms without it keep their argument offsets and their instruction text.
template <int FAM, bool CFG, bool HIST, int W, bool TAB = false>
__global__ __launch_bounds__(256) void known_step_kernel(const half_t* __restrict__ eps2, float* __restrict__ x,
                                                         float* __restrict__ aux, half_t* __restrict__ model_in2, long n,
                                                         int channels, long inner, StepCoef c, KnownOperands k, float in_scale,
                                                         const float* __restrict__ table) {
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * W;
    if (j0 >= inner) return;
    const long i = (long)blockIdx.y * inner + j0;                       // element in [P, C, inner]
    const long mi = (long)(blockIdx.y / (unsigned)channels) * inner + j0;     // its mask element in [P, 1, inner]
    float xt[W], eu[W], ec[W], ax[W], kn[W], nk[W], m[W], xn[W], hist[W];
    half_t h[W];
    float g = 0.f, f = 0.f;
    if constexpr (TAB) {
        const unsigned p = blockIdx.y / (unsigned)channels;
        g = table[2 * p];
        f = table[2 * p + 1];
    }
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
        if constexpr (TAB) {
            const float eps = scaled_guided_eps(eu[j], ec[j], g, f);
            if (FAM == 0) xm = five_coefficient_from_eps(eps, xt[j], c.c4 != 0.f ? ax[j] : 0.f, c);
            else multistep_from_eps<HIST>(eps, xt[j], HIST ? ax[j] : 0.f, c, x0, xm);
        } else if (FAM == 0) xm = five_coefficient_element<CFG>(eu[j], CFG ? ec[j] : 0.f, xt[j], c.c4 != 0.f ? ax[j] : 0.f, c);
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

template <int FAM, bool CFG, bool HIST, bool TAB = false>
static int launch_known(const StepArgs& a, hipStream_t stream) {
    const int64_t planes = a.n / a.inner;
    LAVIE_CHECK(planes >= 1 && planes <= 65535, "known-region step: %lld (video, channel) planes do not fit one launch",
                (long long)planes);
    const bool vec = a.inner % 8 == 0;
    const int64_t blocks = ((vec ? a.inner / 8 : a.inner) + 255) / 256;
    LAVIE_CHECK(blocks <= 0x7fffffff, "known-region step: inner=%lld does not fit one launch", (long long)a.inner);
    auto kern = vec ? known_step_kernel<FAM, CFG, HIST, 8, TAB> : known_step_kernel<FAM, CFG, HIST, 1, TAB>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)planes), dim3(256), 0, stream, a.eps, a.x, a.aux, a.model_in, (long)a.n,
                       a.channels, (long)a.inner, a.c, *a.known, a.in_scale, a.table);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

// the instantiation of a step: the family, guidance (a table is guided by definition), and for the multistep family whether the
// history is read
int launch_step_known(const StepArgs& a, hipStream_t stream) {
    const bool hist = a.c.c4 != 0.f;
    if (!a.multistep) {
        if (a.table) return launch_known<0, true, false, true>(a, stream);
        return a.cfg ? launch_known<0, true, false>(a, stream) : launch_known<0, false, false>(a, stream);
    }
    if (a.table) return hist ? launch_known<1, true, true, true>(a, stream) : launch_known<1, true, false, true>(a, stream);
    if (a.cfg) return hist ? launch_known<1, true, true>(a, stream) : launch_known<1, true, false>(a, stream);
    return hist ? launch_known<1, false, true>(a, stream) : launch_known<1, false, false>(a, stream);
}

int launch_known_blend(float* x, half_t* model_in, bool dup, int64_t n, float in_scale, const float* known, const float* mask,
                       const float* noise_known, int channels, int64_t inner, float a_next, float s_next, hipStream_t stream) {
    const KnownOperands k{known, mask, noise_known, a_next, s_next};
    StepArgs a{};                   // no eps, no aux, no table, coefficients zero
    a.x = x; a.model_in = model_in; a.n = n; a.in_scale = in_scale;
    a.known = &k; a.channels = channels; a.inner = inner;
    return dup ? launch_known<2, true, false>(a, stream) : launch_known<2, false, false>(a, stream);
}

}  // namespace lavie
