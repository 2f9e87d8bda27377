// Perturbed-attention guidance (Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance"; diffusers'
// AnimateDiffPAGPipeline) inside the fused step: the plain steps of both families with one more prediction folded into eps.
//
// eps = [negative | prompt | perturbed] (CFG, fp16 [3, n]) or [prompt | perturbed] ([2, n]): the model outputs of one forward whose
// last part ran with the identity attn1 of the selected blocks (engine.cpp, lavie_unet_set_pag).  Per element, fp32, contraction off:
//   e   = CFG ? fma(g, ec - eu, eu) : ec                     guided_eps<true> (sampler_element.h) / the prompt prediction itself
//   eps = s != 0 ? fma(s, ec - ep, e) : e                    s = pag_scale >= 0, uniform: with s == 0 the third part is not read
//   then five_coefficient_from_eps / multistep_from_eps<HIST> unchanged, x <- x' (x0_prev <- x0), and the family's rounding of
//   x' in_scale (once_rounded_f16 / twice_rounded_f16) as ONE value into all three (two) parts of model_in.
// Rounding points in front of the family's own: ec - eu and the fma (CFG), ec - ep and the fma (s != 0): four at most.
// With s == 0 the element is the plain kernel's (tests/test_gpu_pag.py holds the bits); with ep == ec the added term is an exact
// zero, so the values are the plain kernel's.  One kernel, two launch forms: eight elements per lane with 16-byte accesses
// (n % 8 == 0, every part of eps / model_in then 16-byte aligned with its tensor), else one element per lane.  No atomics, no
// allocation, no host synchronisation: capture-safe, and two runs agree bit for bit.
// Not combined with the known-region, window or table (`_scaled`) forms (include/lavie_hip.h).
#include "common.h"
#include "ops.h"
#include "sampler_element.h"

namespace lavie {

template <bool CFG> __device__ __forceinline__ float pag_eps(float eu, float ec, float ep, float guidance, float s) {
#pragma clang fp contract(off)
    const float e = CFG ? guided_eps<true>(eu, ec, guidance) : ec;
    return s != 0.f ? __builtin_fmaf(s, ec - ep, e) : e;
}

// FAM 0: five-coefficient family (aux = the step's noise, read when c4 != 0); FAM 1: multistep family (aux = x0_prev, read when
// HIST, always written).  V = elements per lane.  Parts of eps / model_in: [eu |] ec | ep, n elements each.
template <int FAM, bool CFG, bool HIST, int V>
__global__ __launch_bounds__(256) void pag_step_kernel(const half_t* __restrict__ eps, const half_t* __restrict__ eps_pag,
                                                       float* __restrict__ x, float* __restrict__ aux, half_t* __restrict__ model_in,
                                                       long n, StepCoef c, float s, float in_scale) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;
    float xt[V], eu[V], ec[V], ep[V], ax[V], xn[V], hist[V];
    half_t h[V];
    load_f32<V>(x + i, xt);
    if (CFG) load_f16<V>(eps + i, eu);
    load_f16<V>(eps + (CFG ? n : 0) + i, ec);
    if (s != 0.f) load_f16<V>(eps_pag + i, ep);
    if (FAM == 0 ? c.c4 != 0.f : HIST) load_f32<V>(aux + i, ax);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float e = pag_eps<CFG>(CFG ? eu[j] : 0.f, ec[j], s != 0.f ? ep[j] : 0.f, c.guidance, s);
        if (FAM == 0) xn[j] = five_coefficient_from_eps(e, xt[j], c.c4 != 0.f ? ax[j] : 0.f, c);
        else multistep_from_eps<HIST>(e, xt[j], HIST ? ax[j] : 0.f, c, hist[j], xn[j]);
        h[j] = FAM == 1 ? twice_rounded_f16(xn[j], in_scale) : once_rounded_f16(xn[j], in_scale);
    }
    if (FAM == 1) store_f32<V>(aux + i, hist);
    store_f32<V>(x + i, xn);
    store_f16<V>(model_in + i, h);
    store_f16<V>(model_in + n + i, h);
    if (CFG) store_f16<V>(model_in + 2 * n + i, h);
}

template <int FAM, bool CFG, bool HIST>
static int launch_pag(const StepArgs& a, hipStream_t stream) {
    const bool vec = a.n % 8 == 0;
    const int64_t blocks = ((vec ? a.n / 8 : a.n) + 255) / 256;
    LAVIE_CHECK(blocks >= 1 && blocks <= 0x7fffffff, "pag step: n=%lld does not fit one launch", (long long)a.n);
    auto kern = vec ? pag_step_kernel<FAM, CFG, HIST, 8> : pag_step_kernel<FAM, CFG, HIST, 1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, stream, a.eps, a.eps_pag, a.x, a.aux, a.model_in, (long)a.n, a.c,
                       a.pag_scale, a.in_scale);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

template <bool CFG>
static int launch_pag_family(const StepArgs& a, hipStream_t stream) {
    if (!a.multistep) return launch_pag<0, CFG, false>(a, stream);
    return a.c.c4 != 0.f ? launch_pag<1, CFG, true>(a, stream) : launch_pag<1, CFG, false>(a, stream);
}

int launch_step_pag(const StepArgs& a, hipStream_t stream) {
    return a.cfg ? launch_pag_family<true>(a, stream) : launch_pag_family<false>(a, stream);
}

}  // namespace lavie
