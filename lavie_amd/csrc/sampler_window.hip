// Sampler steps over overlapping frame windows: one latent tensor holds a clip longer than the model's window, the UNet ran on W
// windows of L frames each, and this kernel fuses their noise predictions where they overlap, advances the WHOLE clip by one
// scheduler step and writes every window's next fp16 model input, one launch per denoising step.
//
// Operands:
//   x   [P, C, F, hw] fp32, read and written          aux the same shape: the step's noise (five-coefficient family, read when
//   c4 != 0) or x0_prev (multistep family, read when HIST, always written)
//   per window w (start frame s_w, s_0 < s_1 < ...): eps_w read, model_in_w written, both fp16 [nb, C, L, hw], nb = 2 P under
//   guidance ([negative | prompt]) else P;   profile[L] > 0: the weight of a window's i-th frame
// Starts, profile and the two pointer tables are kernel arguments (WindowTable, 896 bytes): no device-side table exists.
// Per element (p, c, f, j), fp32, over the windows that cover f in ascending window order:
//   e_w = fma(guidance, ec_w - eu_w, eu_w)   (without guidance eu_w)
//   n_w = profile[f - s_w] / S,  S = the covering windows' profile values added in window order
//   eps = fma(n_w, e_w, eps), from 0
//   x', x0 = the family's plain step from eps (sampler_element.h: the rounding points of the plain kernels)
//   model_in_w[half, c, f - s_w, j] = fp16(x' in_scale) for every covering window and both guidance halves, rounded as the
//   family's plain kernel rounds it
// A frame covered once has n_w = p / p = 1 and eps = fma(1, e_w, 0) = e_w: the plain kernel's bits.  The weights depend on the
// (p, c, f) plane only: blockIdx.y = the plane, so they are block-uniform scalars computed once, and no lane divides.
// HBM-bound: with hw % 8 == 0 every lane takes eight elements with 16-byte accesses, otherwise one, same arithmetic.  No atomics,
// no host synchronisation, no allocation: capture-safe and bit-reproducible.
#include "common.h"
#include <type_traits>

#include "ops.h"
#include "philox.h"
#include "sampler_element.h"

namespace lavie {

struct WindowTable {
    const half_t* eps[kWindowMaxWindows];
    half_t* model_in[kWindowMaxWindows];
    int start[kWindowMaxWindows];
    float profile[kWindowMaxLength];
};
static_assert(sizeof(WindowTable) < 1024, "the window table travels as a kernel argument");

struct WindowShape { int P, C, F, W, L; long hw; };

// FAM 0: five-coefficient family; FAM 1: multistep family.  V = elements per lane.
// TAB: e_w = f fma(g, ec_w - eu_w, eu_w) with (g, f) = table[w][p] (sampler_guidance.hip): every window's prediction is rescaled
// from that window's own statistics before the windows are averaged.  The table pointer is a parameter PACK, empty or one
// `const float*`: with the empty pack the kernel's argument list, and with it its instruction text, is what it was without the table
// (an unused trailing pointer moved the scheduling of the argument loads of the guided forms).
// The pack may instead hold one NoiseKey (philox.h; FAM 0 without a table): with c4 != 0 the step's noise is the function of
// philox.h at (seed[p], draw, the element's index in the WHOLE clip [C, F, hw]) and aux is not read.  The windows do not enter the
// index: the step has the bits of window_step fed the materialised clip noise (launch_philox_normal, tests/test_gpu_noise.py).
template <typename T, typename... Ts> struct pack_holds { static constexpr bool value = (std::is_same<T, Ts>::value || ...); };
template <int FAM, bool CFG, bool HIST, int V, typename... Table>
__global__ __launch_bounds__(256) void window_step_kernel(float* __restrict__ x, float* __restrict__ aux, WindowTable t, WindowShape s,
                                                          StepCoef c, float in_scale, Table... table_arg) {
    constexpr bool TAB = pack_holds<const float*, Table...>::value, SEEDED = pack_holds<NoiseKey, Table...>::value;
    static_assert(sizeof...(Table) <= 1 && (!SEEDED || FAM == 0), "nothing, a table or a noise key");
    const float* table = nullptr;
    if constexpr (TAB) table = (table_arg, ...);
    const long j0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= s.hw) return;
    // the plane: all of this is block-uniform
    const int plane = blockIdx.y;
    const int f = plane % s.F, pc = plane / s.F;
    const int ch = pc % s.C, p = pc / s.C;
    // sorted starts and one length: the windows that cover f are consecutive, first .. first + ncov - 1
    int first = 0, ncov = 0;
    float sum = 0.f;
    for (int w = 0; w < s.W; ++w) {
        const int off = f - t.start[w];
        if (off >= 0 && off < s.L) {
            if (ncov == 0) first = w;
            sum += t.profile[off];
            ++ncov;
        }
    }
    const long half_stride = (long)s.P * s.C * s.L * s.hw;       // to the prompt half of a window's buffers
    const long i = (long)plane * s.hw + j0;                       // element in [P, C, F, hw]
    float xt[V], ax[V], eps[V], eu[V], ec[V], xn[V], hist[V];
    half_t h[V];
    load_f32<V>(x + i, xt);
    if constexpr (SEEDED) {
        const NoiseKey& key = (table_arg, ...);
        if (c.c4 != 0.f) philox_normals<V>(key.seed[p], key.draw, (unsigned long long)(((long)ch * s.F + f) * s.hw + j0), ax);
    } else if (FAM == 0 ? c.c4 != 0.f : HIST) load_f32<V>(aux + i, ax);
#pragma unroll
    for (int j = 0; j < V; ++j) eps[j] = 0.f;
    for (int k = 0; k < ncov; ++k) {
        const int w = first + k;
        const float nw = t.profile[f - t.start[w]] / sum;
        const long wi = (((long)p * s.C + ch) * s.L + (f - t.start[w])) * s.hw + j0;       // element in [nb, C, L, hw], first half
        load_f16<V>(t.eps[w] + wi, eu);
        if (CFG) load_f16<V>(t.eps[w] + half_stride + wi, ec);
        float gw = 0.f, fw = 0.f;           // block-uniform: the pair of (window, latent)
        if constexpr (TAB) {
            gw = table[2 * (w * s.P + p)];
            fw = table[2 * (w * s.P + p) + 1];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma clang fp contract(off)
            if constexpr (TAB) eps[j] = __builtin_fmaf(nw, scaled_guided_eps(eu[j], ec[j], gw, fw), eps[j]);
            else eps[j] = __builtin_fmaf(nw, guided_eps<CFG>(eu[j], CFG ? ec[j] : 0.f, c.guidance), eps[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (FAM == 0) xn[j] = five_coefficient_from_eps(eps[j], xt[j], c.c4 != 0.f ? ax[j] : 0.f, c);
        else multistep_from_eps<HIST>(eps[j], xt[j], HIST ? ax[j] : 0.f, c, hist[j], xn[j]);
        h[j] = FAM == 1 ? twice_rounded_f16(xn[j], in_scale) : once_rounded_f16(xn[j], in_scale);
    }
    if (FAM == 1) store_f32<V>(aux + i, hist);
    store_f32<V>(x + i, xn);
    for (int k = 0; k < ncov; ++k) {
        const int w = first + k;
        const long wi = (((long)p * s.C + ch) * s.L + (f - t.start[w])) * s.hw + j0;
        store_f16<V>(t.model_in[w] + wi, h);
        if (CFG) store_f16<V>(t.model_in[w] + half_stride + wi, h);
    }
}

template <int FAM, bool CFG, bool HIST, bool TAB = false, bool SEEDED = false>
static int launch_window(const WindowStepParams& a, hipStream_t stream) {
    const int64_t planes = (int64_t)a.P * a.C * a.F;
    LAVIE_CHECK(planes >= 1 && planes <= 65535, "window step: P C F = %lld (video, channel, frame) planes do not fit one launch",
                (long long)planes);
    const bool vec = a.hw % 8 == 0;
    const int64_t blocks = ((vec ? a.hw / 8 : a.hw) + 255) / 256;
    LAVIE_CHECK(blocks >= 1 && blocks <= 0x7fffffff, "window step: hw=%lld does not fit one launch", (long long)a.hw);
    LAVIE_CHECK(a.W >= 1 && a.W <= kWindowMaxWindows && a.L >= 1 && a.L <= kWindowMaxLength, "window step: W=%d L=%d", a.W, a.L);
    WindowTable t{};
    for (int w = 0; w < a.W; ++w) {
        t.eps[w] = a.eps[w];
        t.model_in[w] = a.model_in[w];
        t.start[w] = a.starts[w];
    }
    for (int i = 0; i < a.L; ++i) t.profile[i] = a.profile[i];
    const WindowShape s{a.P, a.C, a.F, a.W, a.L, (long)a.hw};
    if constexpr (TAB) {
        auto kern = vec ? window_step_kernel<FAM, CFG, HIST, 8, const float*> : window_step_kernel<FAM, CFG, HIST, 1, const float*>;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)planes), dim3(256), 0, stream, a.x, a.aux, t, s, a.c, a.in_scale, a.table);
    } else if constexpr (SEEDED) {
        auto kern = vec ? window_step_kernel<FAM, CFG, HIST, 8, NoiseKey> : window_step_kernel<FAM, CFG, HIST, 1, NoiseKey>;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)planes), dim3(256), 0, stream, a.x, a.aux, t, s, a.c, a.in_scale, *a.key);
    } else {
        auto kern = vec ? window_step_kernel<FAM, CFG, HIST, 8> : window_step_kernel<FAM, CFG, HIST, 1>;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)planes), dim3(256), 0, stream, a.x, a.aux, t, s, a.c, a.in_scale);
    }
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_window_step(const WindowStepParams& a, hipStream_t stream) {
    if (a.key) {
        LAVIE_CHECK(!a.multistep, "window step: the multistep family draws no noise and takes no noise key");
        LAVIE_CHECK(!a.table, "window step: a noise key is not combined with `table` (a guidance table): pass the materialised noise");
        LAVIE_CHECK(a.key->count == a.P && a.key->per == (long long)a.C * a.F * a.hw, "window step: the noise key holds count=%d per=%lld, "
                    "the clip P=%d and C F hw=%lld", a.key->count, a.key->per, a.P, (long long)a.C * a.F * a.hw);
        return a.cfg ? launch_window<0, true, false, false, true>(a, stream) : launch_window<0, false, false, false, true>(a, stream);
    }
    if (a.table) {                  // guided by definition: the table holds the guidance scales
        if (!a.multistep) return launch_window<0, true, false, true>(a, stream);
        return a.c.c4 != 0.f ? launch_window<1, true, true, true>(a, stream) : launch_window<1, true, false, true>(a, stream);
    }
    if (!a.multistep)
        return a.cfg ? launch_window<0, true, false>(a, stream) : launch_window<0, false, false>(a, stream);
    if (a.cfg) return a.c.c4 != 0.f ? launch_window<1, true, true>(a, stream) : launch_window<1, true, false>(a, stream);
    return a.c.c4 != 0.f ? launch_window<1, false, true>(a, stream) : launch_window<1, false, false>(a, stream);
}

}  // namespace lavie
