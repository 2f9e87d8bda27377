// FreeInit's frequency mix (Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion Models"; diffusers' FreeInitMixin):
//   d     = a x0 + s e0 - r z                                 fp32, formed as the first pass loads: z_T never exists in memory
//   out   = r z + Re IFFT3( filter .* FFT3(d) )               over (F, H, W) of every image [F, H, W]; filter real, FFT-native order
//   model_in[j] = fp16(out in_scale), j < dup                 rounded once, as lavie_latents_to_scaled_model_input1 rounds it
// The host hands in the EVEN part of the low-pass filter, for which the inverse transform of a real d is real: no
// pass computes an imaginary output that would be thrown away, and the last pass forms real parts only.
//
// Six launches, a separable DIRECT DFT in fp32: forward along W (real -> complex), H, F (times the filter as it stores), inverse
// along F, H, W (complex -> real, + r z, the fp16 copies).  Axis lengths are any integers, F <= 256, H, W <= 128: at these lengths
// a direct sum is a few hundred fused multiply-adds per element, far below a millisecond of VALU work, and needs no radix structure.
// Intermediates are complex fp32 in two halves of the caller's workspace (2 x 8 bytes per element), ping-pong.
//
// Twiddles: per axis one table of N (cos, sin)(2 pi j / N) pairs, computed in fp64 on the host, rounded once to fp32, handed to the
// kernel as a launch argument (2 KiB) and copied to LDS; term (k, n) reads entry (k n) mod N, kept as a running INDEX (idx += k,
// minus N on overflow): no angle is accumulated and no device sine or cosine runs.
//
// Tiles and LDS.  Workgroups of 256 threads; a tile is N x 32: the whole axis times 32 contiguous columns (H and F passes: a row of the
// tile is 32 complex values = 256 contiguous bytes of global memory) or 32 contiguous lines (W passes: the tile is 32 N contiguous
// elements, transposed through LDS on the way in and on the way out, so both directions of global traffic are unit-stride).  In LDS the
// 32 lanes of a half wave hold one term index n and 32 consecutive columns: 8-byte reads of 32 consecutive values cover the 64 banks
// once.  The transposed W tiles have a row pitch of 33 values: 33 4-byte words (real) step one bank per line, 33 8-byte values step
// two banks, so the transposing stores and loads are conflict-free as well.  A lane owns one column and the outputs k = g, g + 8, ...
// (g = its group of 32 lanes), two at a time so that a value read from LDS serves two outputs; the two half waves of a wave read two
// twiddle addresses each (broadcast).  LDS per workgroup: H / F passes N (256 + 8) bytes (67.6 KiB at F = 256: 2 workgroups per CU, 10.6 KiB at H = 40: the
// 8-workgroup cap), W passes N (33 x 12 + 8) bytes (51.7 KiB at W = 128: 3 per CU, 25.9 KiB at W = 64: 6 per CU).  The kernels use
// under 64 registers, so LDS alone sets the occupancy; the grids are small (80 to 320 workgroups at the base shape), the op is
// latency-bound.
//
// Determinism: every output is summed by one lane in one fixed order (eight accumulators taking n mod 8 in ascending n, folded as a
// balanced tree; dft_pair) with spelled-out fmas (contraction off); no atomics; a tile never spans two images' columns of the F pass or two outer indices, and its arithmetic does not depend on
// where the tile lies, so two calls agree bit for bit and image j of a batch has the bits of its single-image call.
// Rounding points of an output element: d (three roundings), each pass's sums, the filter product, and fma(sum, 1 / (F H W), r z).
// Built without packed fp32 (Makefile, NOPK_FLAGS).  No allocation, no synchronisation: capturable.
#include <math.h>

#include "common.h"
#include "ops.h"
#include "sampler_element.h"

namespace lavie {

namespace {

constexpr int kCols = 32;           // columns (or lines) of a tile
constexpr int kGroups = 8;          // groups of 32 lanes in a workgroup of 256
constexpr int kPitch = 33;          // row pitch of a transposed W tile, in values
constexpr int kAcc = 8;             // accumulators per sum

struct Twiddle {                    // (cos, sin)(2 pi j / N), j < N, rounded from fp64; a launch argument
    float c[kFreqMixMaxF];
    float s[kFreqMixMaxF];
};
static_assert(sizeof(Twiddle) == 2048, "the twiddle table travels as a kernel argument");

// the table into LDS as (cos, sign sin): sign = -1 forward, +1 inverse
__device__ __forceinline__ void stage_twiddle(float2* tw, const Twiddle& t, int N, float sign) {
    for (int j = threadIdx.x; j < N; j += 256) tw[j] = make_float2(t.c[j], sign * t.s[j]);
}

// One term of a sum into accumulator pair (re, im): acc += v w, the multiply-adds spelled out.  REAL_IN: v is real; REAL_OUT: only the
// real part is formed.
template <bool REAL_IN, bool REAL_OUT>
__device__ __forceinline__ void term(float& re, float& im, float2 v, float2 w) {
#pragma clang fp contract(off)
    re = __builtin_fmaf(v.x, w.x, re);
    if constexpr (!REAL_IN) re = __builtin_fmaf(-v.y, w.y, re);
    if constexpr (!REAL_OUT) {
        im = __builtin_fmaf(v.x, w.y, im);
        if constexpr (!REAL_IN) im = __builtin_fmaf(v.y, w.x, im);
    }
}

__device__ __forceinline__ float fold(const float (&a)[kAcc]) {
#pragma clang fp contract(off)
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// Outputs k0 and k0 + kGroups of one column of a tile (pitch in values; real values when REAL_IN, else complex).  The order of every
// sum is fixed: accumulator q takes the terms n = q, q + 8, q + 16, ... in ascending order and the eight are folded as a balanced
// tree.  Eight short chains instead of one long one: the rounding error of a straight fp32 sum grows with the chain's length
// (DESIGN.md 7.15), and the chains are independent, which also hides the fma latency.
template <bool REAL_IN, bool REAL_OUT>
__device__ __forceinline__ void dft_pair(const void* tile, int pitch, int col, const float2* tw, int N, int k0, float2& o0, float2& o1) {
    const int k1 = k0 + kGroups < N ? k0 + kGroups : k0;       // past the end: a harmless repeat of k0, never stored
    float r0[kAcc], i0[kAcc], r1[kAcc], i1[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; ++q) r0[q] = i0[q] = r1[q] = i1[q] = 0.f;
    int j0 = 0, j1 = 0;
    auto step = [&](int n, int q) {
        float2 v;
        if constexpr (REAL_IN) v = make_float2(static_cast<const float*>(tile)[n * pitch + col], 0.f);
        else v = static_cast<const float2*>(tile)[n * pitch + col];
        term<REAL_IN, REAL_OUT>(r0[q], i0[q], v, tw[j0]);
        term<REAL_IN, REAL_OUT>(r1[q], i1[q], v, tw[j1]);
        j0 += k0; if (j0 >= N) j0 -= N;
        j1 += k1; if (j1 >= N) j1 -= N;
    };
    int n = 0;
    for (; n + kAcc <= N; n += kAcc) {
#pragma unroll
        for (int q = 0; q < kAcc; ++q) step(n + q, q);
    }
#pragma unroll
    for (int q = 0; q < kAcc - 1; ++q)
        if (n + q < N) step(n + q, q);
    o0 = make_float2(fold(r0), REAL_OUT ? 0.f : fold(i0));
    o1 = make_float2(fold(r1), REAL_OUT ? 0.f : fold(i1));
}

// ---- H and F passes: complex -> complex along an axis of length N with `inner` contiguous columns behind it.
// Element (o, n, c) of [outer, N, inner] lies at (o N + n) inner + c.  FILTER: the stored value is multiplied by filter[k inner + c]
// (the F pass: N = F, inner = H W, one filter for all images).
template <bool FILTER>
__global__ __launch_bounds__(256) void freq_axis_kernel(const float2* __restrict__ in, float2* __restrict__ out,
                                                        const float* __restrict__ filter, Twiddle t, int N, long inner, int tiles,
                                                        float sign) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float2* tw = reinterpret_cast<float2*>(lds_raw);
    float2* tile = tw + N;
    const long o = blockIdx.x / tiles;
    const long c = (long)(blockIdx.x % tiles) * kCols + (threadIdx.x & 31);
    const int col = threadIdx.x & 31, g = threadIdx.x >> 5;
    const long base = o * N * inner + c;
    stage_twiddle(tw, t, N, sign);
    if (c < inner)
        for (int n = g; n < N; n += kGroups) tile[n * kCols + col] = in[base + n * inner];
    __syncthreads();
    if (c >= inner) return;
    for (int k0 = g; k0 < N; k0 += 2 * kGroups) {
        float2 a, b;
        dft_pair<false, false>(tile, kCols, col, tw, N, k0, a, b);
        if constexpr (FILTER) {
#pragma clang fp contract(off)
            const float f0 = filter[k0 * inner + c];
            a.x *= f0; a.y *= f0;
        }
        out[base + k0 * inner] = a;
        if (k0 + kGroups < N) {
            if constexpr (FILTER) {
#pragma clang fp contract(off)
                const float f1 = filter[(k0 + kGroups) * inner + c];
                b.x *= f1; b.y *= f1;
            }
            out[base + (k0 + kGroups) * inner] = b;
        }
    }
}

// ---- W forward: 32 lines of N contiguous reals, d = a x0 + s e0 - r z formed at the load, -> complex.
__global__ __launch_bounds__(256) void freq_w_forward_kernel(const float* __restrict__ x0, const float* __restrict__ e0,
                                                             const float* __restrict__ z, float a, float s, float r,
                                                             float2* __restrict__ out, Twiddle t, int N, long lines) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float2* tw = reinterpret_cast<float2*>(lds_raw);
    float2* tout = tw + N;                                          // [N][kPitch] complex
    float* tin = reinterpret_cast<float*>(tout + N * kPitch);       // [N][kPitch] real
    const long l0 = (long)blockIdx.x * kCols;
    const int nl = lines - l0 < kCols ? (int)(lines - l0) : kCols;
    const long g0 = l0 * N;
    const int col = threadIdx.x & 31, g = threadIdx.x >> 5;
    stage_twiddle(tw, t, N, -1.f);
    for (int i = threadIdx.x; i < nl * N; i += 256) {
#pragma clang fp contract(off)
        const int line = i / N, n = i - line * N;
        const float rz = r * z[g0 + i];
        tin[n * kPitch + line] = __builtin_fmaf(a, x0[g0 + i], __builtin_fmaf(s, e0[g0 + i], -rz));
    }
    __syncthreads();
    if (col < nl)
        for (int k0 = g; k0 < N; k0 += 2 * kGroups) {
            float2 a, b;
            dft_pair<true, false>(tin, kPitch, col, tw, N, k0, a, b);
            tout[k0 * kPitch + col] = a;
            if (k0 + kGroups < N) tout[(k0 + kGroups) * kPitch + col] = b;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < nl * N; i += 256) {
        const int line = i / N, k = i - line * N;
        out[g0 + i] = tout[k * kPitch + line];
    }
}

// ---- W inverse: 32 lines of N contiguous complex values -> the real part, out = fma(sum, 1 / (F H W), r z) and its fp16 copies.
__global__ __launch_bounds__(256) void freq_w_inverse_kernel(const float2* __restrict__ in, const float* __restrict__ z, float r,
                                                             float inv_count, float* __restrict__ out, half_t* __restrict__ model_in,
                                                             int dup, long dup_stride, float in_scale, Twiddle t, int N, long lines) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float2* tw = reinterpret_cast<float2*>(lds_raw);
    float2* tin = tw + N;                                           // [N][kPitch] complex
    float* tout = reinterpret_cast<float*>(tin + N * kPitch);       // [N][kPitch] real
    const long l0 = (long)blockIdx.x * kCols;
    const int nl = lines - l0 < kCols ? (int)(lines - l0) : kCols;
    const long g0 = l0 * N;
    const int col = threadIdx.x & 31, g = threadIdx.x >> 5;
    stage_twiddle(tw, t, N, 1.f);
    for (int i = threadIdx.x; i < nl * N; i += 256) {
        const int line = i / N, n = i - line * N;
        tin[n * kPitch + line] = in[g0 + i];
    }
    __syncthreads();
    if (col < nl)
        for (int k0 = g; k0 < N; k0 += 2 * kGroups) {
            float2 a, b;
            dft_pair<false, true>(tin, kPitch, col, tw, N, k0, a, b);
            tout[k0 * kPitch + col] = a.x;
            if (k0 + kGroups < N) tout[(k0 + kGroups) * kPitch + col] = b.x;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < nl * N; i += 256) {
#pragma clang fp contract(off)
        const int line = i / N, k = i - line * N;
        const float rz = r * z[g0 + i];
        const float v = __builtin_fmaf(tout[k * kPitch + line], inv_count, rz);
        out[g0 + i] = v;
        if (model_in) {
            const half_t h = once_rounded_f16(v, in_scale);
            for (int j = 0; j < dup; ++j) model_in[j * dup_stride + g0 + i] = h;
        }
    }
}

Twiddle make_twiddle(int N) {
    Twiddle t{};
    for (int j = 0; j < N; ++j) {
        const double ang = 2.0 * M_PI * (double)j / (double)N;
        t.c[j] = (float)cos(ang);
        t.s[j] = (float)sin(ang);
    }
    return t;
}

template <bool FILTER>
int launch_axis(const float2* in, float2* out, const float* filter, int N, int64_t outer, int64_t inner, float sign, hipStream_t stream) {
    const int64_t tiles = (inner + kCols - 1) / kCols;
    LAVIE_CHECK(outer * tiles <= 0x7fffffff, "freq_mix: %lld tiles do not fit one launch", (long long)(outer * tiles));
    const int lds = N * (kCols + 1) * (int)sizeof(float2);
    auto kern = freq_axis_kernel<FILTER>;
    if (int rc = ensure_dynamic_lds((const void*)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(outer * tiles)), dim3(256), lds, stream, in, out, filter, make_twiddle(N), N, (long)inner,
                       (int)tiles, sign);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace

bool freq_mix_supported(int images, int F, int H, int W) {
    return images >= 1 && images <= kFreqMixMaxImages && F >= 1 && F <= kFreqMixMaxF && H >= 1 && H <= kFreqMixMaxHW && W >= 1 &&
           W <= kFreqMixMaxHW;
}

size_t freq_mix_workspace_floats(int images, int F, int H, int W) {
    return freq_mix_supported(images, F, H, W) ? (size_t)4 * images * F * H * W : 0;      // two complex fp32 buffers
}

int launch_freq_mix(const FreqMixParams& p, hipStream_t stream) {
    LAVIE_CHECK(freq_mix_supported(p.images, p.F, p.H, p.W), "freq_mix: images=%d F=%d H=%d W=%d is out of range", p.images, p.F, p.H, p.W);
    const int64_t count = (int64_t)p.F * p.H * p.W, total = count * p.images, lines = (int64_t)p.images * p.F * p.H;
    float2* A = reinterpret_cast<float2*>(p.workspace);
    float2* B = A + total;
    const int64_t wblocks = (lines + kCols - 1) / kCols;
    const int wlds = p.W * ((int)sizeof(float2) + kPitch * (int)(sizeof(float2) + sizeof(float)));
    if (int rc = ensure_dynamic_lds((const void*)freq_w_forward_kernel, wlds)) return rc;
    if (int rc = ensure_dynamic_lds((const void*)freq_w_inverse_kernel, wlds)) return rc;
    hipLaunchKernelGGL(freq_w_forward_kernel, dim3((unsigned)wblocks), dim3(256), wlds, stream, p.x0, p.e0, p.z, p.a, p.s, p.r, A,
                       make_twiddle(p.W), p.W, (long)lines);
    LAVIE_HIP(hipGetLastError());
    if (int rc = launch_axis<false>(A, B, nullptr, p.H, (int64_t)p.images * p.F, p.W, -1.f, stream)) return rc;
    if (int rc = launch_axis<true>(B, A, p.filter, p.F, p.images, (int64_t)p.H * p.W, -1.f, stream)) return rc;
    if (int rc = launch_axis<false>(A, B, nullptr, p.F, p.images, (int64_t)p.H * p.W, 1.f, stream)) return rc;
    if (int rc = launch_axis<false>(B, A, nullptr, p.H, (int64_t)p.images * p.F, p.W, 1.f, stream)) return rc;
    hipLaunchKernelGGL(freq_w_inverse_kernel, dim3((unsigned)wblocks), dim3(256), wlds, stream, A, p.z, p.r, (float)(1.0 / (double)count),
                       p.out, p.model_in, p.dup, (long)p.dup_stride, p.in_scale, make_twiddle(p.W), p.W, (long)lines);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
