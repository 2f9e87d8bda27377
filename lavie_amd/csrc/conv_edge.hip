// The narrow ends of a convolutional autoencoder (AutoencoderKL: 3 / 4 / 8 channels on one side, 128 - 512 on the other), gfx950.
// The implicit GEMM needs multiples of 64 channels on both sides and channels-last rows on both sides; these two kernels sit where
// one side is an NCHW image of at most 8 channels:
//
//  conv_edge_in   NCHW fp16 / fp32 [N, Cin <= 8, H, W]  ->  channels-last fp16 rows [N H W, Cout], 3x3, pad 1.
//      K = 9 Cin <= 72 per output: vector ALU (v_dot2_f32_f16 over channel pairs), weights in LDS, one thread per (pixel, 8 output
//      channels) as the UNet engine's conv_in_kernel; a workgroup stages the weights once and walks a grid-stride list of items.  The
//      image is read in place in its own dtype (fp32 values are rounded to fp16 on the way into the dot product); an odd Cin is a
//      guarded read against a zero weight.  `tap_bias` [9][Cout] is added for the taps that fall INSIDE the image: a 1x1 conv in
//      front of this conv folds into the weights, and its bias, which the unfused pair sees only through the in-image taps (the
//      zero padding comes after the 1x1 conv), becomes such a per-tap bias.
//
//  conv_edge_out  channels-last fp16 rows [N H W, Cin]  ->  NCHW fp16 / fp32 [N, Cout <= 8, H, W], 3x3, pad 1.
//      The matrix pipe with the output channels as the rows of the 16-row A operand (rows Cout .. 15 are zeros) and 16 consecutive
//      pixels as the columns of B: lane l supplies B[k = 8 (l >> 4) + j][pixel l & 15], which is 16 contiguous bytes of that pixel's
//      row at the tap's offset, so the activation operand goes from global memory straight into the MFMA with no LDS staging and no
//      transposition.  9 taps x ceil(Cin / 32) v_mfma_f32_16x16x32_f16 per 16 pixels, one accumulator (fp32), fixed order: tap
//      major, channel block minor.  The weights live in LDS in fragment order (8 real rows per step; lanes of the zero rows read a
//      zero block); a workgroup stages them once and its four waves walk a contiguous run of tiles.  The result leaves in the
//      accumulator layout (lane = pixel, registers = 4 consecutive output channels): 64-byte runs per channel plane, in the
//      caller's dtype.  No atomics, no cross-lane reduction: two calls give the same bits.
#include "ops.h"
#include "profile.h"

namespace lavie {

// ------------------------------------------------------------------ conv_edge_in
constexpr int EDGE_MAXC = 8;
constexpr int EDGE_IN_MAX_WG = 4096;

template <typename TIN>
__global__ __launch_bounds__(256) void conv_edge_in_kernel(const TIN* __restrict__ x, const half_t* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ tap_bias,
                                                          half_t* __restrict__ y, int N, int Cin, int H, int W, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Cp = (Cin + 1) & ~1;                               // channel pairs: an odd Cin is padded with a zero-weight channel
    half_t* sw = reinterpret_cast<half_t*>(smem);                // [(tap * Cp + ci) / 2][Cout][2]
    float* stb = reinterpret_cast<float*>(sw + 9 * Cp * Cout);   // [9][Cout] (tap_bias only)
    for (int i = threadIdx.x * 8; i < 9 * Cp * Cout; i += 256 * 8)
        *reinterpret_cast<half8_t*>(sw + i) = *reinterpret_cast<const half8_t*>(wp + i);
    if (tap_bias)
        for (int i = threadIdx.x; i < 9 * Cout; i += 256) stb[i] = tap_bias[i];
    __syncthreads();
    const int ng = Cout >> 3;
    const long M = (long)N * H * W;
    const long total = M * ng;
    const size_t plane = (size_t)H * W;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long m = idx / ng;
        const int g = (int)(idx - m * ng);
        const int xw = (int)(m % W);
        const int yh = (int)((m / W) % H);
        const long n = m / ((long)W * H);
        const TIN* xn = x + (size_t)n * Cin * plane;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = bias ? bias[g * 8 + j] : 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = yh + ky - 1;
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = xw + kx - 1;
                if ((unsigned)ix >= (unsigned)W) continue;
                const int tap = ky * 3 + kx;
                if (tap_bias) {
                    const float* tb = stb + tap * Cout + g * 8;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += tb[j];
                }
                const TIN* px = xn + (size_t)iy * W + ix;
                for (int ci = 0; ci < Cp; ci += 2) {
                    const half_t v0 = (half_t)px[(size_t)ci * plane];
                    const half_t v1 = ci + 1 < Cin ? (half_t)px[(size_t)(ci + 1) * plane] : (half_t)0.f;
                    const half2_t v = {v0, v1};
                    const half_t* wr = sw + ((size_t)((tap * Cp + ci) >> 1) * Cout + g * 8) * 2;
                    const half8_t w0 = *reinterpret_cast<const half8_t*>(wr);
                    const half8_t w1 = *reinterpret_cast<const half8_t*>(wr + 8);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[j] = __builtin_amdgcn_fdot2(v, (half2_t){w0[2 * j], w0[2 * j + 1]}, acc[j], false);
                        acc[j + 4] = __builtin_amdgcn_fdot2(v, (half2_t){w1[2 * j], w1[2 * j + 1]}, acc[j + 4], false);
                    }
                }
            }
        }
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)acc[j];
        *reinterpret_cast<half8_t*>(y + m * Cout + g * 8) = o;
    }
}

// [Cout][Cin][3][3] -> [(tap * Cp + ci) / 2][Cout][2], Cp = Cin rounded up to even, the pad channel's weights zero
__global__ void pack_conv_edge_in_kernel(const half_t* __restrict__ w, half_t* __restrict__ out, int Cout, int Cin) {
    const int Cp = (Cin + 1) & ~1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * Cp * Cout) return;
    const int e = i & 1, co = (i >> 1) % Cout, kp = (i >> 1) / Cout;
    const int k = kp * 2 + e, tap = k / Cp, ci = k - tap * Cp;
    out[i] = ci < Cin ? w[((size_t)co * Cin + ci) * 9 + tap] : (half_t)0.f;
}

int launch_pack_conv_edge_in(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream) {
    LAVIE_CHECK(Cin >= 1 && Cin <= EDGE_MAXC, "pack_conv_edge_in: Cin=%d must be 1 .. %d", Cin, EDGE_MAXC);
    LAVIE_CHECK(Cout >= 8 && Cout % 8 == 0, "pack_conv_edge_in: Cout=%d must be a multiple of 8", Cout);
    const int total = 9 * ((Cin + 1) & ~1) * Cout;
    hipLaunchKernelGGL(pack_conv_edge_in_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, w, out, Cout, Cin);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_conv_edge_in(const void* x, bool x_f32, const half_t* wp, const float* bias, const float* tap_bias, half_t* y, int N, int Cin,
                        int H, int W, int Cout, hipStream_t stream) {
    LAVIE_CHECK(Cin >= 1 && Cin <= EDGE_MAXC, "conv_edge_in: Cin=%d must be 1 .. %d", Cin, EDGE_MAXC);
    LAVIE_CHECK(Cout >= 8 && Cout % 8 == 0, "conv_edge_in: Cout=%d must be a multiple of 8", Cout);
    LAVIE_CHECK(N >= 1 && H >= 1 && W >= 1 && (long long)N * H * W * Cout < (1ll << 40), "conv_edge_in: bad shape N=%d %dx%d", N, H, W);
    const int Cp = (Cin + 1) & ~1;
    const size_t lds = (size_t)9 * Cp * Cout * sizeof(half_t) + (tap_bias ? (size_t)9 * Cout * sizeof(float) : 0);
    LAVIE_CHECK(lds <= 128 * 1024, "conv_edge_in: weights do not fit LDS (%zu B: Cin=%d Cout=%d)", lds, Cin, Cout);
    const void* kern = x_f32 ? (const void*)conv_edge_in_kernel<float> : (const void*)conv_edge_in_kernel<half_t>;
    if (int rc = ensure_dynamic_lds(kern, (int)lds)) return rc;
    const long total = (long)N * H * W * (Cout / 8);
    const long wgs = (total + 255) / 256;
    const unsigned grid = (unsigned)(wgs < EDGE_IN_MAX_WG ? wgs : EDGE_IN_MAX_WG);
    ProfileScope prof(KC_CONV3X3, stream, 2.0 * N * H * W * (double)Cout * 9.0 * Cin,
                      (double)N * H * W * (Cin * (x_f32 ? 4.0 : 2.0) + 2.0 * Cout));
    if (x_f32)
        hipLaunchKernelGGL(conv_edge_in_kernel<float>, dim3(grid), dim3(256), lds, stream, (const float*)x, wp, bias, tap_bias, y, N, Cin,
                           H, W, Cout);
    else
        hipLaunchKernelGGL(conv_edge_in_kernel<half_t>, dim3(grid), dim3(256), lds, stream, (const half_t*)x, wp, bias, tap_bias, y, N,
                           Cin, H, W, Cout);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ conv_edge_out
constexpr int EDGE_OUT_TILE = 16;          // pixels per wave tile = columns of the MFMA
constexpr int EDGE_OUT_MAX_WG = 2048;
constexpr int EDGE_OUT_STEP_HALFS = 256;   // one K step of the weight image: [4 k-quads][8 rows][8 halfs]

__host__ __device__ static inline int edge_out_ncb(int Cin) { return (Cin + 31) / 32; }

// NCB > 0: ceil(Cin / 32) known at compile time (the taps' loads are issued one tap ahead of their MFMAs); 0: any Cin % 8 == 0
template <int NCB, typename TOUT>
__global__ __launch_bounds__(256) void conv_edge_out_kernel(const half_t* __restrict__ x, const half_t* __restrict__ wp,
                                                           const float* __restrict__ bias, TOUT* __restrict__ y, int N, int Cin,
                                                           int H, int W, int Cout, int quads_per_wg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* sw = reinterpret_cast<half_t*>(smem);
    const int ncb = NCB > 0 ? NCB : edge_out_ncb(Cin);
    const int wn = 9 * ncb * EDGE_OUT_STEP_HALFS;
    for (int i = threadIdx.x * 8; i < wn; i += 256 * 8)
        *reinterpret_cast<half8_t*>(sw + i) = *reinterpret_cast<const half8_t*>(wp + i);
    if (threadIdx.x == 0) *reinterpret_cast<half8_t*>(sw + wn) = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};      // the zero rows' fragment
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;                   // B: pixel column, k-quad; A: row = col, k-quad; D: rows 4 kq .. 4 kq + 3
    const bool wrow = col < 8;                                   // lanes of the A operand's real rows
    const half_t* wl = wrow ? sw + (kq * 8 + col) * 8 : sw + wn;
    const int wstep = wrow ? EDGE_OUT_STEP_HALFS : 0;
    const long M = (long)N * H * W;
    const long ntiles = (M + EDGE_OUT_TILE - 1) / EDGE_OUT_TILE;
    const size_t plane = (size_t)H * W;
    const int c_lane = kq * 8;                                   // this lane's first channel inside a 32-channel block
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (bias && kq * 4 + r < Cout) bias4[r] = bias[kq * 4 + r];
    const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    const long q0 = (long)blockIdx.x * quads_per_wg;
    for (int q = 0; q < quads_per_wg; ++q) {
        const long tile = (q0 + q) * 4 + wave;
        if (tile >= ntiles) break;
        const long m_raw = tile * EDGE_OUT_TILE + col;
        const long m = m_raw < M ? m_raw : M - 1;                // a ragged last tile computes its last pixel again and drops it
        const int xw = (int)(m % W);
        const int yh = (int)((m / W) % H);
        const long n = m / ((long)W * H);
        const half_t* xm = x + (size_t)m * Cin + c_lane;
        f32x4 acc = bias4;
        if constexpr (NCB > 0) {
            half8_t b[2][NCB];
            auto load_tap = [&](int tap, half8_t* dst) {
                const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                const bool ok = (unsigned)(yh + dy) < (unsigned)H && (unsigned)(xw + dx) < (unsigned)W;
                const half_t* src = ok ? xm + ((long)dy * W + dx) * Cin : xm;     // clamped address, value dropped: no divergent load
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const half8_t v = *reinterpret_cast<const half8_t*>(src + cb * 32);
                    dst[cb] = ok ? v : zero8;
                }
            };
            load_tap(0, b[0]);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                if (tap < 8) load_tap(tap + 1, b[(tap + 1) & 1]);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const half8_t a = *reinterpret_cast<const half8_t*>(wl + (tap * NCB + cb) * wstep);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[tap & 1][cb], acc, 0, 0, 0);
                }
            }
        } else {
            for (int tap = 0; tap < 9; ++tap) {
                const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                const bool ok = (unsigned)(yh + dy) < (unsigned)H && (unsigned)(xw + dx) < (unsigned)W;
                const half_t* src = ok ? xm + ((long)dy * W + dx) * Cin : xm;
                for (int cb = 0; cb < ncb; ++cb) {
                    const bool have = ok && cb * 32 + c_lane < Cin;              // a last block of fewer than 32 channels
                    const half8_t v = *reinterpret_cast<const half8_t*>(have ? src + cb * 32 : xm - c_lane);
                    const half8_t a = *reinterpret_cast<const half8_t*>(wl + (tap * ncb + cb) * wstep);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, have ? v : zero8, acc, 0, 0, 0);
                }
            }
        }
        if (m_raw < M) {
            TOUT* dst = y + ((size_t)n * Cout + kq * 4) * plane + (size_t)yh * W + xw;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kq * 4 + r < Cout) dst[r * plane] = (TOUT)acc[r];
        }
    }
}

// [Cout][Cin][3][3] -> [tap * ncb + cb][k-quad][row 0..7][8 halfs]: element j of (step, kq, row) = w[row][cb * 32 + kq * 8 + j][tap],
// zero for row >= Cout or a channel >= Cin
__global__ void pack_conv_edge_out_kernel(const half_t* __restrict__ w, half_t* __restrict__ out, int Cout, int Cin) {
    const int ncb = edge_out_ncb(Cin);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * ncb * EDGE_OUT_STEP_HALFS) return;
    const int j = i & 7, row = (i >> 3) & 7, kq = (i >> 6) & 3, step = i >> 8;
    const int tap = step / ncb, cb = step - tap * ncb;
    const int ci = cb * 32 + kq * 8 + j;
    out[i] = (row < Cout && ci < Cin) ? w[((size_t)row * Cin + ci) * 9 + tap] : (half_t)0.f;
}

int launch_pack_conv_edge_out(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream) {
    LAVIE_CHECK(Cout >= 1 && Cout <= EDGE_MAXC, "pack_conv_edge_out: Cout=%d must be 1 .. %d", Cout, EDGE_MAXC);
    LAVIE_CHECK(Cin >= 8 && Cin % 8 == 0, "pack_conv_edge_out: Cin=%d must be a multiple of 8", Cin);
    const int total = 9 * edge_out_ncb(Cin) * EDGE_OUT_STEP_HALFS;
    hipLaunchKernelGGL(pack_conv_edge_out_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, w, out, Cout, Cin);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

long long conv_edge_out_image_halfs(int Cin) { return Cin >= 8 && Cin % 8 == 0 ? 9ll * edge_out_ncb(Cin) * EDGE_OUT_STEP_HALFS : 0; }

template <int NCB, typename TOUT>
static int launch_edge_out(const half_t* x, const half_t* wp, const float* bias, void* y, int N, int Cin, int H, int W, int Cout,
                           hipStream_t stream) {
    auto kern = conv_edge_out_kernel<NCB, TOUT>;
    const int lds = 9 * edge_out_ncb(Cin) * EDGE_OUT_STEP_HALFS * (int)sizeof(half_t) + 16;
    if (int rc = ensure_dynamic_lds((const void*)kern, lds)) return rc;
    const long ntiles = ((long)N * H * W + EDGE_OUT_TILE - 1) / EDGE_OUT_TILE;
    const long quads = (ntiles + 3) / 4;
    const int per = (int)((quads + EDGE_OUT_MAX_WG - 1) / EDGE_OUT_MAX_WG);
    const unsigned grid = (unsigned)((quads + per - 1) / per);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, x, wp, bias, (TOUT*)y, N, Cin, H, W, Cout, per);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_conv_edge_out(const half_t* x, const half_t* wp, const float* bias, void* y, bool y_f32, int N, int Cin, int H, int W, int Cout,
                         hipStream_t stream) {
    LAVIE_CHECK(Cout >= 1 && Cout <= EDGE_MAXC, "conv_edge_out: Cout=%d must be 1 .. %d", Cout, EDGE_MAXC);
    LAVIE_CHECK(Cin >= 8 && Cin % 8 == 0, "conv_edge_out: Cin=%d must be a multiple of 8", Cin);
    LAVIE_CHECK(N >= 1 && H >= 1 && W >= 1 && (long long)N * H * W < (1ll << 31), "conv_edge_out: bad shape N=%d %dx%d", N, H, W);
    LAVIE_CHECK(9 * edge_out_ncb(Cin) * EDGE_OUT_STEP_HALFS * 2 + 16 <= 128 * 1024, "conv_edge_out: Cin=%d weights do not fit LDS", Cin);
    ProfileScope prof(KC_CONV3X3, stream, 2.0 * N * H * W * (double)Cout * 9.0 * Cin,
                      (double)N * H * W * (2.0 * Cin + Cout * (y_f32 ? 4.0 : 2.0)));
    // the widths of the SD autoencoders take the unrolled loop (loads one tap ahead); anything else the rolled, untuned one
    if (Cin == 128)
        return y_f32 ? launch_edge_out<4, float>(x, wp, bias, y, N, Cin, H, W, Cout, stream)
                     : launch_edge_out<4, half_t>(x, wp, bias, y, N, Cin, H, W, Cout, stream);
    if (Cin == 256)
        return y_f32 ? launch_edge_out<8, float>(x, wp, bias, y, N, Cin, H, W, Cout, stream)
                     : launch_edge_out<8, half_t>(x, wp, bias, y, N, Cin, H, W, Cout, stream);
    if (Cin == 512)
        return y_f32 ? launch_edge_out<16, float>(x, wp, bias, y, N, Cin, H, W, Cout, stream)
                     : launch_edge_out<16, half_t>(x, wp, bias, y, N, Cin, H, W, Cout, stream);
    return y_f32 ? launch_edge_out<0, float>(x, wp, bias, y, N, Cin, H, W, Cout, stream)
                 : launch_edge_out<0, half_t>(x, wp, bias, y, N, Cin, H, W, Cout, stream);
}

}  // namespace lavie
