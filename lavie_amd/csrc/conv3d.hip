// nn.Conv3d for the video ResNet behind lavie_r3d_* (DESIGN.md 7.20), gfx950: implicit GEMM on v_mfma_f32_16x16x32_f16.
//
//  conv3d_kernel       channels-last fp16 rows x [N, T, H, W, Cin] -> y [N, To, Ho, Wo, Cout]; (3,3,3) pad 1 stride 1 | 2, or (1,1,1)
//      stride 2 (the downsample shortcut).  Weights [Cout][kt][kh][kw][Cin]: K = tap-major, channel-minor, in K-tiles of 64 halfs, so
//      a K-tile is 128 contiguous bytes of ONE tap of every row.  A tap outside the volume stages zeros.
//  conv3d_stem_kernel  the (3,7,7) stride (1,2,2) pad (1,3,3) conv over 3 channels.  Reads the pixels in place, fp16 or fp32, through
//      element strides of the clip, frame and channel axes (rows contiguous), so both the frames-major planar layout the
//      preprocessor writes and a channels-first [N, 3, T, H, W] tensor are read without a transpose pass.  K = 147 taps x 3
//      channels = 441, zero-padded to 448 = 7 K-tiles (the pad columns stage zeros against zero weights).
//  Both: ONE tile geometry, 64 output rows x 64 channels per 256-thread workgroup, each of the 4 waves a 32 x 32 quarter (2 x 2
//  MFMA tiles), fp32 accumulation in the matrix pipe over the K-tiles in ascending order, no split-K, no atomics: an output element
//  is one fixed-order sum whatever the batch size, the clip's position or the grid.  Staging: global -> registers -> LDS, two
//  stages, one barrier per K-tile; the loads of K-tile k + 1 are in flight under the MFMAs of K-tile k.  LDS rows are 128 B with the
//  family's XOR swizzle (16-byte piece p of row r sits at piece p ^ (r & 7)): the fragment reads of 16 rows x 4 pieces spread
//  over all banks.  Epilogue, written with scalar fp32 operations: v = acc + bias (the folded BatchNorm shift); v += residual;
//  v = max(v, 0); ONE rounding to fp16.
//
//  mean_rows           fp16 [N, rows, C] -> fp32 [N, C] (AdaptiveAvgPool3d(1) of channels-last rows): four sequential fp32 partials
//      per (clip, channel) (rows r = g, g + 4, ...), summed (p0 + p1) + (p2 + p3), one division by rows.  No atomics.
#include <limits.h>

#include "ops.h"

namespace lavie {

namespace {

constexpr int C3_BM = 64, C3_BN = 64, C3_THREADS = 256;
constexpr int C3_STAGE = (C3_BM + C3_BN) * 128;      // activations rows then weight rows, 128 B each

struct Conv3dGeo {
    int Ti, Hi, Wi, To, Ho, Wo;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
    int Cin, Cout, M, nk, ldw;
    int relu;
};

// one K-tile from LDS stage `sm` into the wave's 2 x 2 accumulators: acc[nt][mt][r] = channel wn 32 + nt 16 + 4 (lane >> 4) + r of
// row wm 32 + mt 16 + (lane & 15)
__device__ __forceinline__ void c3_mma(const char* sm, int wm, int wn, int lane, f32x4 (&acc)[2][2]) {
    const int r = lane & 15, fg = lane >> 4, fsw = lane & 7;
    const char* abase = sm + (wm * 32 + r) * 128;
    const char* wbase = sm + C3_BM * 128 + (wn * 32 + r) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int slot = ((ks * 4 + fg) ^ fsw) * 16;
        half8_t af[2], wf[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) af[mt] = *reinterpret_cast<const half8_t*>(abase + mt * 16 * 128 + slot);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) wf[nt] = *reinterpret_cast<const half8_t*>(wbase + nt * 16 * 128 + slot);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt], af[mt], acc[nt][mt], 0, 0, 0);
    }
}

__device__ __forceinline__ void c3_store_piece(char* sm, int row, int piece, half8_t v) {
    *reinterpret_cast<half8_t*>(sm + row * 128 + ((piece ^ (row & 7)) * 16)) = v;
}

__device__ __forceinline__ void c3_epilogue(const f32x4 (&acc)[2][2], const float* __restrict__ bias, const half_t* __restrict__ R,
                                            half_t* __restrict__ y, int m0, int n0, int wm, int wn, int lane, int M, int Cout, int relu) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + wm * 32 + mt * 16 + (lane & 15);
        if (m >= M) continue;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = n0 + wn * 32 + nt * 16 + (lane >> 4) * 4;
            const size_t at = (size_t)m * Cout + n;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[nt][mt][r] + bias[n + r];
            if (R) {
                const half4_t rv = *reinterpret_cast<const half4_t*>(R + at);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] + (float)rv[r];
            }
            if (relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
            const half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *reinterpret_cast<half4_t*>(y + at) = o;
        }
    }
}

// the two weight pieces of a thread for K-tile k: rows (tid >> 3) and (tid >> 3) + 32 of the column tile, piece tid & 7
__device__ __forceinline__ void c3_load_w(const half_t* __restrict__ w, int ldw, int n0, int k, int tid, half8_t (&wv)[2]) {
    const half_t* p = w + (size_t)(n0 + (tid >> 3)) * ldw + (size_t)k * 64 + (tid & 7) * 8;
    wv[0] = *reinterpret_cast<const half8_t*>(p);
    wv[1] = *reinterpret_cast<const half8_t*>(p + (size_t)32 * ldw);
}

__global__ __launch_bounds__(C3_THREADS) void conv3d_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w,
                                                           const float* __restrict__ bias, const half_t* __restrict__ R,
                                                           half_t* __restrict__ y, Conv3dGeo g) {
    __shared__ __attribute__((aligned(16))) char smem[2 * C3_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * C3_BM, n0 = blockIdx.y * C3_BN;
    const int piece = tid & 7;
    // the two activation rows this thread stages: their clip and the input coordinates of tap (0, 0, 0)
    int t0[2], h0[2], w0[2];
    size_t clip[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m0 + (tid >> 3) + 32 * i;
        m = m < g.M ? m : g.M - 1;                 // a ragged last tile stages its last row again; the epilogue drops it
        const int wo = m % g.Wo;
        int q = m / g.Wo;
        const int ho = q % g.Ho;
        q /= g.Ho;
        const int to = q % g.To;
        clip[i] = (size_t)(q / g.To) * g.Ti;
        t0[i] = to * g.st - g.pt;
        h0[i] = ho * g.sh - g.ph;
        w0[i] = wo * g.sw - g.pw;
    }
    const int chunks = g.Cin >> 6;
    int dt = 0, dh = 0, dw = 0, ch = 0;            // tap and 64-channel chunk of the K-tile the next load fetches
    const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8_t av[2], wv[2];
    auto load = [&](int k) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ti = t0[i] + dt, hi = h0[i] + dh, wi = w0[i] + dw;
            const bool ok = (unsigned)ti < (unsigned)g.Ti && (unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi;
            const size_t pix = ((clip[i] + (size_t)ti) * g.Hi + (size_t)hi) * g.Wi + (size_t)wi;
            const half_t* p = x + (ok ? pix * g.Cin : (size_t)0) + ch * 64 + piece * 8;      // clamped address, value dropped
            const half8_t v = *reinterpret_cast<const half8_t*>(p);
            av[i] = ok ? v : zero8;
        }
        c3_load_w(w, g.ldw, n0, k, tid, wv);
        if (++ch == chunks) {
            ch = 0;
            if (++dw == g.kw) {
                dw = 0;
                if (++dh == g.kh) { dh = 0; ++dt; }
            }
        }
    };
    auto store = [&](char* sm) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            c3_store_piece(sm, (tid >> 3) + 32 * i, piece, av[i]);
            c3_store_piece(sm + C3_BM * 128, (tid >> 3) + 32 * i, piece, wv[i]);
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    load(0);
    store(smem);
    __syncthreads();
    for (int k = 0; k < g.nk; ++k) {
        const bool more = k + 1 < g.nk;
        if (more) load(k + 1);
        c3_mma(smem + (k & 1) * C3_STAGE, wm, wn, lane, acc);
        if (more) store(smem + ((k + 1) & 1) * C3_STAGE);
        __syncthreads();
    }
    c3_epilogue(acc, bias, R, y, m0, n0, wm, wn, lane, g.M, g.Cout, g.relu);
}

constexpr int STEM_KT = 3, STEM_KH = 7, STEM_KW = 7, STEM_CIN = 3, STEM_COUT = 64;
constexpr int STEM_K = STEM_KT * STEM_KH * STEM_KW * STEM_CIN;      // 441
constexpr int STEM_KPAD = (STEM_K + 63) / 64 * 64;                   // 448

template <typename TIN>
__global__ __launch_bounds__(C3_THREADS) void conv3d_stem_kernel(const TIN* __restrict__ x, long long sn, long long sf, long long sc,
                                                                const half_t* __restrict__ w, const float* __restrict__ bias,
                                                                half_t* __restrict__ y, Conv3dGeo g) {
    __shared__ __attribute__((aligned(16))) char smem[2 * C3_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * C3_BM;
    // activations: this thread stages pieces `wave` and `wave + 4` of row `lane` (neighbouring lanes = neighbouring output pixels: the
    // element loads of one k coalesce); the k of a piece is the same in every lane of a wave
    int m = m0 + lane;
    m = m < g.M ? m : g.M - 1;
    const int wo = m % g.Wo;
    int q = m / g.Wo;
    const int ho = q % g.Ho;
    q /= g.Ho;
    const int to = q % g.To;
    const TIN* xn = x + (size_t)(q / g.To) * sn;
    const int t0 = to * g.st - g.pt, h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
    half8_t av[2], wv[2];
    auto load = [&](int k) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int kk0 = k * 64 + (wave + 4 * i) * 8;
            half8_t v;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = kk0 + j;
                const int tap = kk / STEM_CIN, c = kk - tap * STEM_CIN;
                const int dt = tap / (STEM_KH * STEM_KW), rem = tap - dt * (STEM_KH * STEM_KW);
                const int dh = rem / STEM_KW, dw = rem - dh * STEM_KW;
                const int ti = t0 + dt, hi = h0 + dh, wi = w0 + dw;
                const bool ok = kk < STEM_K && (unsigned)ti < (unsigned)g.Ti && (unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi;
                const size_t at = ok ? (size_t)ti * sf + (size_t)c * sc + (size_t)hi * g.Wi + (size_t)wi : (size_t)0;
                const TIN e = xn[at];
                v[j] = ok ? (half_t)e : (half_t)0.f;
            }
            av[i] = v;
        }
        c3_load_w(w, STEM_KPAD, 0, k, tid, wv);
    };
    auto store = [&](char* sm) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            c3_store_piece(sm, lane, wave + 4 * i, av[i]);
            c3_store_piece(sm + C3_BM * 128, (tid >> 3) + 32 * i, tid & 7, wv[i]);
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int NK = STEM_KPAD / 64;
    load(0);
    store(smem);
    __syncthreads();
    for (int k = 0; k < NK; ++k) {
        const bool more = k + 1 < NK;
        if (more) load(k + 1);
        c3_mma(smem + (k & 1) * C3_STAGE, wm, wn, lane, acc);
        if (more) store(smem + ((k + 1) & 1) * C3_STAGE);
        __syncthreads();
    }
    c3_epilogue(acc, bias, nullptr, y, m0, 0, wm, wn, lane, g.M, STEM_COUT, g.relu);
}

// w [Cout][Cin][taps] (nn.Conv3d's [Cout, Cin, kt, kh, kw]) -> out [Cout][kpad], k = tap * Cin + ci, zero behind taps * Cin.
// With bn = (gamma, beta, running_mean, running_var) the BatchNorm that follows the conv is folded in: scale = gamma / sqrt(var + eps)
// in double, out = fp16(w * scale) (one rounding), shift[co] = fp32(beta - mean * scale).
template <typename TW>
__global__ void conv3d_pack_kernel(const TW* __restrict__ w, half_t* __restrict__ out, int Cout, int Cin, int taps, int kpad,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                                   const float* __restrict__ var, double eps, float* __restrict__ shift) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Cout * kpad) return;
    const int co = (int)(i / kpad), k = (int)(i - (long)co * kpad);
    double scale = 1.0;
    if (gamma) {
        scale = (double)gamma[co] / sqrt((double)var[co] + eps);
        if (k == 0) shift[co] = (float)((double)beta[co] - (double)mean[co] * scale);
    }
    half_t v = (half_t)0.f;
    if (k < taps * Cin) {
        const int tap = k / Cin, ci = k - tap * Cin;
        v = (half_t)((double)w[((size_t)co * Cin + ci) * taps + tap] * scale);
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void mean_rows_kernel(const half_t* __restrict__ x, float* __restrict__ out, int rows, int C) {
    __shared__ float part[4][64];
    const int l = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int n = blockIdx.y, c = blockIdx.x * 64 + l;
    float s = 0.f;
    if (c < C) {
        const half_t* p = x + (size_t)n * rows * C + c;
        for (int r = grp; r < rows; r += 4) s += (float)p[(size_t)r * C];
    }
    part[grp][l] = s;
    __syncthreads();
    if (grp == 0 && c < C) out[(size_t)n * C + c] = ((part[0][l] + part[1][l]) + (part[2][l] + part[3][l])) / (float)rows;
}

bool r3d_width(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

int out_extent(int n, int s) { return (n - 1) / s + 1; }

}  // namespace

long long conv3d_packed_halfs(int Cout, int Cin, int kt, int kh, int kw) {
    if (Cout < 1 || Cin < 1 || kt < 1 || kh < 1 || kw < 1 || kt > 7 || kh > 7 || kw > 7 || Cin > 4096 || Cout > 4096) return -1;
    const long long k = (long long)kt * kh * kw * Cin;
    return (long long)Cout * ((k + 63) / 64 * 64);
}

static int pack_launch(const void* w, bool w_f32, half_t* out, int Cout, int Cin, int kt, int kh, int kw, const float* gamma,
                       const float* beta, const float* mean, const float* var, double eps, float* shift, hipStream_t stream) {
    const long long total = conv3d_packed_halfs(Cout, Cin, kt, kh, kw);
    LAVIE_CHECK(total > 0, "conv3d_pack: bad shape Cout=%d Cin=%d kernel (%d,%d,%d)", Cout, Cin, kt, kh, kw);
    LAVIE_CHECK(w && out, "conv3d_pack: null tensor");
    const int taps = kt * kh * kw, kpad = (int)(total / Cout);
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (w_f32)
        hipLaunchKernelGGL(conv3d_pack_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)w, out, Cout, Cin, taps, kpad, gamma,
                           beta, mean, var, eps, shift);
    else
        hipLaunchKernelGGL(conv3d_pack_kernel<half_t>, dim3(grid), dim3(256), 0, stream, (const half_t*)w, out, Cout, Cin, taps, kpad, gamma,
                           beta, mean, var, eps, shift);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_conv3d_pack(const half_t* w, half_t* out, int Cout, int Cin, int kt, int kh, int kw, hipStream_t stream) {
    return pack_launch(w, false, out, Cout, Cin, kt, kh, kw, nullptr, nullptr, nullptr, nullptr, 0.0, nullptr, stream);
}

int launch_conv3d_fold_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, double eps,
                            half_t* out, float* shift, int Cout, int Cin, int kt, int kh, int kw, hipStream_t stream) {
    LAVIE_CHECK(gamma && beta && mean && var && shift, "conv3d_fold_pack: null BatchNorm tensor");
    return pack_launch(w, true, out, Cout, Cin, kt, kh, kw, gamma, beta, mean, var, eps, shift, stream);
}

int conv3d_out_shape(int T, int H, int W, int ksize, int stride, int* To, int* Ho, int* Wo) {
    LAVIE_CHECK((ksize == 3 && (stride == 1 || stride == 2)) || (ksize == 1 && stride == 2),
                "conv3d: kernel (%d,%d,%d) stride %d is not built: (3,3,3) pad 1 stride 1 | 2 and (1,1,1) stride 2 are", ksize, ksize, ksize,
                stride);
    LAVIE_CHECK(T >= 1 && H >= 1 && W >= 1, "conv3d: extents T=%d H=%d W=%d must be at least 1", T, H, W);
    *To = out_extent(T, stride);
    *Ho = out_extent(H, stride);
    *Wo = out_extent(W, stride);
    return 0;
}

int launch_conv3d(const half_t* x, const half_t* wp, const float* bias, const half_t* R, bool relu, half_t* y, int N, int T, int H, int W,
                  int Cin, int Cout, int ksize, int stride, hipStream_t stream) {
    LAVIE_CHECK(x && wp && bias && y, "conv3d: null tensor");
    LAVIE_CHECK(r3d_width(Cin) && r3d_width(Cout), "conv3d: Cin=%d Cout=%d must each be 64, 128, 256 or 512", Cin, Cout);
    LAVIE_CHECK(N >= 1, "conv3d: N=%d must be at least 1", N);
    Conv3dGeo g;
    if (int rc = conv3d_out_shape(T, H, W, ksize, stride, &g.To, &g.Ho, &g.Wo)) return rc;
    const long long rows_in = (long long)N * T * H * W, rows_out = (long long)N * g.To * g.Ho * g.Wo;
    LAVIE_CHECK(rows_in <= INT_MAX - C3_BM, "conv3d: N T H W = %lld input rows exceed the 32-bit row index", rows_in);
    g.Ti = T; g.Hi = H; g.Wi = W;
    g.kt = g.kh = g.kw = ksize;
    g.st = g.sh = g.sw = stride;
    g.pt = g.ph = g.pw = ksize == 3 ? 1 : 0;
    g.Cin = Cin; g.Cout = Cout;
    g.M = (int)rows_out;
    g.nk = ksize * ksize * ksize * (Cin / 64);
    g.ldw = g.nk * 64;
    g.relu = relu ? 1 : 0;
    const dim3 grid((unsigned)cdiv(g.M, C3_BM), (unsigned)(Cout / C3_BN));
    hipLaunchKernelGGL(conv3d_kernel, grid, dim3(C3_THREADS), 0, stream, x, wp, bias, R, y, g);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int conv3d_stem_out_shape(int T, int H, int W, int* To, int* Ho, int* Wo) {
    LAVIE_CHECK(T >= 1 && H >= 1 && W >= 1, "conv3d_stem: extents T=%d H=%d W=%d must be at least 1", T, H, W);
    *To = T;
    *Ho = out_extent(H, 2);
    *Wo = out_extent(W, 2);
    return 0;
}

int launch_conv3d_stem(const void* px, bool px_f32, long long stride_n, long long stride_t, long long stride_c, const half_t* wp,
                       const float* bias, bool relu, half_t* y, int N, int T, int H, int W, hipStream_t stream) {
    LAVIE_CHECK(px && wp && bias && y, "conv3d_stem: null tensor");
    LAVIE_CHECK(N >= 1, "conv3d_stem: N=%d must be at least 1", N);
    Conv3dGeo g;
    if (int rc = conv3d_stem_out_shape(T, H, W, &g.To, &g.Ho, &g.Wo)) return rc;
    const long long plane = (long long)H * W;
    LAVIE_CHECK(stride_c >= plane && stride_t >= plane && stride_n >= plane,
                "conv3d_stem: strides (clip %lld, frame %lld, channel %lld) must each hold one H x W = %lld plane", stride_n, stride_t,
                stride_c, plane);
    const long long rows_out = (long long)N * g.To * g.Ho * g.Wo;
    LAVIE_CHECK(rows_out <= INT_MAX - C3_BM, "conv3d_stem: N T Ho Wo = %lld output rows exceed the 32-bit row index", rows_out);
    g.Ti = T; g.Hi = H; g.Wi = W;
    g.kt = STEM_KT; g.kh = STEM_KH; g.kw = STEM_KW;
    g.st = 1; g.sh = 2; g.sw = 2;
    g.pt = 1; g.ph = 3; g.pw = 3;
    g.Cin = STEM_CIN; g.Cout = STEM_COUT;
    g.M = (int)rows_out;
    g.nk = STEM_KPAD / 64;
    g.ldw = STEM_KPAD;
    g.relu = relu ? 1 : 0;
    const dim3 grid((unsigned)cdiv(g.M, C3_BM));
    if (px_f32)
        hipLaunchKernelGGL(conv3d_stem_kernel<float>, grid, dim3(C3_THREADS), 0, stream, (const float*)px, stride_n, stride_t, stride_c, wp,
                           bias, y, g);
    else
        hipLaunchKernelGGL(conv3d_stem_kernel<half_t>, grid, dim3(C3_THREADS), 0, stream, (const half_t*)px, stride_n, stride_t, stride_c, wp,
                           bias, y, g);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_mean_rows(const half_t* x, float* out, int N, int rows, int C, hipStream_t stream) {
    LAVIE_CHECK(x && out, "mean_rows: null tensor");
    LAVIE_CHECK(N >= 1 && N <= 65535 && rows >= 1 && C >= 1, "mean_rows: N=%d (1..65535) rows=%d C=%d must be at least 1", N, rows, C);
    hipLaunchKernelGGL(mean_rows_kernel, dim3((unsigned)cdiv(C, 64), (unsigned)N), dim3(256), 0, stream, x, out, rows, C);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
