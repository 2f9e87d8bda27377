// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; diffusers' apply_freeu / fourier_filter) on the two operands of a decoder
// concat, both channels-last row matrices: h [(n y x), C_h] gets its first C_h / 2 channels scaled by b, the skip [(n y x), C2] gets the
// 2 x 2 block around the centre of its shifted 2-D spectrum scaled by s, per image n and channel.  That block is the set of modes
// ky in {0, -1 mod H} x kx in {0, -1 mod W} (one mode at 1 x 1, two at 1 x W or H x 1, four otherwise), so no FFT runs:
//   out(y, x) = in(y, x) + (s - 1) / (H W) * sum_k [cos phi_k(y, x) A_k + sin phi_k(y, x) B_k],  phi_k = 2 pi (y / H [ky] + x / W [kx]),
//   A_k = sum in cos phi_k,  B_k = sum in sin phi_k        (the sign of phi drops out: it enters sin on both sides)
// Seven fp32 sums per (image, channel): A of the constant mode, (A, B) of the x, y and xy modes.
//
// Two LDS-light streaming kernels, lanes across channels with 16-byte loads:
//   sums:  a workgroup owns (64 channels, one run of pixel slabs, one image): 8 channel lanes x 32 pixel lanes, a slab = 32 pixels, one
//          per pixel lane.  Each thread adds its pixel of slab after slab in ascending order into 7 x 8 registers; the 32 pixel lanes
//          are then folded in a fixed order (8 sequential adds, then 4) through 9 KB of LDS and stored as one partial per run.  The run
//          geometry (freeu_geom) depends on H and W alone, so an image's sums do not depend on the images around it.  No atomics.
//   apply: one launch over both tensors.  A skip thread owns 8 channels of 16 consecutive pixels: it folds the runs' partials of its
//          channels in ascending order, then forms in + correction in fp32 and rounds once to fp16.  An h thread owns 8 channels of one
//          row: fp16(b * in) below C_h / 2; above it the bits are copied (out of place) or not touched (in place).
// Trigonometry is sincospif of 2 y / H and 2 x / W on the device: nothing is tabulated, a call has no state.
#include "ops.h"

namespace lavie {

namespace {
constexpr int kChanLanes = 8;                       // x 8 channels = the 64-channel tile of a sums workgroup
constexpr int kTileC = kChanLanes * 8;
constexpr int kApplyPixels = 16;                    // pixels a skip thread of the apply kernel walks
}

FreeuGeom freeu_geom(int H, int W) {
    FreeuGeom g;
    g.P = H * W;
    g.nslabs = cdiv(g.P, kFreeuSlab);
    const int spw = cdiv(g.nslabs, kFreeuMaxRuns);
    g.slabs_per_run = spw > kFreeuMinRunSlabs ? spw : kFreeuMinRunSlabs;
    g.runs = cdiv(g.nslabs, g.slabs_per_run);
    return g;
}

size_t freeu_workspace_floats(int C2, int NI, int H, int W) {
    return (size_t)NI * freeu_geom(H, W).runs * kFreeuSums * C2;
}

// cos / sin of the x, y and xy modes at pixel (y, x); a mode the image does not have (W == 1: x, H == 1: y) comes out as the constant one
struct FreeuTrig { float cx, sx, cy, sy, cxy, sxy; };
__device__ __forceinline__ FreeuTrig freeu_trig(int y, int x, float fh, float fw) {
    FreeuTrig t;
    sincospif((float)(2 * y) / fh, &t.sy, &t.cy);   // the angle in units of pi, 2 y / H in [0, 2): one rounding (the quotient)
    sincospif((float)(2 * x) / fw, &t.sx, &t.cx);
    t.cxy = t.cy * t.cx - t.sy * t.sx;
    t.sxy = t.sy * t.cx + t.cy * t.sx;
    return t;
}

__global__ __launch_bounds__(256) void freeu_sums_kernel(const half_t* __restrict__ skip, float* __restrict__ part, int C2, int H, int W,
                                                         int nslabs, int slabs_per_run) {
    __shared__ float red[kFreeuSlab][kTileC];
    __shared__ float red2[4][kTileC];
    const int tid = threadIdx.x;
    const int cl = tid & (kChanLanes - 1), py = tid / kChanLanes;
    const int c = blockIdx.x * kTileC + cl * 8;
    const int run = blockIdx.y, runs = gridDim.y, n = blockIdx.z;
    const int P = H * W;
    const float fh = (float)H, fw = (float)W;
    const half_t* img = skip + (size_t)n * P * C2;
    float acc[kFreeuSums][8];
#pragma unroll
    for (int m = 0; m < kFreeuSums; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[m][j] = 0.f;
    const int slab0 = run * slabs_per_run, slab1 = min(nslabs, slab0 + slabs_per_run);
    if (c < C2) {                                   // C2 % 8 == 0: the 8 channels are all in or all out
        for (int sl = slab0; sl < slab1; ++sl) {
            const int p = sl * kFreeuSlab + py;
            if (p >= P) break;                      // the ragged last slab
            const int y = p / W, x = p - y * W;
            const FreeuTrig t = freeu_trig(y, x, fh, fw);
            const half8_t v8 = *(const half8_t*)(img + (size_t)p * C2 + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)v8[j];
                acc[0][j] += v;
                acc[1][j] = fmaf(v, t.cx, acc[1][j]);
                acc[2][j] = fmaf(v, t.sx, acc[2][j]);
                acc[3][j] = fmaf(v, t.cy, acc[3][j]);
                acc[4][j] = fmaf(v, t.sy, acc[4][j]);
                acc[5][j] = fmaf(v, t.cxy, acc[5][j]);
                acc[6][j] = fmaf(v, t.sxy, acc[6][j]);
            }
        }
    }
    // the 32 pixel lanes of each channel, in a fixed order: lanes 8 q .. 8 q + 7 one after the other, then q = 0 .. 3
    const int cc = tid & (kTileC - 1), q = tid / kTileC;
    float* out = part + ((size_t)n * runs + run) * kFreeuSums * C2;
#pragma unroll
    for (int m = 0; m < kFreeuSums; ++m) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[py][cl * 8 + j] = acc[m][j];
        __syncthreads();
        float t = red[q * 8][cc];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += red[q * 8 + i][cc];
        red2[q][cc] = t;
        __syncthreads();                            // (red is rewritten behind this barrier, red2 behind the next one)
        if (tid < kTileC && blockIdx.x * kTileC + cc < C2)
            out[(size_t)m * C2 + blockIdx.x * kTileC + cc] = ((red2[0][cc] + red2[1][cc]) + red2[2][cc]) + red2[3][cc];
    }
}

// fp16_rne of a FINISHED fp32 value (lora.hip round_f16: keeps hipcc from fusing the last fp32 operation with the conversion)
__device__ __forceinline__ half_t freeu_round_f16(float v) {
    asm volatile("" : "+v"(v));
    return (half_t)v;
}

// skip_mode: 0 = the skip is not touched, 1 = copied, 2 = filtered; h: its first h_cols channels are walked (0, C_h / 2 in place, C_h).  Items [0, skip_items) are skip threads
// (channel octet fastest, then pixel group, then image), the rest h threads (channel octet fastest over h_cols channels, then row).
__global__ __launch_bounds__(256) void freeu_apply_kernel(const half_t* skip, half_t* skip_out, const float* __restrict__ part, int C2, int H,
                                                          int W, int runs, float gain, int skip_mode, long long skip_items,
                                                          const half_t* h, half_t* h_out, int C_h, int h_cols, float b,
                                                          long long items) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= items) return;
    if (id < skip_items) {
        const int octs = C2 / 8, P = H * W, groups = cdiv(P, kApplyPixels);
        const int c = (int)(id % octs) * 8;
        const int pg = (int)((id / octs) % groups), n = (int)(id / ((long long)octs * groups));
        const int p0 = pg * kApplyPixels, p1 = min(P, p0 + kApplyPixels);
        const half_t* src = skip + ((size_t)n * P) * C2 + c;
        half_t* dst = skip_out + ((size_t)n * P) * C2 + c;
        if (skip_mode == 1) {
            for (int p = p0; p < p1; ++p) *(half8_t*)(dst + (size_t)p * C2) = *(const half8_t*)(src + (size_t)p * C2);
            return;
        }
        float sum[kFreeuSums][8];                    // the runs' partials in ascending order, then the gain (s - 1) / (H W)
#pragma unroll
        for (int m = 0; m < kFreeuSums; ++m)
#pragma unroll
            for (int j = 0; j < 8; ++j) sum[m][j] = 0.f;
        for (int r = 0; r < runs; ++r) {
            const float* pr = part + ((size_t)n * runs + r) * kFreeuSums * C2 + c;
#pragma unroll
            for (int m = 0; m < kFreeuSums; ++m) {
                const f32x4 a = *(const f32x4*)(pr + (size_t)m * C2), bb = *(const f32x4*)(pr + (size_t)m * C2 + 4);
                sum[m][0] += a.x; sum[m][1] += a.y; sum[m][2] += a.z; sum[m][3] += a.w;
                sum[m][4] += bb.x; sum[m][5] += bb.y; sum[m][6] += bb.z; sum[m][7] += bb.w;
            }
        }
        const float gx = W > 1 ? gain : 0.f, gy = H > 1 ? gain : 0.f, gxy = W > 1 && H > 1 ? gain : 0.f;   // the mode SET: no mode twice
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sum[0][j] *= gain;
            sum[1][j] *= gx; sum[2][j] *= gx;
            sum[3][j] *= gy; sum[4][j] *= gy;
            sum[5][j] *= gxy; sum[6][j] *= gxy;
        }
        const float fh = (float)H, fw = (float)W;
        for (int p = p0; p < p1; ++p) {
            const int y = p / W, x = p - y * W;
            const FreeuTrig t = freeu_trig(y, x, fh, fw);
            const half8_t v8 = *(const half8_t*)(src + (size_t)p * C2);
            half8_t o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float corr = sum[0][j];
                corr = fmaf(t.cx, sum[1][j], corr);
                corr = fmaf(t.sx, sum[2][j], corr);
                corr = fmaf(t.cy, sum[3][j], corr);
                corr = fmaf(t.sy, sum[4][j], corr);
                corr = fmaf(t.cxy, sum[5][j], corr);
                corr = fmaf(t.sxy, sum[6][j], corr);
                o[j] = freeu_round_f16((float)v8[j] + corr);      // the one rounding to fp16
            }
            *(half8_t*)(dst + (size_t)p * C2) = o;
        }
        return;
    }
    const long long e = id - skip_items;
    const int octs = h_cols / 8;
    const int c = (int)(e % octs) * 8;
    const size_t off = (size_t)(e / octs) * C_h + c;
    const half8_t v8 = *(const half8_t*)(h + off);
    half8_t o = v8;
    if (c < C_h / 2 && b != 1.0f) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = freeu_round_f16(b * (float)v8[j]);
    }
    *(half8_t*)(h_out + off) = o;
}

int launch_freeu(const half_t* h, int C_h, const half_t* skip, int C2, int NI, int H, int W, float b, float s, half_t* h_out,
                 half_t* skip_out, float* workspace, hipStream_t stream) {
    LAVIE_CHECK(h && skip && h_out && skip_out, "freeu: null tensor");
    LAVIE_CHECK(NI >= 1 && NI <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= (1 << 24), "freeu: NI=%d (1..65535) H=%d W=%d unsupported", NI, H, W);
    LAVIE_CHECK(C_h >= 16 && C_h % 16 == 0, "freeu: C_h=%d must be a positive multiple of 16 (its scaled half is walked in 8-channel vectors)", C_h);
    LAVIE_CHECK(C2 >= 8 && C2 % 8 == 0, "freeu: C2=%d must be a positive multiple of 8", C2);
    LAVIE_CHECK(__builtin_isfinite(b) && __builtin_isfinite(s) && b > 0.f && s > 0.f, "freeu: b=%g s=%g must be finite and > 0", (double)b, (double)s);
    LAVIE_CHECK(((uintptr_t)h | (uintptr_t)skip | (uintptr_t)h_out | (uintptr_t)skip_out | (uintptr_t)workspace) % 16 == 0,
                "freeu: h / skip / h_out / skip_out / workspace must be 16-byte aligned");
    LAVIE_CHECK(s == 1.f || workspace, "freeu: s=%g needs a workspace of lavie_freeu_workspace_bytes()", (double)s);
    const FreeuGeom g = freeu_geom(H, W);
    const int skip_mode = s != 1.f ? 2 : (skip_out != skip ? 1 : 0);
    const int h_cols = h_out != h ? C_h : (b != 1.f ? C_h / 2 : 0);       // in place: only the scaled half is walked
    const long long skip_items = skip_mode ? (long long)NI * cdiv(g.P, kApplyPixels) * (C2 / 8) : 0;
    const long long items = skip_items + (long long)NI * g.P * (h_cols / 8);
    LAVIE_CHECK(items / 256 < (1ll << 31) - 1, "freeu: %lld work items exceed one grid", items);
    if (skip_mode == 2) {
        hipLaunchKernelGGL(freeu_sums_kernel, dim3(cdiv(C2, kTileC), g.runs, NI), dim3(256), 0, stream, skip, workspace, C2, H, W, g.nslabs,
                           g.slabs_per_run);
        LAVIE_HIP(hipGetLastError());
    }
    if (items > 0) {
        hipLaunchKernelGGL(freeu_apply_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, skip, skip_out, workspace, C2, H, W,
                           g.runs, (s - 1.f) / (float)g.P, skip_mode, skip_items, h, h_out, C_h, h_cols > 0 ? h_cols : 8, b, items);
        LAVIE_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace lavie
