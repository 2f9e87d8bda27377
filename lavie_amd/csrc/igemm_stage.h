// Staging code shared by the implicit-GEMM kernels (DESIGN.md "Shared staging code of the GEMM kernels"):
//   * xcd_chunk: the XCD-contiguous workgroup order (every kernel of the family);
//   * the gather side: source-pixel table fill and the segment-descriptor read (igemm_kernel, igemm_pp_kernel);
//   * the ping-pong side, namespace pp: tile geometry, wave roles, fragment reads, MFMA block, phase barrier
//     (igemm_pp_kernel, igemm_ppx_kernel).
// Everything is __forceinline__ and takes the kernels' register arrays by reference: the kernels compile to what they were
// with this text written out in each of them.
#pragma once
#include "igemm.h"

namespace lavie {

// Workgroup (or tile) ids are dealt round-robin to the 8 XCDs; id -> its place in an order in which the ids of one XCD are
// contiguous (chunk sizes n / 8, the first n % 8 chunks one longer).  Bijective on [0, n) for any n.
__device__ __forceinline__ int xcd_chunk(int id, int n) {
    const int q = n >> 3, r = n & 7, xcd = id & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

__device__ __forceinline__ int to_sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- gather side.  LDS behind the stages: tab[rows * 9] source pixels, then segtab[IGEMM_MAX_SEG][6] segment descriptors.
constexpr int gather_tab_bytes(int rows) { return rows * 9 * 4 + IGEMM_MAX_SEG * 6 * 4; }

// Per-block table of source pixels, tab[row * 9 + tap] = pixel index in the source grid or -1 (out of image).  K order is
// segment > 64-channel chunk > tap: the 9 taps of one channel slab are fetched back to back, so the shifted re-reads of the
// same cache lines hit in L1/L2 instead of going to the fabric.  The caller synchronises.
template <int ROWS, int THREADS>
__device__ __forceinline__ void gather_fill_pixels(const IgemmParams& p, int m0, int tid, int* tab) {
    const int hw = p.Ho * p.Wo;
    const int Hv = p.Hi << p.ups, Wv = p.Wi << p.ups;
    if (p.tframes > 0) {          // temporal taps (IgemmParams::tframes): slot t of row m = the same pixel, t - T/2 frames away (or -1)
        const int T_ = p.seg[0].ntaps;
        for (int idx = tid; idx < ROWS * 9; idx += THREADS) {
            const int row = idx / 9, tap = idx - row * 9;
            int m = m0 + row;
            m = m < p.M ? m : p.M - 1;
            const int ff = (m / p.tpix) % p.tframes + tap - (T_ >> 1);
            tab[idx] = (tap < T_ && (unsigned)ff < (unsigned)p.tframes) ? m + (tap - (T_ >> 1)) * p.tpix : -1;
        }
    } else
    for (int idx = tid; idx < ROWS * 9; idx += THREADS) {
        const int row = idx / 9, tap = idx - row * 9;
        int m = m0 + row;
        m = m < p.M ? m : p.M - 1;
        const int n = m / hw;
        const int rem = m - n * hw;
        const int y = rem / p.Wo, x = rem - y * p.Wo;
        const int iy = y * p.stride + tap / 3 - p.pad_lo, ix = x * p.stride + tap % 3 - p.pad_lo;
        const bool ok = (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
        tab[idx] = ok ? (n * p.Hi + (iy >> p.ups)) * p.Wi + (ix >> p.ups) : -1;
    }
}

// Segment descriptors live in LDS, segtab[IGEMM_MAX_SEG][6] = src lo, src hi, C, c0, nchunks, ntaps (written once by the kernel
// with constant indices, read here with the runtime segment index): a runtime index into the by-value kernel-parameter struct
// would make the compiler copy the whole parameter block to scratch, and scratch loads are vmcnt-counted VMEM — every one of
// them inside the K loop would drain the LDS-DMA pipeline (guide §5, trap (b)).  LDS reads only touch lgkmcnt.
__device__ __forceinline__ IgemmSeg gather_load_seg(const int* segtab, int i) {
    IgemmSeg r;
    const unsigned lo = (unsigned)to_sgpr(segtab[i * 6 + 0]), hi = (unsigned)to_sgpr(segtab[i * 6 + 1]);
    r.src = reinterpret_cast<const half_t*>(((unsigned long long)hi << 32) | lo);
    r.C = to_sgpr(segtab[i * 6 + 2]);
    r.c0 = to_sgpr(segtab[i * 6 + 3]);
    r.nchunks = to_sgpr(segtab[i * 6 + 4]);
    r.ntaps = to_sgpr(segtab[i * 6 + 5]);
    return r;
}

// ---- ping-pong side: the 160-row, 8-wave, two-group tile of igemm_pp.hip (its header describes the schedule)
namespace pp {
constexpr int MT = 5;
constexpr int BM = 160, THREADS = 512;
constexpr int A_BYTES = BM * 128;                       // one A stage: 20,480
constexpr int A_STAGES = 3, W_STAGES = 2;
constexpr int W_BASE = A_STAGES * A_BYTES;              // A stages first, then W stages
// NT = 16-wide column tiles per wave: 5 -> 160x320 block tile (N % 320 == 0),
// 4 -> 160x256 (GEGLU: value / gate tile pairs need an even NT; the power-of-two widths of the VSR UNet)
template <int NT>
struct Geo {
    static constexpr int BN = 4 * NT * 16;
    static constexpr int HALF_ROWS = 2 * NT * 16;       // W rows read by one group
    static constexpr int HALF_PIECES = HALF_ROWS / 8;   // 20 or 16: group 0 stages 16 of each half, group 1 the rest
    static constexpr int W_BYTES = BN * 128;
    static constexpr int STAGE_BYTES = W_BASE + W_STAGES * W_BYTES;    // what follows (gather tables, aux area) starts here
};

// wave -> group (0: leading, 1: trailing; SIMD partners), place in the group, and the wave tile (wm, wn) it computes
struct Roles { int grp, q, wm, wn; };
__device__ __forceinline__ Roles roles(int wave) {
    const int grp = wave >> 2, q = wave & 3;
    return Roles{grp, q, q >> 1, grp * 2 + (q & 1)};
}

// fragment read offsets of a lane (bytes): a = (wm * MT * 16 + (lane & 15)) * 128 inside an A stage, w = W_BASE + (wn * NT * 16 +
// (lane & 15)) * 128 from the start of LDS, swizzle terms fsw = lane & 7, fg = lane >> 4.  The kernels compute them in place.
struct FragOfs { int a, w, fsw, fg; };
template <int NT>
__device__ __forceinline__ void read_frags(const char* smem, const FragOfs& f, int ast, int wst, int ks, half8_t (&af)[MT], half8_t (&wf)[NT]) {
    const char* abase = smem + ast * A_BYTES + f.a;
    const char* wbase = smem + wst * Geo<NT>::W_BYTES + f.w;
    const int slot = ((ks * 4 + f.fg) ^ f.fsw) * 16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const half8_t*>(abase + mt * 16 * 128 + slot);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wf[nt] = *reinterpret_cast<const half8_t*>(wbase + nt * 16 * 128 + slot);
}
template <int NT>
__device__ __forceinline__ void mfma_block(const half8_t (&af)[MT], const half8_t (&wf)[NT], f32x4 (&acc)[NT][MT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt], af[mt], acc[nt][mt], 0, 0, 0);
}
// phase boundary: nothing is scheduled across it
__device__ __forceinline__ void phase_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
}  // namespace pp

}  // namespace lavie
