// Implicit-GEMM on the gfx950 matrix cores: C[M,N] = gather(A)[M,Ktot] * W[N,Ktot]^T (+ epilogue).
//
// One kernel serves every dense contraction of the denoiser: Linear layers and
// 1x1 convs (plain A rows), 3x3 convs with stride 1/2, folded nearest-x2 upsample, two-tensor
// (skip-concat) inputs and a fused 1x1 shortcut (K-segments gathered per output pixel from
// channels-last activations).  Reference ops replaced: `InflatedConv3d.forward` (resnet.py:13-21),
// `nn.Linear` in CrossAttention / FeedForward (attention.py:95-104, 479), `proj_in/proj_out`
// (attention.py:328,356), `conv_shortcut` (resnet.py:175,203), `F.interpolate` + conv (resnet.py:62-72),
// `torch.cat([h, skip])` (unet_blocks.py:538,630).
//
// Design (MI355X_MICROARCH / cdna_hip_programming §5):
//  * 64-wide waves, v_mfma_f32_16x16x32_f16, fp32 accumulation.  The WEIGHT tile is the MFMA A
//    operand and the ACTIVATION tile the B operand, so each lane ends up with 4 consecutive output
//    channels of one token: the epilogue stores 8-byte vectors along the contiguous axis.
//  * Both tiles are staged HBM -> LDS by `global_load_lds_dwordx4` (no VGPR round trip), K-tile 64
//    halfs = 128-B rows.  The LDS image is lane-linear, so the bank-conflict swizzle
//    (16-B slot ^= row & 7) is applied to the per-lane SOURCE address and again on the fragment
//    read (rule 21 of the guide); ds_read_b128 fragment reads are then conflict-free.
//  * Two LDS stages, one barrier per K-tile: loads of tile t+1 are in flight under the MFMAs of tile t.
//  * Out-of-image taps read a 128-B zero page instead of branching.
//  * blockIdx is remapped so that consecutive tiles (which share activation rows) share an XCD L2.
#include <math.h>

#include <type_traits>

#include "igemm.h"
#include "igemm_epilogue.h"
#include "igemm_stage.h"
#include "profile.h"

namespace lavie {

template <int WM, int WN, int MT, int NT, int NSTAGE>
struct IgemmTile {
    static constexpr int NW = WM * WN;
    static constexpr int THREADS = 64 * NW;
    static constexpr int BM = WM * MT * 16;
    static constexpr int BN = WN * NT * 16;
    static constexpr int STAGE_BYTES = (BM + BN) * 128;
    static constexpr int LDS_BYTES = NSTAGE * STAGE_BYTES;
    static constexpr int APIECES = BM / 8, WPIECES = BN / 8;          // 1-KiB pieces per stage
    static constexpr int AP = (APIECES + NW - 1) / NW;                 // pieces per wave per stage; when the count
    static constexpr int WP = (WPIECES + NW - 1) / NW;                 // does not divide, the surplus slots re-load
    static constexpr int LOADS = AP + WP;                              // pieces 0.. (same bytes, same place: benign)
    static constexpr int TAB_BYTES = gather_tab_bytes(BM);             // GATHER: source-pixel table + segment table
    static_assert(LDS_BYTES <= 160 * 1024, "tile does not fit LDS");
};

template <int WM, int WN, int MT, int NT, int NSTAGE, bool GATHER, int EPI>
__global__ __launch_bounds__(64 * WM * WN, 2) void igemm_kernel(const IgemmParams p) {
    using T = IgemmTile<WM, WN, MT, NT, NSTAGE>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // ---- XCD-aware tile order (bijective for any grid size) ----
    const int n_tiles = p.N / T::BN;
    int tile_m, tile_n, split = 0;
    if (gridDim.y == 1) {
        int bid = blockIdx.x;
        const int nwg = gridDim.x;
        split = blockIdx.y;
        bid = xcd_chunk(bid, nwg);
        igemm_tile_of(bid, (int)gridDim.x / n_tiles, n_tiles, (long)p.N * p.nk * IGEMM_BK, &tile_m, &tile_n);
    } else {
        // split-K = the weight-bound convolutions of the deep levels (M 1280, K 11520 .. 23040: 30 - 59 MB of weights for
        // 3 MB of activations).  N-fastest order spread the M tiles that share a weight slice over all eight XCDs and every XCD
        // pulled most of W through the fabric (PMC: 244 / 352 MB read per launch, ~5 TB/s under the kernel).  Here the whole
        // (x, y) grid is linearised as the hardware dispatches it, made XCD-contiguous, and walked M tile fastest, then N
        // tile, then K split: the workgroups that share a weight slice are neighbours inside one XCD's L2.
        const int nwg = gridDim.x * gridDim.y;
        const int lin = xcd_chunk(blockIdx.x + blockIdx.y * gridDim.x, nwg);
        const int m_tiles = (int)gridDim.x / n_tiles;
        tile_m = lin % m_tiles;
        const int rest = lin / m_tiles;
        tile_n = rest % n_tiles;
        split = rest / n_tiles;
    }
    const int m0 = tile_m * T::BM;
    const int n0 = tile_n * T::BN;

    // ---- staging addresses ----
    const int lr = lane >> 3;                       // row of this lane inside an 8-row piece
    const int kofs = ((lane & 7) ^ lr) * 8;         // source K offset (halfs) after the slot swizzle

    // GATHER: source-pixel and segment tables behind the stages (igemm_stage.h)
    int* tab = reinterpret_cast<int*>(smem + T::LDS_BYTES);
    const half_t* aptr[T::AP];
    int arow[T::AP];
#pragma unroll
    for (int i = 0; i < T::AP; ++i) {
        arow[i] = ((wave + T::NW * i) % T::APIECES) * 8 + lr;
        int m = m0 + arow[i];
        m = m < p.M ? m : p.M - 1;
        aptr[i] = GATHER ? p.zero : p.A + (size_t)m * p.lda + kofs;
    }
    if constexpr (GATHER) {
        gather_fill_pixels<T::BM, T::THREADS>(p, m0, tid, tab);
        __syncthreads();
    }
    const half_t* wptr[T::WP];
#pragma unroll
    for (int i = 0; i < T::WP; ++i) {
        const int n = n0 + ((wave + T::NW * i) % T::WPIECES) * 8 + lr;
        wptr[i] = p.W + (size_t)n * p.ldw + kofs;
    }

    // split-K: this workgroup owns K-tiles [t_begin, t_end) of the flattened K loop
    const int t_begin = (int)((long)p.nk * split / p.splits);
    const int t_end = (int)((long)p.nk * (split + 1) / p.splits);

    // gather cursor (igemm_stage.h: why the segment descriptors are read from LDS), positioned at t_begin
    auto sgpr = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    int* segtab = tab + T::BM * 9;                 // [IGEMM_MAX_SEG][6] : src lo, src hi, C, c0, nchunks, ntaps
    if constexpr (GATHER) {
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < IGEMM_MAX_SEG; ++i) {
                const unsigned long long a = reinterpret_cast<unsigned long long>(p.seg[i].src);
                segtab[i * 6 + 0] = (int)(unsigned)a;
                segtab[i * 6 + 1] = (int)(unsigned)(a >> 32);
                segtab[i * 6 + 2] = p.seg[i].C;
                segtab[i * 6 + 3] = p.seg[i].c0;
                segtab[i * 6 + 4] = p.seg[i].nchunks;
                segtab[i * 6 + 5] = p.seg[i].ntaps;
            }
        }
        __syncthreads();
    }
    auto load_seg = [&](int i) { return gather_load_seg(segtab, i); };
    const half_t* const zero_page = reinterpret_cast<const half_t*>(
        ((unsigned long long)(unsigned)sgpr((int)(unsigned)(reinterpret_cast<unsigned long long>(p.zero) >> 32)) << 32) |
        (unsigned)sgpr((int)(unsigned)reinterpret_cast<unsigned long long>(p.zero)));
    const int nseg = sgpr(p.nseg);
    int seg = 0, cchunk = 0, tap = 0;
    IgemmSeg sg = GATHER ? load_seg(0) : IgemmSeg{nullptr, 0, 0, 0, 1};
    if constexpr (GATHER) {
        int skip = t_begin;
        while (skip >= sg.nchunks * sg.ntaps && seg + 1 < nseg) {
            skip -= sg.nchunks * sg.ntaps;
            sg = load_seg(++seg);
        }
        cchunk = skip / sg.ntaps;
        tap = skip - cchunk * sg.ntaps;
    }

    // Source pointers of the NEXT tile to be issued are computed one step ahead, in two halves: `prepare_read` only
    // issues the pixel-table LDS reads (together with the fragment reads of the current tile, so their latency is
    // shared), `prepare_finish` does the address arithmetic and advances the cursor (placed between the two MFMA
    // blocks of a tile, where the matrix pipe is already fed).  prepare() = both, for the prologue.
    const half_t* nptr[T::AP];
    int pv[T::AP];
    auto prepare_read = [&]() {
        if constexpr (GATHER) {
            const int tp = sg.ntaps == 1 ? 4 : tap;
#pragma unroll
            for (int i = 0; i < T::AP; ++i) pv[i] = tab[arow[i] * 9 + tp];
        }
    };
    auto prepare_finish = [&](int t) {
        if constexpr (GATHER) {
            // 32-bit element offsets: a source tensor holds < 2^31 halfs (checked by the launcher)
            const unsigned cofs = (unsigned)(sg.c0 + cchunk * IGEMM_BK + kofs);
#pragma unroll
            for (int i = 0; i < T::AP; ++i) {
                const half_t* inside = sg.src + ((unsigned)pv[i] * (unsigned)sg.C + cofs);
                nptr[i] = pv[i] >= 0 ? inside : zero_page + kofs;
            }
            if (++tap == sg.ntaps) {
                tap = 0;
                if (++cchunk == sg.nchunks) {
                    cchunk = 0;
                    if (seg + 1 < nseg) sg = load_seg(++seg);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < T::AP; ++i) nptr[i] = aptr[i] + t * IGEMM_BK;
        }
    };
    auto prepare = [&](int t) { prepare_read(); prepare_finish(t); };
    auto issue = [&](int t, int buf) {
        char* base = smem + buf * T::STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < T::AP; ++i)
            __builtin_amdgcn_global_load_lds(GLB_PTR(nptr[i]), LDS_PTR(base + ((wave + T::NW * i) % T::APIECES) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < T::WP; ++i)
            __builtin_amdgcn_global_load_lds(GLB_PTR(wptr[i] + t * IGEMM_BK),
                                             LDS_PTR(base + T::BM * 128 + ((wave + T::NW * i) % T::WPIECES) * 1024), 16, 0, 0);
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // fragment read offsets inside a stage (bytes)
    const int frow = lane & 15;
    const int fsw = lane & 7;
    const int fg = lane >> 4;
    const int a_frag = (wm * MT * 16 + frow) * 128;
    const int w_frag = T::BM * 128 + (wn * NT * 16 + frow) * 128;

    // Fragment reads are issued for BOTH 32-deep k-steps of a tile before the first MFMA (two register sets), so the
    // LDS latency is exposed once per K-tile instead of once per fragment group; the LDS-DMA of the next tile is
    // issued between the reads and the MFMAs, under that latency.
    auto read_frags = [&](const char* base, int ks, half8_t (&af)[MT], half8_t (&wf)[NT]) {
        const int slot = ((ks * 4 + fg) ^ fsw) * 16;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const half8_t*>(base + a_frag + mt * 16 * 128 + slot);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[nt] = *reinterpret_cast<const half8_t*>(base + w_frag + nt * 16 * 128 + slot);
    };
    auto mfma_block = [&](half8_t (&af)[MT], half8_t (&wf)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt], af[mt], acc[nt][mt], 0, 0, 0);
            }
    };
    // one K-tile: fragment + table reads -> LDS-DMA issue of a later tile -> MFMAs(k-step 0) -> pointer arithmetic for
    // the tile after that -> MFMAs(k-step 1)
    auto tile_step = [&](int buf, auto&& issue_next, int t_prep) {
        const char* base = smem + buf * T::STAGE_BYTES;
        half8_t af0[MT], wf0[NT], af1[MT], wf1[NT];
        read_frags(base, 0, af0, wf0);
        read_frags(base, 1, af1, wf1);
        const bool prep = t_prep < t_end;
        if (prep) prepare_read();
        issue_next();
        mfma_block(af0, wf0);
        if (prep) prepare_finish(t_prep);
        mfma_block(af1, wf1);
    };
    if constexpr (NSTAGE == 2) {
        // one tile in flight: loads of tile t+1 run under the MFMAs of tile t
        prepare(t_begin);
        issue(t_begin, 0);
        if (t_begin + 1 < t_end) prepare(t_begin + 1);
        int buf = 0;
        for (int t = t_begin; t < t_end; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA pieces of tile t have landed
            __syncthreads();   // ... and everybody else's; the other buffer is no longer being read
            tile_step(buf, [&]() { if (t + 1 < t_end) issue(t + 1, buf ^ 1); }, t + 2);
            buf ^= 1;
        }
    } else {
        // NSTAGE-1 tiles in flight across the barrier: counted vmcnt + raw s_barrier (a __syncthreads() would
        // drain the LDS-DMA queue, guide §5 "Pipelining across barriers").  Every wave issues exactly
        // T::LOADS LDS-DMA instructions per tile, so "all but the newest (NSTAGE-2)*LOADS" == tile t landed.
        static_assert(NSTAGE == 3, "counted-wait schedule is written for 3 stages");
        prepare(t_begin);
        issue(t_begin, 0);
        if (t_begin + 1 < t_end) { prepare(t_begin + 1); issue(t_begin + 1, 1); }
        if (t_begin + 2 < t_end) prepare(t_begin + 2);
        int buf = 0;
        for (int t = t_begin; t < t_end; ++t) {
            if (t + 1 < t_end) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(T::LOADS) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                       // tile t visible to all; tile t-1's buffer is free
            asm volatile("" ::: "memory");
            tile_step(buf, [&]() { if (t + 2 < t_end) issue(t + 2, buf == 0 ? 2 : buf - 1); }, t + 3);
            buf = buf == 2 ? 0 : buf + 1;
        }
    }

    igemm_epilogue<MT, NT, EPI>(p, acc, m0 + wm * MT * 16 + (lane & 15), n0 + wn * NT * 16 + (lane >> 4) * 4,
                                n0 + wn * NT * 16, lane, split);
}

// out[m, n] = sum_s slab[s, m, n] (+ bias[n]) (+ bias2[m / rows_per_batch, n]) (+ R[m, n]); fixed summation order.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const IgemmParams p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int nv = p.N >> 2;
    if (idx >= (long)p.M * nv) return;
    const int m = (int)(idx / nv), n = (int)(idx - (long)m * nv) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(p.slab + (size_t)m * p.N + n);
    for (int s = 1; s < p.splits; ++s) v += *reinterpret_cast<const f32x4*>(p.slab + ((size_t)s * p.M + m) * p.N + n);
    if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + n);
    if (p.bias2) v += *reinterpret_cast<const f32x4*>(p.bias2 + (size_t)(m / p.rows_per_batch) * p.ldb2 + n);
    if (p.R) {
        const half4_t r = *reinterpret_cast<const half4_t*>(p.R + (size_t)m * p.ldr + n);
        v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
    }
    const half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
    *reinterpret_cast<half4_t*>(p.C + (size_t)m * p.ldc + n) = o;
}

// The same with GroupNorm column statistics of the rounded output (IgemmParams::colstat_out): a workgroup = 64 channel quads x 4
// row lanes over one block of COLSTAT_REDUCE_ROWS rows; the row lanes' sums (rows ascending per lane) meet in LDS in lane order.
constexpr int RCS_LANES = 16;       // row lanes: 2 rows each (4 lanes x 8 rows left the M = 1280 reduces at 200 workgroups of 256 threads: 15 us against 7)
__global__ __launch_bounds__(64 * RCS_LANES) void splitk_reduce_cs_kernel(const IgemmParams p) {
    __shared__ f32x4 s_sum[RCS_LANES][64], s_sq[RCS_LANES][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int nv = p.N >> 2;
    const int nq = blockIdx.x * 64 + tx, n = nq * 4;
    const int r0 = blockIdx.y * COLSTAT_REDUCE_ROWS;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f}, cq = {0.f, 0.f, 0.f, 0.f};
    if (nq < nv) {
        const f32x4 bv = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int m = r0 + ty; m < r0 + COLSTAT_REDUCE_ROWS && m < p.M; m += RCS_LANES) {
            f32x4 v = *reinterpret_cast<const f32x4*>(p.slab + (size_t)m * p.N + n);
            for (int s = 1; s < p.splits; ++s) v += *reinterpret_cast<const f32x4*>(p.slab + ((size_t)s * p.M + m) * p.N + n);
            v += bv;
            if (p.bias2) v += *reinterpret_cast<const f32x4*>(p.bias2 + (size_t)(m / p.rows_per_batch) * p.ldb2 + n);
            if (p.R) {
                const half4_t r = *reinterpret_cast<const half4_t*>(p.R + (size_t)m * p.ldr + n);
                v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
            }
            const half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *reinterpret_cast<half4_t*>(p.C + (size_t)m * p.ldc + n) = o;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float f = (float)o[r]; cs[r] += f; cq[r] += f * f; }
        }
    }
    s_sum[ty][tx] = cs;
    s_sq[ty][tx] = cq;
    __syncthreads();
    if (ty == 0 && nq < nv) {
        f32x4 a = s_sum[0][tx], b = s_sq[0][tx];
#pragma unroll
        for (int y = 1; y < RCS_LANES; ++y) { a += s_sum[y][tx]; b += s_sq[y][tx]; }
        float* dst = p.colstat_out + cs_index((size_t)blockIdx.y, n, 0, p.N);
        *reinterpret_cast<f32x4*>(dst) = a;
        *reinterpret_cast<f32x4*>(dst + 4) = b;
    }
}
// fixed-order sum of the split-K slabs + bias / residual / rounding (+ column statistics when the caller asked for them)
static int launch_splitk_reduce(const IgemmParams& p, hipStream_t stream) {
    if (p.colstat_out) {
        hipLaunchKernelGGL(splitk_reduce_cs_kernel, dim3(cdiv(p.N / 4, 64), cdiv(p.M, COLSTAT_REDUCE_ROWS)), dim3(64 * RCS_LANES), 0, stream, p);
    } else {
        const long total = (long)p.M * (p.N / 4);
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p);
    }
    LAVIE_HIP(hipGetLastError());
    return 0;
}

// ---- planner (igemm_plan): the force switches are decoded once, into the policy every rule below reads
static int g_force_tile = 0;   // see igemm_force_tile() in igemm.h
static int g_force_splits = 0;
void igemm_force_splits(int s) { g_force_splits = s; }
struct Policy {
    bool widest;        // 1, 3: the 128-row kernel takes the widest tile
    bool pp_split;      // all but 1, 4: the ping-pong grid rule proposes the split factor
    bool pp_rule;       // 0, 6, 8, 9: the ping-pong kernels run where their grid rule holds
    bool pp_force;      // 3: the ping-pong kernels run wherever N % 320 == 0 (GEGLU: N % 256 == 0)
    bool patch_split;   // 0, 5, 8, 9: the halo-patch grid rule proposes the split factor
    bool patch_rule;    // 0, 8, 9: the halo-patch kernel runs where its grid rule holds
    bool patch_force;   // 5: the halo-patch kernel runs wherever the conv is eligible
    bool ppx_rule;      // 0, 6, 9: the persistent kernel runs where its rule holds
    bool ppx_geglu;     // 0: ... for the GEGLU GEMMs too
    bool ppx_force;     // 7: the persistent kernel runs for every plain GEMM of its shape
    int splits;         // force_splits, 0 = automatic
};
static Policy policy() {
    const int m = g_force_tile;
    return Policy{m == 1 || m == 3, m != 1 && m != 4, m == 0 || m == 6 || m == 8 || m == 9, m == 3, m == 0 || m == 5 || m == 8 || m == 9,
                  m == 0 || m == 8 || m == 9, m == 5, m == 0 || m == 6 || m == 9, m == 0, m == 7, g_force_splits};
}

// measured: at 5 K-tiles (K = 320) the GEGLU epilogue, with no second workgroup to hide it, loses; from 8 K-tiles on the
// ping-pong variant wins or ties (K = 640 of the base model: +0.2 %, K = 512 of the VSR UNet: GEMM class -3.5 %)
constexpr int GEGLU_PP_MIN_NK = 8;

// ---- 160x320 ping-pong kernel (igemm_pp.hip): when it is used.  Measured on this model's shapes (tools/bench_ops.py
// pp_splits, check_pp): it is 15-25 % faster than the 128-row kernel whenever its grid quantises onto the 256 CUs
// (one workgroup per CU) and the K loop is long enough to amortise its 60 KiB prologue; an under-filled grid or a
// short K loop loses.  Rule: N % 320 == 0, >= 10 K-tiles, the grid's last round at least 85 % full, and with
// split-K at least 45 K-tiles per split (the fp32 slab round trip must stay small beside the loop).
// tile width of the ping-pong kernel for this N: 320, or 256 (NT = 4) for the power-of-two widths of the VSR UNet; 0 = none
static int pp_bn(int N) { return N % 320 == 0 ? 320 : (N % 256 == 0 ? 256 : 0); }
static bool pp_fits(int M, int N, int nk, int s) {
    const int bn = pp_bn(N);
    if (bn == 0 || nk < 10 || s < 1 || s > nk) return false;      // (5 K-tiles at N = 320 measured +0.2 %: within noise, not taken)
    if (s > 1 && nk / s < 40) return false;       // (40: the L2 ff2 GEMM, 80 K-tiles, 128 tiles: 91 -> 79 us with two splits)
    const double r = (double)cdiv(M, 160) * (N / bn) * s / 256.0;
    return r / ceil(r) >= 0.85;
}
// split-K factor with which the ping-pong kernel should run this problem, 0 = do not use it
static int pp_plan(const Policy& q, int M, int N, int nk, int epilogue) {
    if (epilogue != EPI_LINEAR || !q.pp_split) return 0;
    for (int s = 1; s <= 4; ++s)
        if (pp_fits(M, N, nk, s)) return s;
    return 0;
}

// ---- 320x160 halo-patch conv kernel (igemm_patch.hip): 5-8 % faster than the ping-pong kernel on the convs it accepts
// (tools/check_patch.py); same grid rule with its own tile: one workgroup per CU, last round at least 85 % full,
// split-K (over whole slabs) only with at least 45 K-tiles per split.
static bool patch_fits(int M, int N, int nk, int s, int ntaps = 9) {
    // temporal convs (ntaps 3 / 5): the 128-wide tile only, and only from 1024 channels on — tools/bench_ops.py tconv measured
    // the temporal mode equal to the ping-pong kernel within +-5 % at 256 / 512 channels (short K loops: 12 - 40 K-tiles, the
    // activation tile is staged once per N tile instead of once) and 30 % ahead at 1024
    if (ntaps != 9 && N < 1024) return false;
    const int bn = ntaps == 9 ? igemm_patch_bn(N) : (N % 128 == 0 ? 128 : 0);
    if (M % 320 != 0 || bn == 0 || nk % ntaps != 0 || s < 1 || s > nk / ntaps) return false;
    if (s > 1 && nk / s < 45) return false;
    const double r = (double)(M / 320) * (N / bn) * s / 256.0;
    return r / ceil(r) >= 0.85;
}
static int pt_bm_rows() { return 320; }      // the halo-patch kernel's tile height (igemm_patch.hip pt::BM)

// ---- persistent ping-pong kernel (igemm_ppx.hip) for plain GEMMs: forced (mode 7) or by the measured rule; shape only
static bool ppx_shape(const Policy& q, int M, int N, int nk, int epilogue) {
    if (M % 160 != 0 || nk < 5 || (epilogue == EPI_GEGLU ? N % 256 != 0 : (N % 320 != 0 && N % 256 != 0))) return false;   // = igemm_ppx_eligible's shape part
    if (q.ppx_force) return true;
    if (!q.ppx_rule) return false;
    // Measured (tools/check_ppx.py, profiles/r02_ppx_shapes.txt): the persistent kernel wins where the K loop is short and
    // every CU gets at least one whole tile — the L0 GEMMs with K = 320 (N = 320: -14 .. -23 %, QKV -7 %, GEGLU -10 %) and
    // the L1 K = 640 linear ones (-3 .. -10 %); it loses on long K loops (the one-tile kernels' second workgroup per CU
    // hides their epilogue better) and on under-filled grids (M = 5120: 128 tiles).
    // GEGLU: -10 % in the operator benchmark but +3 % inside the UNet (rocprofv3, profiles/r02_a_kernel_summary.md: its
    // VALU-heavy epilogue stalls both groups once per tile): left to the one-tile kernels.
    // Round 4, re-measured inside the forward (tools/ab_tile.py, profiles/r04_ab_geglu_on_persistent_kernel.txt, same box,
    // interleaved, A B B A): with the level-1 GEGLU GEMM (K = 640) on the persistent kernel the forward is 0.23 ms shorter (20.18 vs
    // 20.41 ms) at an unchanged class time — its stores are spread over the launch instead of ending it in one burst: taken (mode 9
    // runs the automatic rule without it for A/B).  The same run order showed that EXACTLY one tile per CU (level-1 N = 640) still
    // belongs here and not on the one-tile kernel, although that is 11 % faster in isolation.
    const long tiles = (long)(M / 160) * (N / pp_bn(N));
    if (tiles < 256 || nk > 10) return false;
    return epilogue == EPI_LINEAR || q.ppx_geglu;
}

// Tile width by grid quantisation: the 4-wave tiles run 2 workgroups per CU (512 slots per round); a narrower
// tile is a little less efficient per flop (exponent 0.9) but can save a whole round on short grids.
static int igemm_pick_bn(const Policy& q, int M, int N, int splits) {
    double best = 1e30;
    int bn = 0;
    const int cand[3] = {160, 128, 64};
    for (int i = 0; i < 3; ++i) {
        if (N % cand[i] != 0) continue;
        const long blocks = (long)cdiv(M, 128) * (N / cand[i]) * splits;
        const double cost = (double)((blocks + 511) / 512) * pow(cand[i] / 160.0, 0.9);
        if (cost < best * 0.97) { best = cost; bn = cand[i]; }
    }
    if (q.widest && N % 160 == 0) bn = 160;   // forced modes: widest
    return bn;
}

// Split-K factor.  The 128-row tiles run 2 workgroups per CU (512 slots); a grid of `blocks` tiles takes ceil(blocks*S/512)
// rounds of (nk/S + fixed) K-steps plus a reduce pass over S slabs.
static int plan_splits(const Policy& q, const IgemmParams& p, bool gather, int epilogue) {
    if (p.ln_stats || p.rowstat_out) return 1;                     // LayerNorm folding: a plain, unsplit GEMM
    if (p.par_ups) {
        // parity upsample: one workgroup per CU and 85 % of a round as everywhere in the family; split-K over whole slabs when the
        // grid is short.  Quirk: force_splits does not apply here.
        const int nchunks = p.seg[0].nchunks;
        const long wgs = (long)(p.M / 4 / pt_bm_rows()) * (p.N / 160) * 4;
        return wgs >= 218 ? 1 : (2 * wgs >= 218 && nchunks >= 10) ? 2 : (nchunks >= 20 ? 4 : 1);
    }
    if (gather) {
        if (q.splits == 0 && q.patch_split) {
            IgemmParams t = p;
            for (int s = 1; s <= 4; ++s) {
                t.splits = s;
                if (patch_fits(p.M, p.N, p.nk, s, p.tframes > 0 ? p.seg[0].ntaps : 9) && igemm_patch_eligible(t)) return s;
            }
        }
        epilogue = EPI_LINEAR;
    }
    if (epilogue != EPI_LINEAR || p.N % 64 != 0) return 1;
    // quirk: the persistent kernel's shape, not its eligibility, makes a plain GEMM unsplit (where it refuses, another kernel runs)
    if (!gather && q.splits == 0 && ppx_shape(q, p.M, p.N, p.nk, epilogue)) return 1;
    if (q.splits > 0) return q.splits <= p.nk ? q.splits : 1;
    // quirk: modes 2, 5 and 7 take the ping-pong rule's split factor, though the ping-pong kernel does not run under them
    if (const int s = pp_plan(q, p.M, p.N, p.nk, epilogue)) return s;
    const long blocks = (long)cdiv(p.M, 128) * cdiv(p.N, 160);
    if (blocks >= 1024) return 1;
    double best = 1e30;
    int best_s = 1;
    for (int s = 1; s <= 8; ++s) {
        if (s > 1 && p.nk / s < 12) break;
        const double rounds = (double)((blocks * s + 511) / 512);
        double cost = rounds * ((double)p.nk / s + 6.0);
        if (s > 1) cost += 1.5e-6 * s * (double)p.M * p.N;     // slab write + read (~8 s M N bytes at ~4 TB/s) in K-step units of ~1.3 us
        if (cost < best * 0.93) { best = cost; best_s = s; }
    }
    return best_s;
}

// the kernel for `p` at split factor p.splits
static void plan_kernel(const Policy& q, const IgemmParams& p, bool gather, int epilogue, IgemmPlan* r) {
    const bool ppx = !gather && p.splits == 1 && igemm_ppx_eligible(p, epilogue) && ppx_shape(q, p.M, p.N, p.nk, epilogue);
    if (p.par_ups) {                       // parity form of an upsample conv: the halo-patch kernel is the only one that runs it
        *r = {IGEMM_PATCH_PARITY, 160};
    } else if (epilogue == EPI_GEGLU) {    // 160x256 ping-pong variant: the 160x320 kernel's grid rule, from GEGLU_PP_MIN_NK K-tiles on
        const double f = (double)cdiv(p.M, 160) * (p.N / 256) / 256.0;
        if (ppx) *r = {IGEMM_PPX, 256};
        else if (p.N % 256 == 0 && (q.pp_force || (q.pp_rule && p.nk >= GEGLU_PP_MIN_NK && f / ceil(f) >= 0.85))) *r = {IGEMM_PP_GEGLU, 256};
        else *r = {IGEMM_TILE, 128};
    } else if (ppx) {
        *r = {IGEMM_PPX, pp_bn(p.N)};
    } else if (gather && igemm_patch_eligible(p) &&
               (q.patch_force || (q.patch_rule && patch_fits(p.M, p.N, p.nk, p.splits, p.tframes > 0 ? p.seg[0].ntaps : 9)))) {
        if (p.tframes > 0) *r = {IGEMM_PATCH_TEMPORAL, 128};
        else *r = {pt_bm_rows() % p.Wo != 0 ? IGEMM_PATCH_2D : IGEMM_PATCH_ROWS, igemm_patch_bn(p.N)};
    } else if ((q.pp_force && p.N % 320 == 0) || (q.pp_rule && pp_fits(p.M, p.N, p.nk, p.splits))) {
        *r = {IGEMM_PP, pp_bn(p.N)};
    } else {                               // 128-row kernel: two independent workgroups per CU, tile width by grid quantisation
        *r = {IGEMM_TILE, igemm_pick_bn(q, p.M, p.N, p.splits)};
    }
}

IgemmPlan igemm_plan(const IgemmParams& p0, bool gather, int epilogue) {
    const Policy q = policy();
    IgemmParams p = p0;
    p.splits = plan_splits(q, p0, gather, epilogue);
    IgemmPlan r;
    plan_kernel(q, p, gather, epilogue, &r);
    r.gather = gather;
    r.epilogue = epilogue;
    r.splits = p.splits;
    // quirk: row-statistics slots follow the shape rules alone (the persistent kernel's shape without its eligibility, the ping-pong
    // split rule, mode 3 by N % 320); launch_igemm refuses a launch whose kernel writes other slots
    if (ppx_shape(q, p.M, p.N, p.nk, EPI_LINEAR) || (q.pp_force ? p.N % 320 == 0 : pp_plan(q, p.M, p.N, p.nk, EPI_LINEAR) == 1))
        r.rowstat_cols = pp_bn(p.N) / 4;
    else
        r.rowstat_cols = igemm_pick_bn(q, p.M, p.N, 1) / 2;
    // column statistics: 16 * MT rows of the kernel that runs; the split-K reduce writes them when there are slabs
    r.colstat_rows = epilogue != EPI_LINEAR ? 0 : p.splits > 1 ? COLSTAT_REDUCE_ROWS : r.kernel != IGEMM_TILE ? 80 : r.bn != 0 ? 64 : 0;
    r.colstat_span = r.colstat_rows;
    if (r.colstat_rows > 0 && p.splits == 1) {
        const int rows = r.colstat_rows, hw = p.Ho * p.Wo;
        if (r.kernel == IGEMM_PATCH_PARITY) {           // 80 source rows -> their 4 output parities, one set each
            const int shw = p.Hi * p.Wi;
            r.colstat_span = 4 * (shw % rows == 0 ? shw : (rows % shw == 0 ? rows : 320));
        } else if (r.kernel == IGEMM_PATCH_TEMPORAL) {  // a tile = every frame of 320 / F pixels of ONE video
            r.colstat_span = p.tframes * p.tpix;
        } else if (r.kernel == IGEMM_PATCH_2D) {        // 2-D tile: 10 rows x 32 columns of ONE frame
            r.colstat_span = hw;
        } else if (r.kernel == IGEMM_PATCH_ROWS) {      // whole image rows: contiguous; frames smaller than a wave tile nest
            r.colstat_span = hw % rows == 0 || rows % hw == 0 ? rows : 320;
        }
    }
    return r;
}

template <int WM, int WN, int MT, int NT, int NSTAGE, bool GATHER, int EPI>
static int launch_tile(const IgemmParams& p, hipStream_t stream) {
    using T = IgemmTile<WM, WN, MT, NT, NSTAGE>;
    auto kern = igemm_kernel<WM, WN, MT, NT, NSTAGE, GATHER, EPI>;
    constexpr int lds = T::LDS_BYTES + (GATHER ? T::TAB_BYTES : 0);
    static_assert(lds <= 160 * 1024, "tile + pixel table do not fit LDS");
    static bool attr_set = false;   // one per instantiation
    if (!attr_set) {
        LAVIE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set = true;
    }
    const int grid = cdiv(p.M, T::BM) * (p.N / T::BN);
    hipLaunchKernelGGL(kern, dim3(grid, p.splits), dim3(T::THREADS), lds, stream, p);
    LAVIE_HIP(hipGetLastError());
    if (p.splits > 1) return launch_splitk_reduce(p, stream);
    return 0;
}

__global__ void rowstat_finalize_kernel(const float* __restrict__ partials, int slots, int M, float inv_len, float eps,
                                        float* __restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const float* st = partials + (size_t)m * slots * 2;
    float sum = 0.f, sq = 0.f;
    for (int j = 0; j < slots; ++j) { sum += st[2 * j]; sq += st[2 * j + 1]; }
    const float mean = sum * inv_len;
    out[(size_t)m * 2] = mean;
    out[(size_t)m * 2 + 1] = rsqrtf(fmaxf(sq * inv_len - mean * mean, 0.f) + eps);
}

int launch_rowstat_finalize(const float* partials, int slots, int M, int row_len, float eps, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(rowstat_finalize_kernel, dim3(cdiv(M, 256)), dim3(256), 0, stream, partials, slots, M,
                       1.0f / (float)row_len, eps, out);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

int launch_igemm(const IgemmParams& p, const IgemmPlan& plan, hipStream_t stream) {
    const bool gather = plan.gather;
    const int epilogue = plan.epilogue;
    LAVIE_CHECK(p.M > 0 && p.N > 0 && p.nk > 0, "igemm: empty problem M=%d N=%d nk=%d", p.M, p.N, p.nk);
    const double K = (double)p.nk * IGEMM_BK;
    // algorithmic work: 2 M N K flops; bytes = every operand element once (A incl. im2col reuse counted once)
    ProfileScope prof(gather ? KC_CONV3X3 : KC_LINEAR, stream, 2.0 * p.M * p.N * K,
                      2.0 * ((double)p.M * K / (gather ? 9.0 : 1.0) + (double)p.N * K + (double)p.M * p.N));
    LAVIE_CHECK(p.N % 4 == 0 && p.ldc % 4 == 0, "igemm: N and ldc must be multiples of 4");
    LAVIE_CHECK(!(p.rowstat_out || p.ln_stats) || (p.splits == 1 && !gather), "igemm: LayerNorm folding needs a plain, unsplit GEMM");
    LAVIE_CHECK(p.splits == plan.splits && p.splits >= 1 && p.splits <= p.nk && (p.splits == 1 || (p.slab && epilogue == EPI_LINEAR)),
                "igemm: bad split-K setup (splits=%d, planned %d)", p.splits, plan.splits);
    LAVIE_CHECK(!p.colstat_out || plan.colstat_rows > 0, "igemm: column statistics asked of a launch that writes none");
    if (p.par_ups)
        LAVIE_CHECK(gather && epilogue == EPI_LINEAR && igemm_patch_eligible(p), "igemm: parity upsample conv outside the halo-patch kernel's geometry");
    if (epilogue == EPI_GEGLU) {
        LAVIE_CHECK(p.N % 128 == 0, "igemm: GEGLU needs N %% 128 == 0 (N=%d)", p.N);
        LAVIE_CHECK(!p.R && !p.bias2, "igemm: GEGLU epilogue takes no residual / per-batch bias");
        LAVIE_CHECK(!gather, "igemm: GEGLU epilogue is only built for plain A rows");
    } else {
        // row statistics: one slot per wave tile (16 * NT columns) of the kernel that runs
        const int cols = plan.kernel == IGEMM_TILE ? plan.bn / 2 : plan.bn / 4;
        LAVIE_CHECK(!p.rowstat_out || plan.rowstat_cols == cols, "igemm: row-statistics slots planned for %d columns, the kernel writes %d",
                    plan.rowstat_cols, cols);
    }
    int rc = 0;
    switch (plan.kernel) {
    case IGEMM_PPX: return launch_igemm_ppx(p, epilogue, stream);
    case IGEMM_PP_GEGLU: return launch_igemm_pp_geglu(p, stream);
    case IGEMM_PP: rc = launch_igemm_pp(p, gather, stream); break;
    case IGEMM_TILE:        // (launch_tile runs the split-K reduce itself)
        if (epilogue == EPI_GEGLU) return launch_tile<2, 2, 4, 4, 2, false, EPI_GEGLU>(p, stream);
        LAVIE_CHECK(plan.bn != 0, "igemm: N=%d is not a multiple of 64", p.N);
        if (plan.bn == 160)
            return gather ? launch_tile<2, 2, 4, 5, 2, true, EPI_LINEAR>(p, stream) : launch_tile<2, 2, 4, 5, 2, false, EPI_LINEAR>(p, stream);
        if (plan.bn == 128)
            return gather ? launch_tile<2, 2, 4, 4, 2, true, EPI_LINEAR>(p, stream) : launch_tile<2, 2, 4, 4, 2, false, EPI_LINEAR>(p, stream);
        return gather ? launch_tile<2, 2, 4, 2, 2, true, EPI_LINEAR>(p, stream) : launch_tile<2, 2, 4, 2, 2, false, EPI_LINEAR>(p, stream);
    default: rc = launch_igemm_patch(p, stream); break;
    }
    if (rc) return rc;
    return p.splits > 1 ? launch_splitk_reduce(p, stream) : 0;      // fixed-order sum of the split-K slabs + bias / residual / rounding
}

int igemm_force_tile(int mode) {
    LAVIE_CHECK(mode >= 0 && mode <= 9, "force_tile: mode %d is not one of 0 - 9", mode);
    g_force_tile = mode;
    return 0;
}

}  // namespace lavie
