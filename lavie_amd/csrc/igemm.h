// Implicit-GEMM MFMA kernel family: parameters shared by Linear / 1x1 conv / 3x3 conv launchers.
#pragma once
#include "common.h"

namespace lavie {

constexpr int IGEMM_MAX_SEG = 4;    // two conv sources + two shortcut sources
constexpr int IGEMM_BK = 64;    // K-tile in halfs: 128-B rows in LDS, one 16x16x32 MFMA pair per tile

// One K-segment of the A operand: a source tensor `src` (channels-last rows of `C` halfs) contributing
// `nchunks` 64-channel slabs, each visited at `ntaps` spatial taps (9 = the 3x3 stencil, 1 = centre only).
// K order inside a segment: slab-major, tap-minor.  A 3x3 conv over a concatenated input [x1 | x2] is two
// 9-tap segments; a fused 1x1 shortcut appends one or two 1-tap segments.
struct IgemmSeg {
    const half_t* src;
    int C;        // row length (channels) of src
    int c0;       // first channel of this segment inside src rows
    int nchunks;  // number of 64-channel slabs
    int ntaps;    // 9 (3x3) or 1 (centre tap: fused 1x1 shortcut); temporal mode: 3 or 5 frame taps
};

struct IgemmParams {
    // A operand, plain mode (GATHER = false): row-major [M, K] with leading dimension lda.
    const half_t* A;
    int lda;
    // W operand: row-major [N, Ktot] (PyTorch Linear layout; conv weights repacked [Cout][tap][Cin]).
    const half_t* W;
    int ldw;
    half_t* C;
    int ldc;
    const float* bias;    // [N] or nullptr   (GEGLU: permuted like W rows)
    const float* bias2;   // [M / rows_per_batch, ldb2] or nullptr (time-embedding projection per video)
    int ldb2;
    int rows_per_batch;
    const half_t* R;      // residual [M, N] (ldr) or nullptr; may alias C
    int ldr;
    int M, N, nk;         // nk = total number of K-tiles
    // LayerNorm folding: a producer GEMM writes per-row partial (sum, sum of squares) of its fp16 output,
    // one pair per 16*NT-column wave tile: rowstat_out[m * rowstat_slots + slot]; the consumer GEMM runs on the RAW
    // rows with gamma folded into W and finishes  y = rstd_m (acc - mean_m s_n) + bias_n  in its epilogue.
    float* rowstat_out;        // [M, N / IgemmPlan::rowstat_cols, 2] or nullptr (EPI_LINEAR, splits == 1 only)
    const float* ln_stats;     // [M, 2] (mean, rstd) of the A rows (launch_rowstat_finalize), or nullptr
    const float* ln_s;         // [N]: s_n = sum_k W'[n, k]
    // GroupNorm statistics from the producer (round 4): per (row block, channel) sum and sum of squares of the ROUNDED fp16 output,
    // written by the epilogue that stores the tensor (or by the split-K reduce), so that the consuming GroupNorm needs no statistics
    // pass over the tensor (resnet.py:180,191; attention.py:369; unet.py:504).  Layout (cs_index below): per block and channel quad
    // four sums then four sums of squares.  A block = the rows of one wave tile (IgemmPlan::colstat_rows = 16 * MT of the kernel that
    // runs, 32 for the split-K reduce); the parity-form upsample conv writes four sets of source-row blocks (one per output parity).
    float* colstat_out;        // [sets][ceil(rows / colstat_rows)][N / 4][2][4] or nullptr (EPI_LINEAR only)
    int splits;           // split-K factor (1 = none); > 1 needs `slab`
    float* slab;          // [splits, M, N] fp32 partial sums
    // Gather geometry (GATHER = true): output pixel grid [NI, Ho, Wo], source grid [NI, Hi, Wi],
    // virtual input grid (Hi << ups, Wi << ups) for the folded nearest-x2 upsample.
    int Ho, Wo, Hi, Wi, stride, ups;
    // Leading pad of the 3x3 stencil: tap (ky, kx) of output (y, x) reads input (y stride + ky - pad_lo, x stride + kx - pad_lo).
    // 1 = the symmetric pad-1 conv (every conv of the UNet); 0 with stride 2 = the VAE encoder's downsampler, which pads one
    // zero row / column at the far side only (F.pad(x, (0, 1, 0, 1)) + a pad-0 conv).  Read by the 9-tap gather alone.
    int pad_lo;
    // Temporal mode (tframes > 0; GATHER = true; 128-row and ping-pong kernels): rows are tokens (b, f, pixel) with tpix pixels per
    // frame, and tap t of a segment with ntaps = T reads row m + (t - T/2) * tpix, or zeros when frame f + t - T/2 falls
    // outside [0, tframes) — nn.Conv3d with kernel (T, 1, 1), padding (T/2, 0, 0) (vsr/models/resnet.py:258-259, 274).
    int tframes, tpix;
    int nseg;
    int par_ups;          // halo-patch kernel only: parity form of the 3x3 conv of a nearest-x2 upsampled image (igemm_patch.hip MODE 3):
                          // W = four [N][ldw] matrices (parity py * 2 + px), one 4-tap segment, M = OUTPUT rows, Hi x Wi = source grid
    IgemmSeg seg[IGEMM_MAX_SEG];
    const half_t* zero;   // >= 128 B of zeros: source of out-of-image taps
};

enum IgemmEpilogue { EPI_LINEAR = 0, EPI_GEGLU = 1 };

// The kernels of the family; the halo-patch kernel by its mode (igemm_patch.hip MODE 0 - 3).
enum IgemmKernel {
    IGEMM_TILE,              // 128-row kernel (this file's igemm_kernel), bn = 160 / 128 / 64; GEGLU: 128
    IGEMM_PP,                // 160x320 ping-pong kernel (igemm_pp.hip), bn = 320, or 256 for the power-of-two widths
    IGEMM_PP_GEGLU,          // its 160x256 GEGLU variant
    IGEMM_PPX,               // persistent ping-pong kernel (igemm_ppx.hip), bn = 320 / 256
    IGEMM_PATCH_ROWS,        // halo-patch 3x3 conv kernel, tiles of whole image rows
    IGEMM_PATCH_2D,          // ... 2-D tiles (10 image rows x 32 columns)
    IGEMM_PATCH_TEMPORAL,    // ... temporal (T,1,1) conv
    IGEMM_PATCH_PARITY,      // ... parity form of the 3x3 conv of a nearest-x2 upsampled image
};

// Everything launch_igemm will do for one GEMM, decided once by igemm_plan.  The plan reads the shape, strides and segments of the
// parameters, which optional operands are present (R, bias2, ln_stats, rowstat_out; never their addresses) and the force switches:
// the workspace dry run, which passes placeholder addresses, gets the plan of the real call.
struct IgemmPlan {
    IgemmKernel kernel;
    int bn;              // column-tile width of the kernel (0: N is not a multiple of 64, the launch is refused)
    int splits;          // split-K factor: the caller sets p.splits to it and, when > 1, p.slab to splits * M * N floats
    int rowstat_cols;    // columns per row-statistics slot: rowstat_out holds N / rowstat_cols slots per row
    int colstat_rows;    // rows per column-statistics block: 80 (halo-patch, ping-pong and persistent kernels), 64 (128-row kernel),
                         // 32 (split-K: the reduce kernel writes them), 0 = this launch cannot emit them (GEGLU)
    int colstat_span;    // the aligned run of output rows inside which the rows of one block lie (GnColStat::span): the block height
                         // for kernels whose wave tiles are contiguous rows; one frame for the halo-patch kernel's 2-D tiles and for
                         // the parity-form upsample conv; one video for its temporal-conv tiles
    bool gather;
    int epilogue;
};
IgemmPlan igemm_plan(const IgemmParams& p, bool gather, int epilogue);
// Launches the planned kernel (+ the split-K reduce).  Returns 0 or a negative status with lavie::set_error().
int launch_igemm(const IgemmParams& p, const IgemmPlan& plan, hipStream_t stream);
// One implicit GEMM from parameters to launch: plan it, set p.splits, point p.colstat_out at `cs_buf` when the planned launch writes
// column statistics (else nullptr), take the split-K slab from `slab(bytes, &p.slab)` (called only when the plan splits; returns 0
// or an error), launch unless `dry`.  *plan_out (optional) receives the plan.
template <class SlabSource>
int igemm_run(IgemmParams& p, bool gather, int epilogue, hipStream_t stream, SlabSource&& slab, float* cs_buf = nullptr, bool dry = false,
              IgemmPlan* plan_out = nullptr) {
    const IgemmPlan plan = igemm_plan(p, gather, epilogue);
    if (plan_out) *plan_out = plan;
    p.splits = plan.splits;
    p.colstat_out = plan.colstat_rows > 0 ? cs_buf : nullptr;
    p.slab = nullptr;
    if (p.splits > 1)
        if (const int rc = slab((size_t)p.splits * p.M * p.N * sizeof(float), &p.slab)) return rc;
    return dry ? 0 : launch_igemm(p, plan, stream);
}
// 160x320 two-group ping-pong kernel (igemm_pp.hip); EPI_LINEAR only, N %% 320 == 0, the caller runs the split-K reduce.
int launch_igemm_pp(const IgemmParams& p, bool gather, hipStream_t stream);
int launch_igemm_pp_geglu(const IgemmParams& p, hipStream_t stream);   // 160x256 variant, GEGLU epilogue, N %% 256 == 0
// Persistent ping-pong kernel (igemm_ppx.hip): plain A rows, no split-K; at most 256 workgroups walk the output tiles with
// the LDS-DMA stream running across tile boundaries.  EPI_LINEAR (N %% 320 == 0 or N %% 256 == 0) and EPI_GEGLU (N %% 256 == 0).
bool igemm_ppx_eligible(const IgemmParams& p, int epilogue);
int launch_igemm_ppx(const IgemmParams& p, int epilogue, hipStream_t stream);
// 320x160 halo-patch 3x3 conv kernel (igemm_patch.hip): stride 1, 9-tap segments only; the caller runs the split-K reduce.
bool igemm_patch_eligible(const IgemmParams& p);
int igemm_patch_bn(int N);                        // 160 / 128 / 0: column-tile width of the halo-patch kernel for N channels
int launch_igemm_patch(const IgemmParams& p, hipStream_t stream);
// Geometry of a 3x3 conv (pad 1, stride 1 / 2, `ups` = folded nearest-x2 upsample; pad_lo = 0: stride 2 only, the far-side pad of
// IgemmParams::pad_lo, Ho = (Hi - 2) / 2 + 1) y [NI, Ho, Wo, Cout] over the channel-concatenated
// sources src[0..nsrc) (9-tap segments) and the centre-tap shortcut sources sc[0..nsc) (stride 1 only), sources of 0 channels
// skipped; W rows of ldw halfs.  Fills p (zeroed first; rows_per_batch = 1, the caller adds bias, bias2, R).  0 or an error.
int igemm_setup_conv3x3(IgemmParams* p, const half_t* const* src, const int* srcC, int nsrc, const half_t* const* sc, const int* scC,
                        int nsc, const half_t* W, int ldw, half_t* y, int NI, int Hi, int Wi, int Cout, int stride, int ups,
                        const half_t* zero, int pad_lo = 1);
// Plain GEMM C [M, N] (ldc) = A [M, K] (lda) W [N, K]^T (ldw) + bias: fills p (zeroed first; rows_per_batch = 1, ldr = ldc).  ldc = N / 2
// for the GEGLU epilogue.  The caller adds the optional operands: R (+ ldr), bias2 (+ ldb2, rows_per_batch), the LayerNorm fold
// (ln_s, ln_stats) or rowstat_out.  0 or an error.
int igemm_setup_linear(IgemmParams* p, const half_t* A, int lda, const half_t* W, int ldw, const float* bias, half_t* C, int ldc, int M,
                       int N, int K);
// (taps,1,1) temporal conv y [(b f d), Cout] over the frame axis of token rows x [(b f d), C] (IgemmParams temporal mode), W rows of
// taps * C halfs: fills p (zeroed first; rows_per_batch = 1, ldr = Cout; the caller adds bias2, rows_per_batch, R).  0 or an error.
int igemm_setup_temporal_conv(IgemmParams* p, const half_t* x, int C, const half_t* W, const float* bias, half_t* y, int B, int F, int D,
                              int Cout, int taps, const half_t* zero);
// parity form of conv3x3(nearest_x2(x)) (igemm_patch.hip MODE 3): fills p (geometry only; the caller sets p->slab), false = not this
// geometry
bool igemm_setup_parity_upsample(IgemmParams* p, const half_t* x, int C, const half_t* wpar, const float* bias, half_t* y, int NI, int Hi,
                                 int Wi, const half_t* zero);
constexpr int COLSTAT_REDUCE_ROWS = 32;
// float index of (block, channel c, which = 0 sum / 1 sum of squares) in a column-statistics buffer of a C-channel tensor
__host__ __device__ inline size_t cs_index(size_t block, int c, int which, int C) {
    return ((block * (size_t)(C >> 2) + (size_t)(c >> 2)) * 2 + (size_t)which) * 4 + (size_t)(c & 3);
}
// partials [M, slots, 2] (sum, sum of squares over `row_len` values per row) -> out [M, 2] = (mean, rstd); fixed order
int launch_rowstat_finalize(const float* partials, int slots, int M, int row_len, float eps, float* out, hipStream_t stream);
// Low nibble: 0 = automatic kernel / tile choice, 1 = 128-row kernel with the widest tile,
// 3 = 160x320 ping-pong kernel whenever N %% 320 == 0, 4 = automatic but never the ping-pong kernel (A/B timing),
// 5 = halo-patch conv kernel whenever the conv is eligible, 6 = automatic but never the halo-patch kernel,
// 7 = persistent ping-pong kernel for every eligible plain GEMM, 8 = automatic but never the persistent kernel,
// 9 = automatic but without the GEGLU GEMMs on the persistent kernel.  Any other value: error, the mode stays as it was.
int igemm_force_tile(int mode);
void igemm_force_splits(int s);   // 0 = automatic

}  // namespace lavie
