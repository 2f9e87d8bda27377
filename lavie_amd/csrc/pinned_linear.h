// The one GEMM plan of the encoders behind lavie_text_*, lavie_vision_* and lavie_mapper_* (DESIGN.md 7.16, 7.17): the planner
// chooses by (M, N, K) and M moves with the batch, so these objects bypass it.  The 128-row kernel at 128 columns and no split-K:
// an output element is the sum of its K products in an order that depends on K alone, whatever M is and wherever its row lies.
#pragma once
#include "igemm.h"

namespace lavie {

constexpr int kPinBn = 128;      // the one tile width: every N of the encoders is a multiple of it

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// C [M, N] (ldc) = A [M, K] (lda) W [N, K]^T + bias (+ R (ldr), which may alias C) on the pinned plan; fp32 sum, one rounding
inline int pinned_linear(const half_t* A, int lda, const half_t* W, const float* bias, const half_t* R, int ldr, half_t* C, int ldc, int M,
                         int N, int K, hipStream_t s) {
    IgemmParams p;
    if (int rc = igemm_setup_linear(&p, A, lda, W, K, bias, C, ldc, M, N, K)) return rc;
    p.R = R;
    p.ldr = ldr;
    p.splits = 1;
    IgemmPlan plan = {};
    plan.kernel = IGEMM_TILE;
    plan.bn = kPinBn;
    plan.splits = 1;
    plan.rowstat_cols = kPinBn / 2;
    plan.gather = false;
    plan.epilogue = EPI_LINEAR;
    return launch_igemm(p, plan, s);
}

// contiguous operands: lda = K, ldr = ldc = N
inline int pinned_linear(const half_t* A, const half_t* W, const float* bias, const half_t* R, half_t* C, int M, int N, int K, hipStream_t s) {
    return pinned_linear(A, K, W, bias, R, N, C, N, M, N, K, s);
}

}  // namespace lavie
