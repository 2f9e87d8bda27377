// Low-rank adapter merge (LoRA on the attention projections): out = fp16_rne(W0 + scale * B A), A / B in fp32.
// Memory-bound: 4 B of W0 / out traffic per element against 2 r FLOP.  A workgroup owns a 32-row x 64-column tile of W0; the
// rank runs in chunks of 32 through LDS (the A columns and B rows of the tile), so every r in 1..128 uses the same 12 KB.
// Each thread keeps 8 consecutive columns of one row in registers and accumulates them in ascending j with fmaf: the sum
// order is fixed and nothing is shared between threads, so two runs give the same bits.
// The multi-term kernel blends up to kLoraMaxTerms adapters in one pass: t = float(W0); t = fmaf(eff_i, acc_i, t) term after term in
// list order, then one conversion of the finished fp32 sum to fp16.  Same tile, same LDS (reused term after term), W0 read and out
// written once per element.  A list with one live term goes to the single kernel (launch_lora_merge_multi).
#include "ops.h"

namespace lavie {

namespace {
constexpr int kTileN = 32, kTileK = 64, kChunkR = 32;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const half_t* W0, const float* __restrict__ A,
                                                         const float* __restrict__ B, half_t* out, int N, int K,
                                                         int r, float scale) {
    __shared__ float sA[kChunkR][kTileK];        // A[j0 + j][k0 + c]
    __shared__ float sB[kTileN][kChunkR + 1];    // B[n0 + i][j0 + j]
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * kTileK, n0 = blockIdx.y * kTileN;
    const int row = tid >> 3, col = (tid & 7) * 8;        // this thread's 8 outputs: row n0 + row, columns k0 + col .. + 7
    const int n = n0 + row, k = k0 + col;
    const bool live = n < N && k < K;                     // K % 8 == 0: the 8 columns are all in or all out
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int j0 = 0; j0 < r; j0 += kChunkR) {
        const int jn = min(kChunkR, r - j0);
        // A chunk: jn rows of 64 columns as float4 (K % 8 == 0 keeps whole float4s inside or outside the matrix)
        for (int e = tid; e < kChunkR * (kTileK / 4); e += 256) {
            const int j = e / (kTileK / 4), c4 = (e % (kTileK / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j < jn && k0 + c4 < K) v = *(const f32x4*)(A + (size_t)(j0 + j) * K + k0 + c4);
            *(f32x4*)&sA[j][c4] = v;
        }
        for (int e = tid; e < kTileN * kChunkR; e += 256) {
            const int i = e / kChunkR, j = e % kChunkR;
            sB[i][j] = (j < jn && n0 + i < N) ? B[(size_t)(n0 + i) * r + j0 + j] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            const float b = sB[row][j];
            const f32x4 a0 = *(const f32x4*)&sA[j][col];
            const f32x4 a1 = *(const f32x4*)&sA[j][col + 4];
            acc[0] = fmaf(b, a0.x, acc[0]); acc[1] = fmaf(b, a0.y, acc[1]);
            acc[2] = fmaf(b, a0.z, acc[2]); acc[3] = fmaf(b, a0.w, acc[3]);
            acc[4] = fmaf(b, a1.x, acc[4]); acc[5] = fmaf(b, a1.y, acc[5]);
            acc[6] = fmaf(b, a1.z, acc[6]); acc[7] = fmaf(b, a1.w, acc[7]);
        }
        __syncthreads();
    }
    if (!live) return;
    const size_t off = (size_t)n * K + k;
    const half8_t w = *(const half8_t*)(W0 + off);
    half8_t o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (half_t)fmaf(scale, acc[i], (float)w[i]);     // one rounding to fp16 (RNE)
    *(half8_t*)(out + off) = o;
}

int launch_lora_merge(const half_t* W0, const float* A, const float* B, half_t* out, int N, int K, int r, float scale,
                      hipStream_t stream) {
    LAVIE_CHECK(W0 && A && B && out, "lora_merge: null tensor");
    LAVIE_CHECK(N >= 1 && K >= 8 && K % 8 == 0, "lora_merge: N=%d K=%d (K must be a positive multiple of 8)", N, K);
    LAVIE_CHECK(r >= 1 && r <= kLoraMaxRank, "lora_merge: rank %d outside 1..%d", r, kLoraMaxRank);
    LAVIE_CHECK(((uintptr_t)W0 | (uintptr_t)out | (uintptr_t)A) % 16 == 0, "lora_merge: W0 / out / A must be 16-byte aligned");
    LAVIE_CHECK(__builtin_isfinite(scale), "lora_merge: scale is not finite");
    hipLaunchKernelGGL(lora_merge_kernel, dim3(cdiv(K, kTileK), cdiv(N, kTileN)), dim3(256), 0, stream, W0, A, B, out, N, K, r,
                       scale);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

// The term list travels by value in the kernel arguments (8 x 24 bytes): no device-side table, nothing to allocate or copy per launch.
struct LoraTermList {
    LoraTerm t[kLoraMaxTerms];      // `scale` holds the effective factor; a zero factor never gets here
};

// fp16_rne of a FINISHED fp32 value.  The empty asm emits nothing; it keeps the compiler from contracting the fmaf that produced v
// with the conversion (gfx950 has v_fma_mixlo / mixhi_f16, which round the exact sum once to fp16 and differ from fp32-then-fp16 in
// about one element in 10^4): the multi-term sum is rounded in this one form in every column, whatever the compiler would pick.
__device__ __forceinline__ half_t round_f16(float v) {
    asm volatile("" : "+v"(v));
    return (half_t)v;
}

__global__ __launch_bounds__(256) void lora_merge_multi_kernel(const half_t* W0, LoraTermList terms, int n_terms, half_t* out, int N,
                                                               int K) {
    __shared__ float sA[kChunkR][kTileK];        // A_i[j0 + j][k0 + c]
    __shared__ float sB[kTileN][kChunkR + 1];    // B_i[n0 + i][j0 + j]
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * kTileK, n0 = blockIdx.y * kTileN;
    const int row = tid >> 3, col = (tid & 7) * 8;
    const int n = n0 + row, k = k0 + col;
    const bool live = n < N && k < K;                     // K % 8 == 0: the 8 columns are all in or all out
    const size_t off = (size_t)n * K + k;
    float t[8];                                           // the running sum, float(W0) first: read once, before any term
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = 0.f;
    if (live) {
        const half8_t w = *(const half8_t*)(W0 + off);
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = (float)w[i];
    }
    for (int ti = 0; ti < n_terms; ++ti) {
        const float* __restrict__ A = terms.t[ti].A;
        const float* __restrict__ B = terms.t[ti].B;
        const int r = terms.t[ti].r;
        const float eff = terms.t[ti].scale;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int j0 = 0; j0 < r; j0 += kChunkR) {         // the chain of lora_merge_kernel, operation for operation
            const int jn = min(kChunkR, r - j0);
            for (int e = tid; e < kChunkR * (kTileK / 4); e += 256) {
                const int j = e / (kTileK / 4), c4 = (e % (kTileK / 4)) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (j < jn && k0 + c4 < K) v = *(const f32x4*)(A + (size_t)(j0 + j) * K + k0 + c4);
                *(f32x4*)&sA[j][c4] = v;
            }
            for (int e = tid; e < kTileN * kChunkR; e += 256) {
                const int i = e / kChunkR, j = e % kChunkR;
                sB[i][j] = (j < jn && n0 + i < N) ? B[(size_t)(n0 + i) * r + j0 + j] : 0.f;
            }
            __syncthreads();
            for (int j = 0; j < jn; ++j) {
                const float b = sB[row][j];
                const f32x4 a0 = *(const f32x4*)&sA[j][col];
                const f32x4 a1 = *(const f32x4*)&sA[j][col + 4];
                acc[0] = fmaf(b, a0.x, acc[0]); acc[1] = fmaf(b, a0.y, acc[1]);
                acc[2] = fmaf(b, a0.z, acc[2]); acc[3] = fmaf(b, a0.w, acc[3]);
                acc[4] = fmaf(b, a1.x, acc[4]); acc[5] = fmaf(b, a1.y, acc[5]);
                acc[6] = fmaf(b, a1.z, acc[6]); acc[7] = fmaf(b, a1.w, acc[7]);
            }
            __syncthreads();                              // the next chunk, or the next term, overwrites the tiles
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = fmaf(eff, acc[i], t[i]);
    }
    if (!live) return;
    half8_t o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = round_f16(t[i]);
    *(half8_t*)(out + off) = o;
}

int launch_lora_merge_multi(const half_t* W0, const LoraTerm* terms, int n_terms, half_t* out, int N, int K, hipStream_t stream) {
    LAVIE_CHECK(W0 && terms && out, "lora_merge_multi: null tensor");
    LAVIE_CHECK(n_terms >= 1 && n_terms <= kLoraMaxTerms, "lora_merge_multi: %d terms outside 1..%d", n_terms, kLoraMaxTerms);
    LAVIE_CHECK(N >= 1 && K >= 8 && K % 8 == 0, "lora_merge_multi: N=%d K=%d (K must be a positive multiple of 8)", N, K);
    LAVIE_CHECK(((uintptr_t)W0 | (uintptr_t)out) % 16 == 0, "lora_merge_multi: W0 / out must be 16-byte aligned");
    LoraTermList list = {};
    int live = 0;
    for (int i = 0; i < n_terms; ++i) {
        const LoraTerm& t = terms[i];
        LAVIE_CHECK(t.A && t.B, "lora_merge_multi: term %d: null tensor", i);
        LAVIE_CHECK(t.r >= 1 && t.r <= kLoraMaxRank, "lora_merge_multi: term %d: rank %d outside 1..%d", i, t.r, kLoraMaxRank);
        LAVIE_CHECK((uintptr_t)t.A % 16 == 0, "lora_merge_multi: term %d: A must be 16-byte aligned", i);
        LAVIE_CHECK(__builtin_isfinite(t.scale), "lora_merge_multi: term %d: scale is not finite", i);
        if (t.scale != 0.f) list.t[live++] = t;           // a zero factor is not a term: it cannot change a bit
    }
    if (live == 0) {                                      // nothing to add: the base, exactly
        if (out != W0) LAVIE_HIP(hipMemcpyAsync(out, W0, (size_t)N * K * sizeof(half_t), hipMemcpyDeviceToDevice, stream));
        return 0;
    }
    if (live == 1)      // one term IS the single merge: its kernel, hence its bits, however the compiler rounded its last step
        return launch_lora_merge(W0, list.t[0].A, list.t[0].B, out, N, K, list.t[0].r, list.t[0].scale, stream);
    hipLaunchKernelGGL(lora_merge_multi_kernel, dim3(cdiv(K, kTileK), cdiv(N, kTileN)), dim3(256), 0, stream, W0, list, live, out, N,
                       K);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

}  // namespace lavie
