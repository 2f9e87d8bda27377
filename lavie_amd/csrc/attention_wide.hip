// Fused attention core for WIDE heads (head dim 512, 256): the single-head self-attention of the AutoencoderKL mid block
// (lavie_amd/vae_hip.py), O = softmax(scale * Q K^T) V per (batch entry, head) with the contract of attention.hip: fp16
// operands, fp32 accumulation, fp32 online softmax, any Lq / Lk >= 1, independent row strides (q | k | v may be column
// slices of one fused tensor), kv_batch_div, no atomics.
//
// Scheme (the one of attention.hip: S^T = K Q^T with the query on the lane, P^T is the B operand of O^T = V^T P^T), laid out
// for a head that fills the register file:
//  * workgroup = 4 waves = one per SIMD, 32 queries per wave (128 per workgroup).  Per lane that is DH / 4 registers of Q
//    fragments and DH / 2 of O accumulators: 128 + 256 of the 512 a lone wave has at head dim 512.  16 queries per wave
//    would halve the FLOP per LDS byte, 48 do not fit;
//  * key tiles of 32 keys, rows of exactly DH * 2 bytes in LDS (no padding).  K and V have a ring of two tiles each
//    (4 x 32 KiB at head dim 512) and are staged HBM / L2 -> LDS with global_load_lds_dwordx4; the loads alternate
//    K0 V0 K1 V1 ..., the waits are counted, and a tile is asked for 1.5 tiles of compute before it is read: K(t+2) when
//    every wave has finished the scores of tile t, V(t+1) when every wave has finished P V of tile t-1;
//  * bank conflicts are removed by an XOR on the 16-byte chunk index, chunk' = chunk ^ ((key & 7) << 1), applied to the
//    per-lane SOURCE address of the LDS-DMA (its LDS side is lane-linear) and to both kinds of read: the ds_read_b128 K
//    fragments (16 keys x one chunk per lane group: sixteen distinct slots of the 256-byte bank row) and the
//    ds_read_b64_tr_b16 V^T fragments (8 keys x 32 bytes per 32-lane half: eight distinct slot pairs);
//  * online softmax with a deferred rescale (attention.hip's RESCALE_THR).  The FIRST tile only sets the running maximum:
//    O and l are still zero, so nothing is rescaled there, and a first tile whose scores all sit far below zero cannot
//    produce 0 * inf;
//  * workgroups are numbered so that the CUs of one XCD take a contiguous run of query blocks of the same (batch, head):
//    the workgroups that run together start together and walk the keys together, so a K / V tile is fetched into an L2 once
//    for the 32 CUs behind it.
#include <utility>

#include "attention_frag.h"
#include "profile.h"

namespace lavie {

constexpr int AW_KEYS = 32;           // keys per tile
constexpr int AW_QT = 2;              // 16-query tiles per wave
constexpr int AW_WAVES = 4;
constexpr int AW_QBLK = AW_WAVES * AW_QT * 16;

template <int DH>
struct AwTile {
    static constexpr int RS = DH * 2;                    // row bytes in LDS
    static constexpr int CH = DH / 8;                    // 16-byte chunks per row
    static constexpr int KPP = 64 / CH;                  // keys per 1-KiB LDS-DMA piece
    static constexpr int TILE_BYTES = AW_KEYS * RS;
    static constexpr int PIECES = TILE_BYTES / 1024 / AW_WAVES;     // pieces per wave and operand tile
    static constexpr int KS = DH / 32, DT = DH / 16;
    static constexpr int NG = DT / 4;                    // P V groups of four output tiles
    static constexpr int LDS_BYTES = 4 * TILE_BYTES + 4096;     // K ring (2 tiles), V ring (2 tiles), 16 B per lane for rescales
    static_assert(CH == 64 || CH == 32, "head dims 512 / 256");
};

// The file is built with the MFMA results in AGPRs (no -amdgpu-mfma-vgpr-form): at head dim 512 the O accumulators are all
// 256 of them, and the Q fragments, scores and K / V fragments need the 256 VGPRs.  The score tiles must then stay out of
// the AGPRs, so their MFMAs are inline asm on VGPRs: in place (vDst = SrcC), in program order, and the vector ALU reads the
// scores behind aw_drain_scores (the compiler pads no hazards around asm).
__device__ __forceinline__ void aw_mfma_v(f32x4& acc, const half8_t& a, const half8_t& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void aw_mfma_v0(f32x4& acc, const half8_t& a, const half8_t& b) {      // first k-step: C = 0
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
// Score product, step N = 2 ks + kt (k-step ks of key block kt): K fragments come AW_KDEPTH steps ahead through a ring of
// registers; the counted wait leaves the younger reads in flight and the fragment passes through it.  (Left to the
// compiler, every ds_read_b128 was followed by lgkmcnt(0) and its two MFMAs.)
constexpr int AW_KDEPTH = 6;
template <int DH, int N>
__device__ __forceinline__ void aw_qk_read(const unsigned (&ka)[4], u32x4_t (&kf)[AW_KDEPTH]) {
    constexpr int ks = N >> 1, kt = N & 1;
    kf[N % AW_KDEPTH] = lds_read_b128_asm<(ks >> 2) * 256 + kt * 16 * AwTile<DH>::RS>(ka[ks & 3]);
}
template <int DH, int N>
__device__ __forceinline__ void aw_qk(const unsigned (&ka)[4], u32x4_t (&kf)[AW_KDEPTH], f32x4 (&s)[2][AW_QT],
                                      const half8_t (&qf)[AW_QT][AwTile<DH>::KS]) {
    constexpr int NS = 2 * AwTile<DH>::KS, ks = N >> 1, kt = N & 1;
    constexpr int LEFT = NS - 1 - N < AW_KDEPTH - 1 ? NS - 1 - N : AW_KDEPTH - 1;
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(kf[N % AW_KDEPTH]) : "n"(LEFT) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    half8_t a;
    __builtin_memcpy(&a, &kf[N % AW_KDEPTH], 16);
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt) {
        if constexpr (ks == 0) aw_mfma_v0(s[kt][qt], a, qf[qt][ks]);
        else aw_mfma_v(s[kt][qt], a, qf[qt][ks]);
    }
    if constexpr (N + AW_KDEPTH < NS) aw_qk_read<DH, N + AW_KDEPTH>(ka, kf);
    if constexpr (N + 1 < NS) aw_qk<DH, N + 1>(ka, kf, s, qf);
}
template <int DH, int... Ns>
__device__ __forceinline__ void aw_qk_prime(const unsigned (&ka)[4], u32x4_t (&kf)[AW_KDEPTH], std::integer_sequence<int, Ns...>) {
    (aw_qk_read<DH, Ns>(ka, kf), ...);
}
// O accumulators: only ever touched as whole AGPR tuples by inline asm inside the key loop (see the kernel)
__device__ __forceinline__ void aw_mfma_a(f32x4& acc, const half8_t& a, const half8_t& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void aw_zero_a(f32x4& acc, const half8_t& zero) {      // 0 * 0 + 0
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %1, 0" : "=a"(acc) : "v"(zero));
}
// acc *= alpha through a 16-byte LDS slot of the lane (rare path: the vector ALU cannot read an AGPR tuple in place)
__device__ __forceinline__ void aw_scale_a(f32x4& acc, float alpha, unsigned slot) {
    f32x4 t;
    asm volatile("ds_write_b128 %1, %2\n\tds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(t) : "v"(slot), "a"(acc) : "memory");
    t *= alpha;
    asm volatile("ds_write_b128 %1, %2\n\tds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=a"(acc) : "v"(slot), "v"(t) : "memory");
}
__device__ __forceinline__ void aw_drain_scores(f32x4 (&s)[2][AW_QT]) {
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(s[0][0]), "+v"(s[0][1]), "+v"(s[1][0]), "+v"(s[1][1]));
}

// V^T fragments of output tiles dt = (G >> 1) * 8 + (G & 1) * 4 + j, j = 0..3: keys +0..15 (lo) and +16..31 (hi)
template <int DH, int G>
__device__ __forceinline__ void aw_read_v(const unsigned (&va)[8], u32x2_t (&lo)[4], u32x2_t (&hi)[4]) {
    constexpr int OFF = (G >> 1) * 256, RS = AwTile<DH>::RS;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[j] = lds_read_tr16_asm<OFF>(va[(G & 1) * 4 + j]);
        hi[j] = lds_read_tr16_asm<OFF + 16 * RS>(va[(G & 1) * 4 + j]);
    }
}

// group G of the P V product: the reads of group G + 1 are issued first, the counted wait leaves exactly those in flight and
// the fragments of group G pass THROUGH it, so no MFMA that reads them can be scheduled above it
template <int DH, int G>
__device__ __forceinline__ void aw_pv(const unsigned (&va)[8], u32x2_t (&lo)[4], u32x2_t (&hi)[4],
                                      f32x4 (&o)[AwTile<DH>::DT][AW_QT], const half8_t (&pb)[AW_QT]) {
    constexpr bool MORE = G + 1 < AwTile<DH>::NG;
    u32x2_t nlo[4], nhi[4];
    if constexpr (MORE) {
        aw_read_v<DH, G + 1>(va, nlo, nhi);
        asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]), "+v"(lo[2]), "+v"(hi[2]), "+v"(lo[3]), "+v"(hi[3])::"memory");
    } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]), "+v"(lo[2]), "+v"(hi[2]), "+v"(lo[3]), "+v"(hi[3])::"memory");
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        constexpr int DT0 = (G >> 1) * 8 + (G & 1) * 4;
        half8_t vf;
        __builtin_memcpy(&vf, &lo[j], 8);
        __builtin_memcpy(reinterpret_cast<char*>(&vf) + 8, &hi[j], 8);
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) aw_mfma_a(o[DT0 + j][qt], vf, pb[qt]);
    }
    if constexpr (MORE) aw_pv<DH, G + 1>(va, nlo, nhi, o, pb);
}

template <int DH>
__global__ __launch_bounds__(64 * AW_WAVES, 1) void attention_wide_kernel(const AttnParams p, const int nqblk) {
    using T = AwTile<DH>;
    constexpr int RS = T::RS, CH = T::CH, KPP = T::KPP, PIECES = T::PIECES;
    extern __shared__ __attribute__((aligned(1024))) char smem[];     // K ring at 0, V ring at 2 * TILE_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;       // 16-lane group
    const int li = lane & 15;

    // workgroup order: blockIdx % 8 labels the blocks that share an XCD; give each label a contiguous run of the
    // (batch, head, query block) list, query block fastest (bijective for any grid size)
    int qblk, head, qb;
    {
        const int nwg = gridDim.x, bid = blockIdx.x;
        const int xq = nwg >> 3, xr = nwg & 7, x = bid & 7;
        const int w = (x < xr ? x * (xq + 1) : xr * (xq + 1) + (x - xr) * xq) + (bid >> 3);
        const int bh = w / nqblk;
        // (wave-uniform, but the divisions run on the vector ALU: back to SGPRs, so that what is derived from them is scalar)
        qblk = __builtin_amdgcn_readfirstlane(w % nqblk);
        head = __builtin_amdgcn_readfirstlane(bh % p.heads);
        qb = __builtin_amdgcn_readfirstlane(bh / p.heads);
    }
    const int kvb = qb / p.kv_batch_div;
    const int q0 = qblk * AW_QBLK + wave * (AW_QT * 16);

    // ---- Q fragments (B operand): lane holds Q[q = li][dims 32 ks + 8 g .. +7]
    half8_t qf[AW_QT][T::KS];
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt) {
        int q = q0 + qt * 16 + li;
        q = q < p.Lq ? q : p.Lq - 1;
        const half_t* qrow = p.q + ((size_t)qb * p.Lq + q) * p.ldq + head * DH;
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) qf[qt][ks] = *reinterpret_cast<const half8_t*>(qrow + ks * 32 + g * 8);
    }

    const half_t* kbase = p.k + (size_t)kvb * p.Lk * p.ldk + head * DH;
    const half_t* vbase = p.v + (size_t)kvb * p.Lk * p.ldv + head * DH;
    // ---- LDS-DMA: piece x = wave * PIECES + i of a tile is keys x * KPP .. + KPP - 1; lane l writes chunk l % CH of key
    // x * KPP + l / CH and fetches the chunk that the swizzle puts there
    const int dkey0 = lane / CH;                                     // key of the lane inside a piece
    const int dch0 = lane % CH;
    auto issue_tile = [&](const half_t* base, int ld, int key0, char* dst) {
        // (opaque per call: hoisted out of the key loop, the pieces' source addresses cost 4 * PIECES registers)
        int dkey = dkey0, dch = dch0;
        asm volatile("" : "+v"(dkey), "+v"(dch));
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int x = wave * PIECES + i;
            const int kl = x * KPP + dkey;                           // key row inside the tile
            int key = key0 + kl;
            key = key < p.Lk ? key : p.Lk - 1;                       // keys past Lk: any finite row (their scores are masked)
            const half_t* src = base + (size_t)key * ld + ((dch ^ ((kl & 7) << 1)) << 3);
            __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(dst + x * 1024), 16, 0, 0);
        }
    };

    f32x4 o[T::DT][AW_QT];
#pragma unroll
    for (int dt = 0; dt < T::DT; ++dt)
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) aw_zero_a(o[dt][qt], (half8_t){0, 0, 0, 0, 0, 0, 0, 0});
    const unsigned oslot = (unsigned)(size_t)LDS_PTR(smem + T::LDS_BYTES - 4096) + tid * 16;      // behind the rings
    float m_run[AW_QT], l_run[AW_QT];      // running max (log2 units, scaled) and per-lane partial row sums
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt) { m_run[qt] = 0.f; l_run[qt] = 0.f; }

    const float sl2 = p.scale * 1.4426950408889634f;   // softmax scale folded with log2(e): p = exp2(s * sl2 - m)
    const int ntile = cdiv(p.Lk, AW_KEYS);

    // read addresses inside a tile.  K fragment of key block kt, k-step ks: key li, chunk 4 ks + g; the XOR touches chunk
    // bits 1..3, the k-step bits 2..5: four bases (ks & 3), the rest is an immediate.  V^T fragment of output tile dt: lane
    // 4 q + p of a group addresses key 4 g + q, chunk 2 dt + (p >> 1), byte 8 (p & 1): eight bases (dt & 7)
    unsigned ka[4], va[8];
    {
        const unsigned kb = li * RS + (((unsigned)g ^ ((li & 7) << 1)) << 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) ka[j] = kb ^ (j << 6);
        const int vkey = g * 4 + (li >> 2);
        const unsigned vb = vkey * RS + (((unsigned)((li & 3) >> 1) ^ ((vkey & 7) << 1)) << 4) + (li & 1) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) va[j] = vb ^ (j << 5);
    }

    // the Q loads are consumed HERE, before any LDS-DMA is in flight (attention.hip: otherwise their wait lands in the
    // loop as vmcnt(0))
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt)
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) asm volatile("" : "+v"(qf[qt][ks]));
    issue_tile(kbase, p.ldk, 0, smem);
    issue_tile(vbase, p.ldv, 0, smem + 2 * T::TILE_BYTES);
    if (ntile > 1) issue_tile(kbase, p.ldk, AW_KEYS, smem + T::TILE_BYTES);

    for (int t = 0; t < ntile; ++t) {
        const int slot = t & 1;
        // ---- K(t) has landed: behind it in the queue are V(t) and, when it exists, K(t+1)
        if (t + 1 < ntile) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // every wave has finished P V of tile t-1: its V slot takes V(t+1)
        if (t + 1 < ntile) issue_tile(vbase, p.ldv, (t + 1) * AW_KEYS, smem + (2 + (slot ^ 1)) * T::TILE_BYTES);

        // ---- S^T[key, q] = K Q^T
        f32x4 s[2][AW_QT];
        {
            const unsigned ktile = (unsigned)(size_t)LDS_PTR(smem + slot * T::TILE_BYTES);
            unsigned kat[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) kat[j] = ka[j] + ktile;
            u32x4_t kf[AW_KDEPTH];
            aw_qk_prime<DH>(kat, kf, std::make_integer_sequence<int, AW_KDEPTH>{});
            aw_qk<DH, 0>(kat, kf, s, qf);
        }
        aw_drain_scores(s);

        // ---- keys past Lk exist only in the last tile (wave-uniform branch)
        const int kleft = p.Lk - t * AW_KEYS;
        if (kleft < AW_KEYS) {
#pragma unroll
            for (int qt = 0; qt < AW_QT; ++qt)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt * 16 + g * 4 + r >= kleft) s[kt][qt][r] = -INFINITY;
        }

        // ---- online softmax per query column (lane li of each 16-lane group), deferred rescale
        half8_t pb[AW_QT];
        float mxl[AW_QT];
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) {
            mxl[qt] = att_lane_max<false>(s, qt) * sl2;          // (scale > 0)
        }
        bool grow = t == 0;
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) grow = grow || mxl[qt] > m_run[qt] + RESCALE_THR;
        if (__builtin_amdgcn_ballot_w64(grow) != 0) {
#pragma unroll
            for (int qt = 0; qt < AW_QT; ++qt) {
                const float mx = att_group_max(mxl[qt]);        // over the four lane groups that hold the query's 32 keys
                if (t == 0) {
                    // first tile: O and l are zero, nothing to rescale; the tile holds at least one real key, so mx is finite
                    m_run[qt] = mx;
                } else {
                    const float m_new = fmaxf(m_run[qt], mx);
                    const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);     // m_run is finite: alpha in [0, 1]
                    m_run[qt] = m_new;
                    l_run[qt] *= alpha;
#pragma unroll
                    for (int dt = 0; dt < T::DT; ++dt) aw_scale_a(o[dt][qt], alpha, oslot);
                }
            }
        }
#pragma unroll
        for (int qt = 0; qt < AW_QT; ++qt) {
            const float nm = -m_run[qt];
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                float e[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][qt][r], sl2, nm));
                    psum += e[r];
                }
                att_pack4(pb[qt], kt, e[0], e[1], e[2], e[3]);
            }
            l_run[qt] += psum;           // per-lane partial; reduced over g at the end
        }

        // ---- V(t) has landed: behind it are K(t+1) and V(t+1) when they exist
        if (t + 1 < ntile) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // every wave has finished the scores of tile t: its K slot takes K(t+2)
        if (t + 2 < ntile) issue_tile(kbase, p.ldk, (t + 2) * AW_KEYS, smem + slot * T::TILE_BYTES);

        // ---- O^T[dim, q] += V^T P^T  (V^T fragments by hardware-transposed LDS reads, inline asm: a compiler-issued 8-byte
        // LDS read beside LDS-DMA in flight gets a vmcnt(0) in front of it)
        {
            const unsigned vtile = (unsigned)(size_t)LDS_PTR(smem + (2 + slot) * T::TILE_BYTES);
            unsigned vat[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) vat[j] = va[j] + vtile;
            u32x2_t lo[4], hi[4];
            aw_read_v<DH, 0>(vat, lo, hi);
            aw_pv<DH, 0>(vat, lo, hi, o, pb);
        }
    }

    // the accumulators were written by MFMAs the compiler does not see as such: drain the matrix pipe before they are read
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
    // ---- normalise and store: lane holds dims dt * 16 + 4 g .. +3 of query li
#pragma unroll
    for (int qt = 0; qt < AW_QT; ++qt) {
        __builtin_amdgcn_sched_barrier(0);      // one query tile's accumulators out of the AGPRs at a time
        const float inv = 1.0f / att_sum_groups(l_run[qt]);
        // (the lane index is taken afresh: kept from the top of the kernel for this use alone, it is spilled across the key loop)
        unsigned zero = 0;
        asm volatile("" : "+v"(zero));
        const int le = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));     // = lane
        const int ge = le >> 4;
        const int q = q0 + qt * 16 + (le & 15);
        if (q < p.Lq) {
            half_t* orow = p.o + ((size_t)qb * p.Lq + q) * p.ldo + head * DH;
#pragma unroll
            for (int dt = 0; dt < T::DT; ++dt) {
                const f32x4 v = o[dt][qt];
                half4_t h = {(half_t)(v[0] * inv), (half_t)(v[1] * inv), (half_t)(v[2] * inv), (half_t)(v[3] * inv)};
                *reinterpret_cast<half4_t*>(orow + dt * 16 + ge * 4) = h;
            }
        }
    }
}

template <int DH>
static int launch_att_wide(const AttnParams& p, hipStream_t stream) {
    using T = AwTile<DH>;
    auto kern = attention_wide_kernel<DH>;
    if (int rc = ensure_dynamic_lds((const void*)kern, T::LDS_BYTES)) return rc;
    const int nqblk = cdiv(p.Lq, AW_QBLK);
    const long long nwg = (long long)nqblk * p.heads * p.NBq;
    LAVIE_CHECK(nwg <= 0x7fffffffLL, "attention: problem too large (%lld workgroups)", nwg);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(64 * AW_WAVES), T::LDS_BYTES, stream, p, nqblk);
    LAVIE_HIP(hipGetLastError());
    return 0;
}

// head dims 256 / 512 (launch_attention has checked everything else and opened the profile scope)
int launch_attention_wide(const AttnParams& p, hipStream_t stream) {
    if (p.dh == 512) return launch_att_wide<512>(p, stream);
    return launch_att_wide<256>(p, stream);
}

}  // namespace lavie
