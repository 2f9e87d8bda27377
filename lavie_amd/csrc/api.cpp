// extern "C" surface of liblavie_hip.so (declared in include/lavie_hip.h).
#include <string.h>

#include <new>

#include "engine.h"
#include "image_engine.h"
#include "profile.h"
#include "r3d_engine.h"
#include "text_engine.h"

using namespace lavie;

struct lavie_unet_s {
    UNet net;
    explicit lavie_unet_s(const lavie_unet_config& c) : net(c) {}
};

struct lavie_text_s {
    TextEncoder enc;
    explicit lavie_text_s(const lavie_text_config& c) : enc(c) {}
};

struct lavie_vision_s {
    VisionEncoder enc;
    explicit lavie_vision_s(const lavie_vision_config& c) : enc(c) {}
};

struct lavie_mapper_s {
    ImageMapper enc;
    explicit lavie_mapper_s(const lavie_mapper_config& c) : enc(c) {}
};

struct lavie_r3d_s {
    R3dEngine enc;
};

static inline hipStream_t S(void* s) { return (hipStream_t)s; }

// The lifecycle of the text, vision and mapper handles, written once: Handle is lavie_<name>_s, Cfg its lavie_<name>_config
template <class Handle, class Cfg>
static int encoder_create(const char* name, const Cfg* cfg, Handle** out) {
    LAVIE_CHECK(cfg && out, "%s_create: null argument", name);
    LAVIE_CHECK(cfg->struct_size == (int)sizeof(Cfg),
                "%s_create: cfg->struct_size=%d but this library's lavie_%s_config has %d bytes (ABI %d): the binding's struct "
                "layout is out of date", name, cfg->struct_size, name, (int)sizeof(Cfg), LAVIE_ABI_VERSION);
    Handle* h = new (std::nothrow) Handle(*cfg);
    LAVIE_CHECK(h != nullptr, "%s_create: out of host memory", name);
    if (int rc = h->enc.validate_config()) {
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

template <class Handle>
static int encoder_destroy(Handle* h) {
    delete h;
    return 0;
}

template <class Handle>
static int encoder_num_params(Handle* h) {
    return h ? (int)h->enc.params().size() : -1;
}

template <class Handle>
static int encoder_param_info(const char* name, Handle* h, int i, const char** pname, long long* numel) {
    LAVIE_CHECK(h && i >= 0 && i < (int)h->enc.params().size(), "%s_param_info: index %d out of range", name, i);
    if (pname) *pname = h->enc.params()[i].name.c_str();
    if (numel) *numel = h->enc.params()[i].numel;
    return 0;
}

template <class Handle>
static int encoder_set_param(const char* name, Handle* h, const char* key, const void* data_f16, long long numel) {
    LAVIE_CHECK(h && key, "%s_set_param: null argument", name);
    return h->enc.set_param(key, data_f16, numel);
}

template <class Handle>
static int encoder_finalize(const char* name, Handle* h, void* stream) {
    LAVIE_CHECK(h, "%s_finalize: null handle", name);
    return h->enc.finalize(S(stream));
}

template <class Handle, class... Shape>
static long long encoder_workspace_bytes(const char* name, Handle* h, Shape... shape) {
    if (!h) {
        set_error("%s_workspace_bytes: null handle", name);
        return -1;
    }
    return h->enc.workspace_bytes(shape...);
}

// Operator-level entry points have no workspace argument: the split-K slab comes from a grow-only scratch
// buffer owned by the library (allocated outside any stream capture; the engine uses its own workspace).
static float* g_slab = nullptr;
static size_t g_slab_bytes = 0;
// The statistics sink of the operator-level GEMM launches (lavie_debug_op_statistics): while armed, op_launch hands the sink's buffers
// to the launch as the engine's run_igemm / linear do, so that the producers' epilogue statistics can be checked per element.  The
// engine never reads it.  g_stats_last: what the last operator launch planned and wrote (lavie_debug_op_statistics_last).
static float* g_sink_cs = nullptr;
static float* g_sink_rs = nullptr;
static long long g_sink_cs_floats = 0, g_sink_rs_floats = 0;
static int g_plan_cs = 0, g_plan_rs = 0;      // lavie_debug_op_statistics_plan: plan as if armed, launch nothing
static lavie_op_statistics_info g_stats_last = {};
static int op_launch(IgemmParams& p, bool gather, int epilogue, hipStream_t stream) {
    const bool plan_only = g_plan_cs || g_plan_rs;
    const bool want_cs = plan_only ? g_plan_cs != 0 : g_sink_cs != nullptr;
    const bool want_rs = (plan_only ? g_plan_rs != 0 : g_sink_rs != nullptr) && !gather && epilogue == EPI_LINEAR && !p.ln_stats;
    static float placeholder;                 // the planner reads which operands are present, never their addresses
    if (want_rs) p.rowstat_out = plan_only ? &placeholder : g_sink_rs;
    IgemmPlan plan = igemm_plan(p, gather, epilogue);
    p.splits = plan.splits;
    lavie_op_statistics_info info = {};
    info.struct_size = (int)sizeof(info);
    info.M = p.M; info.N = p.N; info.splits = plan.splits;
    if (want_cs && plan.colstat_rows > 0) {
        const GnColStat cs = gn_colstat_describe(p, plan, g_sink_cs);
        info.colstat_written = 1;
        info.colstat_rows = cs.rows; info.colstat_span = cs.span; info.nsets = cs.nsets; info.set_blocks = cs.set_blocks;
        info.colstat_contiguous = plan.splits > 1 || plan.kernel == IGEMM_TILE || plan.kernel == IGEMM_PP || plan.kernel == IGEMM_PPX || plan.kernel == IGEMM_PATCH_ROWS ||
                                  plan.kernel == IGEMM_PATCH_PARITY;
        info.colstat_blocks_stored = (long long)gn_colstat_blocks_stored(p, plan);
        info.colstat_floats = info.colstat_blocks_stored * 2 * p.N;
        LAVIE_CHECK(plan_only || g_sink_cs_floats >= info.colstat_floats,
                    "op_statistics: the column-statistics sink holds %lld floats, this launch writes %lld", g_sink_cs_floats, info.colstat_floats);
    }
    if (want_rs) {
        LAVIE_CHECK(plan.rowstat_cols > 0 && p.N % plan.rowstat_cols == 0, "op_statistics: no row-statistics slots for N=%d", p.N);
        info.rowstat_written = 1;
        info.rowstat_cols = plan.rowstat_cols; info.rowstat_slots = p.N / plan.rowstat_cols;
        info.rowstat_floats = (long long)p.M * info.rowstat_slots * 2;
        LAVIE_CHECK(plan_only || g_sink_rs_floats >= info.rowstat_floats,
                    "op_statistics: the row-statistics sink holds %lld floats, this launch writes %lld", g_sink_rs_floats, info.rowstat_floats);
    }
    const int rc = igemm_run(p, gather, epilogue, stream, [](size_t need, float** slab) {
        if (need > g_slab_bytes) {
            if (g_slab) { LAVIE_HIP(hipDeviceSynchronize()); LAVIE_HIP(hipFree(g_slab)); g_slab = nullptr; g_slab_bytes = 0; }
            LAVIE_HIP(hipMalloc((void**)&g_slab, need));
            g_slab_bytes = need;
        }
        *slab = g_slab;
        return 0;
    }, want_cs && !plan_only ? g_sink_cs : nullptr, plan_only);
    if (rc == 0) g_stats_last = info;
    return rc;
}
static inline const half_t* H(const void* p) { return (const half_t*)p; }
static inline half_t* H(void* p) { return (half_t*)p; }

extern "C" {

const char* lavie_last_error(void) { return get_error(); }
int lavie_abi_version(void) { return LAVIE_ABI_VERSION; }

int lavie_linear_f16(const void* A, int lda, const void* W, const float* bias, const float* bias2, int ldb2,
                     int rows_per_batch, const void* R, int ldr, void* C, int ldc, int M, int N, int K, int geglu,
                     void* stream) {
    LAVIE_CHECK(A && W && C, "linear: null tensor");
    LAVIE_CHECK(K % IGEMM_BK == 0, "linear: K=%d must be a multiple of %d", K, IGEMM_BK);
    LAVIE_CHECK(!bias2 || rows_per_batch > 0, "linear: bias2 needs rows_per_batch > 0");
    IgemmParams p;
    if (int rc = igemm_setup_linear(&p, H(A), lda, H(W), K, bias, H(C), ldc, M, N, K)) return rc;
    p.bias2 = bias2; p.ldb2 = ldb2; p.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1;
    p.R = H(R); p.ldr = ldr;
    return op_launch(p, false, geglu ? EPI_GEGLU : EPI_LINEAR, S(stream));
}

// The consumer side of a folded LayerNorm at operator level (engine.cpp's `LnFold`): C = rstd_m (A W'^T - mean_m s) + bias with
// W' = W gamma, s = row sums of W', bias = W beta (+ b) prepared by the caller; stats [M, 2] = (mean, rstd) of the rows of A
int lavie_linear_lnfold_f16(const void* A, const void* Wf, const float* bias, const float* ln_s, const float* ln_stats, void* C,
                            int M, int N, int K, void* stream) {
    LAVIE_CHECK(A && Wf && C && ln_s && ln_stats, "linear_lnfold: null tensor");
    LAVIE_CHECK(K % IGEMM_BK == 0, "linear_lnfold: K=%d must be a multiple of %d", K, IGEMM_BK);
    IgemmParams p;
    if (int rc = igemm_setup_linear(&p, H(A), K, H(Wf), K, bias, H(C), N, M, N, K)) return rc;
    p.ln_s = ln_s; p.ln_stats = ln_stats;
    return op_launch(p, false, EPI_LINEAR, S(stream));      // (unsplit: a LayerNorm fold)
}

// ... with the GEGLU epilogue: the engine's ff1 behind a folded norm3 (engine.cpp `ln_proj(t.ff1, ..., EPI_GEGLU)`).  Wf, bias and ln_s
// are in lavie_pack_geglu_f16's row order (the engine packs all three with one permutation); C [M, N / 2]
int lavie_linear_lnfold_geglu_f16(const void* A, const void* Wf, const float* bias, const float* ln_s, const float* ln_stats, void* C,
                                  int M, int N, int K, void* stream) {
    LAVIE_CHECK(A && Wf && C && ln_s && ln_stats, "linear_lnfold_geglu: null tensor");
    LAVIE_CHECK(K % IGEMM_BK == 0, "linear_lnfold_geglu: K=%d must be a multiple of %d", K, IGEMM_BK);
    LAVIE_CHECK(N > 0 && N % 128 == 0, "linear_lnfold_geglu: N=%d must be a multiple of 128", N);
    IgemmParams p;
    if (int rc = igemm_setup_linear(&p, H(A), K, H(Wf), K, bias, H(C), N / 2, M, N, K)) return rc;
    p.ln_s = ln_s; p.ln_stats = ln_stats;
    return op_launch(p, false, EPI_GEGLU, S(stream));
}

// The encoders' pinned plan (pinned_linear.h) at operator level: the inline function the text encoder, the vision tower and the mapper
// call, behind the refusals check_clip_shape and their workspace carves keep them from needing.  No planner, no force switch, no
// statistics sink: lavie_debug_op_statistics_last does not see this launch.
int lavie_pinned_linear_f16(const void* A, int lda, const void* W, const float* bias, const void* R, int ldr, void* C, int ldc, int M, int N,
                            int K, void* stream) {
    LAVIE_CHECK(A && W && bias && C, "pinned_linear: null tensor");
    LAVIE_CHECK(M >= 1, "pinned_linear: M=%d must be at least 1", M);
    LAVIE_CHECK(N >= kPinBn && N % kPinBn == 0, "pinned_linear: N=%d must be a multiple of %d", N, kPinBn);
    LAVIE_CHECK(K >= IGEMM_BK && K % IGEMM_BK == 0, "pinned_linear: K=%d must be a multiple of %d", K, IGEMM_BK);
    LAVIE_CHECK(lda >= K && lda % 8 == 0, "pinned_linear: lda=%d must be a multiple of 8 and at least K=%d", lda, K);
    LAVIE_CHECK(ldc >= N && ldc % 4 == 0, "pinned_linear: ldc=%d must be a multiple of 4 and at least N=%d", ldc, N);
    LAVIE_CHECK(!R || (ldr >= N && ldr % 4 == 0), "pinned_linear: ldr=%d must be a multiple of 4 and at least N=%d", ldr, N);
    auto aligned = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    LAVIE_CHECK(aligned(A) && aligned(W) && aligned(bias) && aligned(C) && aligned(R), "pinned_linear: the tensors must be 16-byte aligned");
    return pinned_linear(H(A), lda, H(W), bias, H(R), ldr, H(C), ldc, M, N, K, S(stream));
}

int lavie_lora_merge_f16(const void* W0, const float* A, const float* B, void* out, int N, int K, int r, float scale, void* stream) {
    return launch_lora_merge(H(W0), A, B, H(out), N, K, r, scale, S(stream));
}
static_assert(kLoraMaxTerms == LAVIE_LORA_MAX_TERMS, "lavie_lora_term list length");
int lavie_lora_merge_multi_f16(const void* W0, const lavie_lora_term* terms, int n_terms, void* out, int N, int K, void* stream) {
    LAVIE_CHECK(terms, "lora_merge_multi: null term list");
    LAVIE_CHECK(n_terms >= 1 && n_terms <= kLoraMaxTerms, "lora_merge_multi: %d terms outside 1..%d", n_terms, kLoraMaxTerms);
    LoraTerm t[kLoraMaxTerms];
    for (int i = 0; i < n_terms; ++i) t[i] = LoraTerm{terms[i].A, terms[i].B, terms[i].r, terms[i].scale};
    return launch_lora_merge_multi(H(W0), t, n_terms, H(out), N, K, S(stream));
}

long long lavie_freeu_workspace_bytes(int C2, int NI, int H, int W) {
    if (C2 < 8 || C2 % 8 != 0 || NI < 1 || NI > 65535 || H < 1 || W < 1 || (long long)H * W > (1 << 24)) return 0;
    return (long long)(freeu_workspace_floats(C2, NI, H, W) * sizeof(float));
}
int lavie_freeu_f16(const void* h, int C_h, const void* skip, int C2, int NI, int Hh, int W, float b, float s, void* h_out, void* skip_out,
                    void* workspace, void* stream) {
    return launch_freeu(H(h), C_h, H(skip), C2, NI, Hh, W, b, s, H(h_out), H(skip_out), (float*)workspace, S(stream));
}

// FreeInit's frequency mix (freq_mix.hip): everything is checked here before anything is launched; each refusal names its argument.
long long lavie_freq_mix_workspace_bytes(int images, int F, int Hh, int W) {
    return (long long)(freq_mix_workspace_floats(images, F, Hh, W) * sizeof(float));
}
int lavie_freq_mix_f32(const lavie_freq_mix_args* a, void* stream) {
    const char* who = "freq_mix";
    LAVIE_CHECK(a, "%s: args is null", who);
    LAVIE_CHECK(a->struct_size == (int)sizeof(lavie_freq_mix_args),
                "%s: args->struct_size=%d but this library's lavie_freq_mix_args has %d bytes: the binding's struct layout is "
                "out of date", who, a->struct_size, (int)sizeof(lavie_freq_mix_args));
    LAVIE_CHECK(a->images >= 1 && a->images <= kFreqMixMaxImages, "%s: images=%d outside 1..%d", who, a->images, kFreqMixMaxImages);
    LAVIE_CHECK(a->F >= 1 && a->F <= LAVIE_FREQ_MIX_MAX_F, "%s: F=%d outside 1..%d", who, a->F, LAVIE_FREQ_MIX_MAX_F);
    LAVIE_CHECK(a->H >= 1 && a->H <= LAVIE_FREQ_MIX_MAX_HW, "%s: H=%d outside 1..%d", who, a->H, LAVIE_FREQ_MIX_MAX_HW);
    LAVIE_CHECK(a->W >= 1 && a->W <= LAVIE_FREQ_MIX_MAX_HW, "%s: W=%d outside 1..%d", who, a->W, LAVIE_FREQ_MIX_MAX_HW);
    LAVIE_CHECK(a->x0, "%s: x0 is null", who);
    LAVIE_CHECK(a->e0, "%s: e0 is null", who);
    LAVIE_CHECK(a->z, "%s: z is null", who);
    LAVIE_CHECK(a->filter, "%s: filter is null", who);
    LAVIE_CHECK(a->out, "%s: out is null", who);
    LAVIE_CHECK(a->workspace, "%s: workspace is null", who);
    const long long total = (long long)a->images * a->F * a->H * a->W;
    const long long need = lavie_freq_mix_workspace_bytes(a->images, a->F, a->H, a->W);
    LAVIE_CHECK(a->workspace_bytes >= need, "%s: workspace_bytes=%lld, %lld needed", who, a->workspace_bytes, need);
    LAVIE_CHECK(((uintptr_t)a->workspace & 7) == 0, "%s: workspace at %p is not 8-byte aligned", who, a->workspace);
    LAVIE_CHECK(__builtin_isfinite(a->a) && __builtin_isfinite(a->s) && __builtin_isfinite(a->r), "%s: a=%g s=%g r=%g must be finite", who,
                (double)a->a, (double)a->s, (double)a->r);
    if (a->model_in) {
        LAVIE_CHECK(a->dup >= 1 && a->dup <= 3, "%s: dup=%d outside 1..3", who, a->dup);
        LAVIE_CHECK(a->dup_stride >= total && a->dup_stride <= (1ll << 40), "%s: dup_stride=%lld must be >= images F H W = %lld", who,
                    a->dup_stride, total);
        LAVIE_CHECK(__builtin_isfinite(a->input_scale), "%s: input_scale (%g) is not finite", who, (double)a->input_scale);
    }
    // out is written while z is still being read, and after e0 / filter / the workspace have been: it may be x0 and nothing else
    const uintptr_t ob = (uintptr_t)a->out, oe = ob + (uintptr_t)total * 4;
    auto overlaps = [&](const void* p, long long bytes) { return (uintptr_t)p < oe && ob < (uintptr_t)p + (uintptr_t)bytes; };
    LAVIE_CHECK(!overlaps(a->e0, total * 4), "%s: out and e0 overlap (aliasing)", who);
    LAVIE_CHECK(!overlaps(a->z, total * 4), "%s: out and z overlap (aliasing)", who);
    LAVIE_CHECK(!overlaps(a->filter, total / a->images * 4), "%s: out and filter overlap (aliasing)", who);
    LAVIE_CHECK(!overlaps(a->workspace, need), "%s: out and workspace overlap (aliasing)", who);
    LAVIE_CHECK(a->out == a->x0 || !overlaps(a->x0, total * 4), "%s: out and x0 overlap without being equal (aliasing)", who);
    FreqMixParams p{};
    p.x0 = a->x0; p.e0 = a->e0; p.z = a->z; p.filter = a->filter;
    p.a = a->a; p.s = a->s; p.r = a->r;
    p.out = a->out;
    p.model_in = (half_t*)a->model_in;
    p.dup = a->dup; p.dup_stride = a->dup_stride; p.in_scale = a->input_scale;
    p.workspace = (float*)a->workspace;
    p.images = a->images; p.F = a->F; p.H = a->H; p.W = a->W;
    return launch_freq_mix(p, S(stream));
}

long long lavie_geglu_mlp_image_bytes(int C) { return geglu_mlp_supported(C) ? (long long)geglu_mlp_image_bytes(C) : 0; }
long long lavie_geglu_mlp_bias_floats(int C) { return geglu_mlp_supported(C) ? (long long)geglu_mlp_bias_floats(C) : 0; }
int lavie_pack_geglu_mlp_f16(const void* w1, const void* b1_f16, const void* w2, int C, void* img, float* b1img, void* stream) {
    LAVIE_CHECK(w1 && b1_f16 && w2 && img && b1img, "pack_geglu_mlp: null tensor");
    return pack_geglu_mlp(H(w1), H(b1_f16), H(w2), C, (half_t*)img, b1img, S(stream));
}
int lavie_geglu_mlp_f16(const void* x, void* y, int M, int C, const void* img, const float* b1img, const float* gamma,
                        const float* beta, const float* b2, float eps, void* stream) {
    return launch_geglu_mlp(H(x), (half_t*)y, M, C, H(img), b1img, gamma, beta, b2, eps, S(stream));
}

long long lavie_temporal_block_image_bytes(int C, int heads, int F, int rot_dim) {
    return temporal_block_supported(C, heads, F, rot_dim) ? (long long)temporal_block_image_bytes(C) : 0;
}
int lavie_pack_temporal_block_f16(const void* wq, const void* wk, const void* wv, const void* wo, int C, void* img, void* stream) {
    LAVIE_CHECK(wq && wk && wv && wo && img, "pack_temporal_block: null tensor");
    return pack_temporal_block(H(wq), H(wk), H(wv), H(wo), C, (half_t*)img, S(stream));
}
int lavie_temporal_block_f16(const void* x, void* y, int B, int F, int D, int C, int heads, const void* img, const float* gamma,
                             const float* beta, const float* bo, const float* relbias, const float* rot_cos,
                             const float* rot_sin, int rot_dim, float scale, float eps, void* stream) {
    return launch_temporal_block(H(x), (half_t*)y, B, F, D, C, heads, H(img), gamma, beta, bo, relbias, rot_cos, rot_sin, rot_dim,
                                 scale, eps, S(stream));
}

// the two cross-block families of the C ABI: one set of functions (rowfuse_cross.hip), the variant fixed by the entry point's name
long long lavie_cross_block_image_bytes(int C, int heads) {
    return cross_block_variant(C, heads, 1, 16) == CROSS_SHORT ? (long long)cross_block_image_bytes(CROSS_SHORT) : 0;
}
int lavie_pack_cross_block_f16(const void* wo1, const void* wq2, const void* wo2, int C, void* tmpl, void* stream) {
    LAVIE_CHECK(wo1 && wq2 && wo2 && tmpl, "pack_cross_block: null tensor");
    return pack_cross_block(CROSS_SHORT, H(wo1), H(wq2), H(wo2), C, (half_t*)tmpl, S(stream));
}
int lavie_bind_cross_block_f16(const void* tmpl, const void* kv, int B, int ctx_len, int C, void* img, void* stream) {
    LAVIE_CHECK(tmpl && kv && img, "bind_cross_block: null tensor");
    return bind_cross_block(CROSS_SHORT, H(tmpl), H(kv), B, ctx_len, C, (half_t*)img, S(stream));
}
int lavie_cross_block_f16(const void* att, const void* x, void* y, int M, int rows_per_batch, int C, int heads, const void* img,
                          const float* bo1, const float* gamma, const float* beta, const float* bo2, int ctx_len, float scale,
                          float eps, void* stream) {
    return launch_cross_block(CROSS_SHORT, H(att), H(x), (half_t*)y, M, rows_per_batch, C, heads, H(img), bo1, gamma, beta, bo2, ctx_len,
                              scale, eps, S(stream));
}
long long lavie_cross_block_long_image_bytes(int C, int heads) {
    return cross_block_variant(C, heads, 81, 16) == CROSS_LONG ? (long long)cross_block_image_bytes(CROSS_LONG) : 0;
}
int lavie_pack_cross_block_long_f16(const void* wo1, const void* wq2, const void* wo2, int C, void* tmpl, void* stream) {
    LAVIE_CHECK(wo1 && wq2 && wo2 && tmpl, "pack_cross_block_long: null tensor");
    return pack_cross_block(CROSS_LONG, H(wo1), H(wq2), H(wo2), C, (half_t*)tmpl, S(stream));
}
int lavie_bind_cross_block_long_f16(const void* tmpl, const void* kv, int B, int ctx_len, int C, void* img, void* stream) {
    LAVIE_CHECK(tmpl && kv && img, "bind_cross_block_long: null tensor");
    return bind_cross_block(CROSS_LONG, H(tmpl), H(kv), B, ctx_len, C, (half_t*)img, S(stream));
}
int lavie_cross_block_long_f16(const void* att, const void* x, void* y, int M, int rows_per_batch, int C, int heads, const void* img,
                               const float* bo1, const float* gamma, const float* beta, const float* bo2, int ctx_len, float scale,
                               float eps, void* stream) {
    return launch_cross_block(CROSS_LONG, H(att), H(x), (half_t*)y, M, rows_per_batch, C, heads, H(img), bo1, gamma, beta, bo2, ctx_len,
                              scale, eps, S(stream));
}

int lavie_conv3x3_f16(const void* x1, int C1, const void* x2, int C2, const void* sc1, int SC1, const void* sc2, int SC2,
                      const void* Wp, const float* bias, const float* bias2, int ldb2, int rows_per_batch, const void* R,
                      void* y, int NI, int Hi, int Wi, int Cout, int stride, int ups, const void* zero_page,
                      void* stream) {
    LAVIE_CHECK(x1 && Wp && y && zero_page, "conv3x3: null tensor");
    LAVIE_CHECK((stride == 1 || stride == 2) && (ups == 0 || ups == 1) && !(ups && stride != 1), "conv3x3: stride=%d ups=%d", stride, ups);
    LAVIE_CHECK(C1 > 0 && C1 % IGEMM_BK == 0 && C2 % IGEMM_BK == 0 && SC1 % IGEMM_BK == 0 && SC2 % IGEMM_BK == 0,
                "conv3x3: channel counts must be multiples of %d", IGEMM_BK);
    LAVIE_CHECK((!SC1 && !SC2) || (stride == 1 && !ups), "conv3x3: fused shortcut needs stride 1, no upsample");
    LAVIE_CHECK(!bias2 || rows_per_batch > 0, "conv3x3: bias2 needs rows_per_batch > 0");
    const half_t* src[2] = {H(x1), H(x2)};
    const int srcC[2] = {C1, x2 ? C2 : 0};
    const half_t* sc[2] = {H(sc1), H(sc2)};
    const int scC[2] = {sc1 ? SC1 : 0, sc2 ? SC2 : 0};
    IgemmParams p;
    if (int rc = igemm_setup_conv3x3(&p, src, srcC, 2, sc, scC, 2, H(Wp), 9 * (srcC[0] + srcC[1]) + scC[0] + scC[1], H(y), NI, Hi, Wi,
                                     Cout, stride, ups, H(zero_page)))
        return rc;
    p.bias = bias; p.bias2 = bias2; p.ldb2 = ldb2; p.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; p.R = H(R);
    return op_launch(p, true, EPI_LINEAR, S(stream));
}

int lavie_conv3x3_down_f16(const void* x, int C, const void* Wp, const float* bias, void* y, int NI, int Hi, int Wi, int Cout, int stride,
                           int pad_lo, const void* zero_page, void* stream) {
    LAVIE_CHECK(x && Wp && y && zero_page, "conv3x3_down: null tensor");
    LAVIE_CHECK(stride == 1 || stride == 2, "conv3x3_down: stride=%d (1 or 2)", stride);
    LAVIE_CHECK(pad_lo == 0 || pad_lo == 1, "conv3x3_down: pad_lo=%d (0 or 1)", pad_lo);
    LAVIE_CHECK(pad_lo == 1 || stride == 2, "conv3x3_down: pad_lo=0 needs stride 2 (stride=%d)", stride);
    LAVIE_CHECK(C > 0 && C % IGEMM_BK == 0 && Cout > 0 && Cout % IGEMM_BK == 0, "conv3x3_down: channel counts must be multiples of %d (C=%d Cout=%d)",
                IGEMM_BK, C, Cout);
    LAVIE_CHECK(NI >= 1 && Hi >= 2 - pad_lo && Wi >= 2 - pad_lo && (long long)NI * Hi * Wi * (C > Cout ? C : Cout) < (1ll << 31),
                "conv3x3_down: bad shape NI=%d %dx%d", NI, Hi, Wi);
    const half_t* src[1] = {H(x)};
    const int srcC[1] = {C};
    IgemmParams p;
    if (int rc = igemm_setup_conv3x3(&p, src, srcC, 1, nullptr, nullptr, 0, H(Wp), 9 * C, H(y), NI, Hi, Wi, Cout, stride, 0, H(zero_page), pad_lo))
        return rc;
    p.bias = bias;
    return op_launch(p, true, EPI_LINEAR, S(stream));
}

int lavie_pack_conv_edge_in_f16(const void* w, void* out, int Cout, int Cin, void* stream) {
    LAVIE_CHECK(w && out, "pack_conv_edge_in: null tensor");
    return launch_pack_conv_edge_in(H(w), H(out), Cout, Cin, S(stream));
}
int lavie_conv_edge_in_f16(const void* x, int x_dtype, const void* wp, const float* bias, const float* tap_bias, void* y, int N, int Cin,
                           int H_, int W_, int Cout, void* stream) {
    LAVIE_CHECK(x && wp && y, "conv_edge_in: null tensor");
    LAVIE_CHECK(x_dtype == 0 || x_dtype == 1, "conv_edge_in: x_dtype=%d (0 = fp16, 1 = fp32)", x_dtype);
    return launch_conv_edge_in(x, x_dtype == 1, H(wp), bias, tap_bias, H(y), N, Cin, H_, W_, Cout, S(stream));
}
long long lavie_conv_edge_out_image_halfs(int Cin) { return conv_edge_out_image_halfs(Cin); }
int lavie_pack_conv_edge_out_f16(const void* w, void* out, int Cout, int Cin, void* stream) {
    LAVIE_CHECK(w && out, "pack_conv_edge_out: null tensor");
    return launch_pack_conv_edge_out(H(w), H(out), Cout, Cin, S(stream));
}
int lavie_conv_edge_out_f16(const void* x, const void* wp, const float* bias, void* y, int y_dtype, int N, int Cin, int H_, int W_, int Cout,
                            void* stream) {
    LAVIE_CHECK(x && wp && y, "conv_edge_out: null tensor");
    LAVIE_CHECK(y_dtype == 0 || y_dtype == 1, "conv_edge_out: y_dtype=%d (0 = fp16, 1 = fp32)", y_dtype);
    return launch_conv_edge_out(H(x), H(wp), bias, y, y_dtype == 1, N, Cin, H_, W_, Cout, S(stream));
}

int lavie_pack_conv3x3_parity_f16(const void* w, void* out, int Cout, int Cin, void* stream) {
    LAVIE_CHECK(w && out && Cout > 0 && Cin > 0, "pack_conv3x3_parity: bad arguments");
    return launch_pack_conv3x3_parity(H(w), H(out), Cout, Cin, S(stream));
}
int lavie_upsample_conv3x3_supported(int NI, int Hi, int Wi, int C) {
    IgemmParams p;
    return igemm_setup_parity_upsample(&p, nullptr, C, nullptr, nullptr, nullptr, NI, Hi, Wi, nullptr) ? 1 : 0;
}
int lavie_upsample_conv3x3_f16(const void* x, const void* wpar, const float* bias, void* y, int NI, int Hi, int Wi, int C,
                               const void* zero_page, void* stream) {
    LAVIE_CHECK(x && wpar && y && zero_page, "upsample_conv3x3: null tensor");
    IgemmParams p;
    LAVIE_CHECK(igemm_setup_parity_upsample(&p, H(x), C, H(wpar), bias, H(y), NI, Hi, Wi, H(zero_page)),
                "upsample_conv3x3: NI=%d %dx%d C=%d is outside the parity kernel's geometry (lavie_upsample_conv3x3_supported)", NI, Hi, Wi, C);
    return op_launch(p, true, EPI_LINEAR, S(stream));
}

int lavie_pack_conv3x3_f16(const void* w, void* out, int Cout, int Cin, int ld_out, int col0, void* stream) {
    LAVIE_CHECK(w && out && ld_out >= col0 + 9 * Cin, "pack_conv3x3: bad arguments");
    return launch_pack_conv3x3(H(w), H(out), Cout, Cin, ld_out, col0, true, S(stream));
}

int lavie_temporal_conv_f16(const void* x, int C, const void* Wp, const float* bias, const float* bias2, int ldb2,
                            int rows_per_batch, const void* R, void* y, int B, int F, int D, int Cout, int taps,
                            const void* zero_page, void* stream) {
    LAVIE_CHECK(x && Wp && y && zero_page, "temporal_conv: null tensor");
    LAVIE_CHECK(taps == 3 || taps == 5, "temporal_conv: taps=%d (3 or 5)", taps);
    LAVIE_CHECK(C > 0 && C % IGEMM_BK == 0 && Cout % 64 == 0, "temporal_conv: channel counts must be multiples of %d", IGEMM_BK);
    LAVIE_CHECK(B >= 1 && F >= 1 && D >= 1 && (long long)B * F * D * (C > Cout ? C : Cout) < (1ll << 31), "temporal_conv: bad shape");
    LAVIE_CHECK(!bias2 || rows_per_batch > 0, "temporal_conv: bias2 needs rows_per_batch > 0");
    IgemmParams p;
    if (int rc = igemm_setup_temporal_conv(&p, H(x), C, H(Wp), bias, H(y), B, F, D, Cout, taps, H(zero_page))) return rc;
    p.bias2 = bias2; p.ldb2 = ldb2; p.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; p.R = H(R);
    return op_launch(p, true, EPI_LINEAR, S(stream));
}

int lavie_pack_temporal_conv_f16(const void* w, void* out, int Cout, int Cin, int taps, void* stream) {
    LAVIE_CHECK(w && out && (taps == 3 || taps == 5), "pack_temporal_conv: bad arguments");
    return launch_pack_conv_taps(H(w), H(out), Cout, Cin, taps, taps * Cin, 0, true, S(stream));
}

int lavie_pack_geglu_f16(const void* w, const void* bias_f16, void* w_out, float* bias_out, int N, int K, void* stream) {
    LAVIE_CHECK(w && w_out, "pack_geglu: null tensor");
    int rc = launch_pack_geglu_rows(H(w), H(w_out), N, K, S(stream));
    if (rc == 0 && bias_f16 && bias_out) rc = launch_pack_geglu_bias(H(bias_f16), bias_out, N, S(stream));
    return rc;
}

long long lavie_proj_qkv_image_bytes(int C) { return proj_qkv_supported(C) ? (long long)proj_qkv_image_bytes(C) : 0; }
int lavie_pack_proj_qkv_f16(const void* wpin, const void* wqkv, int C, void* img, void* stream) {
    LAVIE_CHECK(wpin && wqkv && img, "pack_proj_qkv: null tensor");
    return pack_proj_qkv(H(wpin), H(wqkv), C, (half_t*)img, S(stream));
}
int lavie_group_norm_affine_f16(const void* x, int C, int NB, int P, int groups, const float* gamma, const float* beta, float eps,
                                float* stats_ws, float* ab_out, void* stream) {
    LAVIE_CHECK(x && gamma && beta && stats_ws && ab_out, "group_norm_affine: null tensor");
    LAVIE_CHECK(NB > 0 && P > 0 && groups > 0, "group_norm_affine: empty problem");
    return launch_group_norm(H(x), C, nullptr, 0, NB, P, groups, gamma, beta, eps, false, stats_ws, nullptr, S(stream), nullptr, nullptr, ab_out);
}
int lavie_proj_qkv_f16(const void* x, const float* gn_ab, int rows_per_domain, const void* img, const float* bpin, const float* ln_gamma,
                       const float* ln_beta, float ln_eps, void* tx, void* qkv, int M, int C, void* stream) {
    return launch_proj_qkv(H(x), gn_ab, rows_per_domain, H(img), bpin, ln_gamma, ln_beta, ln_eps, (half_t*)tx, (half_t*)qkv, M, C, S(stream));
}

int lavie_group_norm_f16(const void* x1, int C1, const void* x2, int C2, int NB, int P, int groups, const float* gamma,
                         const float* beta, float eps, int silu, float* stats_ws, void* y, void* stream) {
    LAVIE_CHECK(x1 && gamma && beta && stats_ws && y, "group_norm: null tensor");
    LAVIE_CHECK(NB > 0 && P > 0 && groups > 0, "group_norm: empty problem");
    if (!x2) C2 = 0;
    return launch_group_norm(H(x1), C1, H(x2), C2, NB, P, groups, gamma, beta, eps, silu != 0, stats_ws, H(y), S(stream));
}

long long lavie_group_norm_ws_floats(int NB, int groups) { return (long long)gn_workspace_floats(NB, groups); }

int lavie_layer_norm_f16(const void* x, const float* gamma, const float* beta, void* y, int rows, int C, float eps,
                         void* stream) {
    LAVIE_CHECK(x && gamma && beta && y && rows > 0, "layer_norm: bad arguments");
    return launch_layernorm(H(x), gamma, beta, H(y), rows, C, eps, S(stream));
}

int lavie_attention_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int NB,
                        int Lq, int Lk, int heads, int dh, int kv_batch_div, float scale, void* stream) {
    LAVIE_CHECK(q && k && v && o, "attention: null tensor");
    AttnParams a;
    a.q = H(q); a.ldq = ldq; a.k = H(k); a.ldk = ldk; a.v = H(v); a.ldv = ldv; a.o = H(o); a.ldo = ldo;
    a.NBq = NB; a.Lq = Lq; a.Lk = Lk; a.heads = heads; a.dh = dh; a.kv_batch_div = kv_batch_div; a.scale = scale;
    return launch_attention(a, S(stream));
}

int lavie_sparse_causal_attention_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o,
                                      int ldo, int NB, int frames, int D, int heads, int dh, float scale, void* stream) {
    LAVIE_CHECK(q && k && v && o, "sparse-causal attention: null tensor");
    LAVIE_CHECK(frames >= 1 && NB >= frames && NB % frames == 0 && D >= 1, "sparse-causal attention: NB=%d frames=%d D=%d", NB, frames, D);
    AttnParams a;
    a.q = H(q); a.ldq = ldq; a.k = H(k); a.ldk = ldk; a.v = H(v); a.ldv = ldv; a.o = H(o); a.ldo = ldo;
    a.NBq = NB; a.Lq = D; a.Lk = 2 * D; a.heads = heads; a.dh = dh; a.kv_batch_div = 1; a.scale = scale;
    a.sc_frames = frames;
    return launch_attention(a, S(stream));
}

int lavie_temporal_attention_f16(const void* qkv, int ld, void* o, int ldo, int B, int F, int D, int heads, int dh,
                                 const float* bias, const float* rot_cos, const float* rot_sin, int rot_dim, float scale,
                                 void* stream) {
    LAVIE_CHECK(qkv && o && bias && (rot_dim == 0 || (rot_cos && rot_sin)), "temporal attention: null tensor");
    TemporalParams t;
    t.qkv = H(qkv); t.ld = ld; t.o = H(o); t.ldo = ldo; t.B = B; t.F = F; t.D = D; t.heads = heads; t.dh = dh;
    t.bias = bias; t.rot_cos = rot_cos; t.rot_sin = rot_sin; t.rot_dim = rot_dim; t.scale = scale;
    return launch_temporal_attention(t, S(stream));
}

int lavie_relpos_buckets(int F, int num_buckets, int max_distance, int* out_host) {
    LAVIE_CHECK(F > 0 && num_buckets >= 4 && max_distance > num_buckets / 4 && out_host, "relpos_buckets: bad arguments");
    relpos_bucket_table(F, num_buckets, max_distance, out_host);
    return 0;
}

// ---- the forward's end and glue kernels at operator level: thin wrappers over the launchers of ops.h, so that each kernel can be
// run on its own operands (tests/opcases.py).  What the engine guarantees by construction is checked here; the launchers' own
// refusals pass through.
int lavie_timestep_sinusoid_f32(const float* t, float* out, int B, int dim, void* stream) {
    LAVIE_CHECK(t && out, "timestep_sinusoid: null tensor");
    LAVIE_CHECK(B >= 1 && dim >= 2 && dim % 2 == 0 && (long long)B * dim < (1ll << 31), "timestep_sinusoid: B=%d dim=%d (dim even, >= 2)", B, dim);
    return launch_timestep_sinusoid(t, out, B, dim, S(stream));
}
int lavie_gemv_f16(const float* in, const void* W, const float* bias, float* out, int B, int N, int K, int act_in, int act_out,
                   void* stream) {
    LAVIE_CHECK(in && W && out, "gemv: null tensor");
    LAVIE_CHECK(N >= 1 && K >= 1, "gemv: N=%d K=%d", N, K);
    LAVIE_CHECK((act_in == 0 || act_in == 1) && (act_out == 0 || act_out == 1), "gemv: act_in=%d act_out=%d (0 or 1)", act_in, act_out);
    return launch_gemv(in, H(W), bias, out, B, N, K, act_in, act_out, S(stream));
}
int lavie_pack_conv_in_f16(const void* w, void* out, int Cout, int Cin, void* stream) {
    LAVIE_CHECK(w && out, "pack_conv_in: null tensor");
    LAVIE_CHECK(Cout >= 8 && Cout % 8 == 0 && Cin >= 2 && Cin % 2 == 0 && (long long)Cout * Cin * 9 < (1ll << 31),
                "pack_conv_in: Cout must be a multiple of 8 and Cin even (Cout=%d Cin=%d)", Cout, Cin);
    return launch_pack_conv_in(H(w), H(out), Cout, Cin, S(stream));
}
int lavie_conv_in_f16(const void* x_ncfhw, const void* wp, const float* bias, void* y, int B, int Cin, int F, int H_, int W_, int Cout,
                      void* stream) {
    LAVIE_CHECK(x_ncfhw && wp && bias && y, "conv_in: null tensor");
    LAVIE_CHECK(B >= 1 && F >= 1 && H_ >= 1 && W_ >= 1 && Cin >= 1 && Cout >= 1, "conv_in: bad shape B=%d Cin=%d F=%d %dx%d Cout=%d", B, Cin, F, H_,
                W_, Cout);
    return launch_conv_in(H(x_ncfhw), H(wp), bias, H(y), B, Cin, F, H_, W_, Cout, S(stream));
}
int lavie_pack_conv_out_f16(const void* w, void* out, int Cout, int Cin, void* stream) {
    LAVIE_CHECK(w && out, "pack_conv_out: null tensor");
    LAVIE_CHECK(Cout >= 1 && Cin >= 1 && (long long)Cout * Cin * 9 < (1ll << 31), "pack_conv_out: Cout=%d Cin=%d", Cout, Cin);
    return launch_pack_conv3x3(H(w), H(out), Cout, Cin, 9 * Cin, 0, false, S(stream));
}
int lavie_conv_out_f16(const void* x, const void* wp, const float* bias, void* y_ncfhw, int B, int Cin, int F, int H_, int W_, int Cout,
                       void* stream) {
    LAVIE_CHECK(x && wp && bias && y_ncfhw, "conv_out: null tensor");
    LAVIE_CHECK(B >= 1 && F >= 1 && H_ >= 1 && W_ >= 1 && Cin >= 1 && Cout >= 1, "conv_out: bad shape B=%d Cin=%d F=%d %dx%d Cout=%d", B, Cin, F, H_,
                W_, Cout);
    return launch_conv_out(H(x), H(wp), bias, H(y_ncfhw), B, Cin, F, H_, W_, Cout, S(stream));
}
int lavie_add_class_emb_silu_f32(float* emb_inout, const void* table, const int* labels_host, int B, int N, int num_classes, void* stream) {
    LAVIE_CHECK(emb_inout && table && labels_host, "add_class_emb_silu: null argument");
    LAVIE_CHECK(B >= 1 && B <= 8 && N >= 1 && num_classes >= 1, "add_class_emb_silu: B=%d (1..8) N=%d num_classes=%d", B, N, num_classes);
    for (int b = 0; b < B; ++b)      // the launcher takes the labels as they come (the engine checks them, engine.cpp forward)
        LAVIE_CHECK(labels_host[b] >= 0 && labels_host[b] < num_classes, "add_class_emb_silu: class label %d out of range (0..%d)", labels_host[b],
                    num_classes - 1);
    return launch_add_class_emb_silu(emb_inout, H(table), labels_host, B, N, S(stream));
}
int lavie_fill_relpos_bias_f32(const void* emb, const int* buckets_dev, float* out, int heads, int F, int num_buckets, void* stream) {
    LAVIE_CHECK(emb && buckets_dev && out, "fill_relpos_bias: null tensor");
    LAVIE_CHECK(heads >= 1 && F >= 1 && num_buckets >= 1 && (long long)heads * F * F < (1ll << 31), "fill_relpos_bias: heads=%d F=%d num_buckets=%d",
                heads, F, num_buckets);
    return launch_fill_relpos_bias(H(emb), buckets_dev, out, heads, F, S(stream));
}
int lavie_ln_fold_f16(const void* W, const float* gamma, const float* beta, const void* bias_f16, void* Wout, float* s_out, float* b_out, int N,
                      int K, void* stream) {
    LAVIE_CHECK(W && gamma && beta && Wout && s_out && b_out, "ln_fold: null tensor");
    LAVIE_CHECK(N >= 1 && K >= 1, "ln_fold: N=%d K=%d", N, K);
    return launch_ln_fold(H(W), gamma, beta, H(bias_f16), H(Wout), s_out, b_out, N, K, S(stream));
}
int lavie_pack_geglu_vec_f32(const float* in, float* out, int N, void* stream) {
    LAVIE_CHECK(in && out, "pack_geglu_vec: null tensor");
    LAVIE_CHECK(N >= 32 && N % 32 == 0, "pack_geglu_vec: N=%d must be a multiple of 32", N);      // (the launcher does not check the vector form)
    return launch_pack_geglu_vec(in, out, N, S(stream));
}
int lavie_copy_rows_f16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, int col0, void* stream) {
    LAVIE_CHECK(src && dst, "copy_rows: null tensor");
    LAVIE_CHECK(rows >= 1 && cols >= 1 && col0 >= 0, "copy_rows: rows=%d cols=%d col0=%d", rows, cols, col0);
    LAVIE_CHECK(ld_src >= cols && (long long)ld_dst >= (long long)col0 + cols, "copy_rows: ld_src=%d < cols=%d or ld_dst=%d < col0 + cols=%d", ld_src, cols,
                ld_dst, col0 + cols);
    return launch_copy_rows(H(src), ld_src, H(dst), ld_dst, rows, cols, col0, S(stream));
}
int lavie_f16_to_f32(const void* a, const void* b, float* dst, long long n, void* stream) {
    LAVIE_CHECK(a && dst && n >= 1, "f16_to_f32: bad arguments");
    return b ? launch_add_f16_to_f32(H(a), H(b), dst, n, S(stream)) : launch_f16_to_f32(H(a), dst, n, S(stream));
}

// ---- The fused scheduler steps.  Every entry fills a StepArgs (ops.h), runs the one checker below and calls launch_step; what is
// checked follows from the arguments, not from the entry: all on the host, before any HIP call.
static int check_aligned(const char* who, const char* name, const void* p) {
    LAVIE_CHECK(((uintptr_t)p & 15) == 0, "%s: %s at %p is not 16-byte aligned", who, name, p);
    return 0;
}

// guidance, the five coefficients and the next step's input scale; c4_name: what the caller calls the fifth coefficient
static int check_coefficients(const char* who, const StepCoef& c, float in_scale, const char* c4_name) {
    const float s[7] = {c.guidance, c.kx, c.ke, c.c0, c.ct, c.c4, in_scale};
    const char* const names[7] = {"guidance", "k_x", "k_eps", "c_x0", "c_xt", c4_name, "next_input_scale"};
    for (int i = 0; i < 7; ++i) LAVIE_CHECK(__builtin_isfinite(s[i]), "%s: %s (%g) is not finite", who, names[i], (double)s[i]);
    return 0;
}

// region -> the launcher's operands in `k` and `a`; a null region or one of another layout is refused before a field is read
static int fill_region(const char* who, const lavie_known_region* r, KnownOperands* k, StepArgs* a) {
    LAVIE_CHECK(r, "%s: region is null", who);
    LAVIE_CHECK(r->struct_size == (int)sizeof(lavie_known_region),
                "%s: region->struct_size=%d but this library's lavie_known_region has %d bytes: the binding's struct layout is "
                "out of date", who, r->struct_size, (int)sizeof(lavie_known_region));
    *k = KnownOperands{r->known, r->mask, r->noise_known, r->a_next, r->s_next};
    a->known = k; a->channels = r->channels; a->inner = r->inner;
    return 0;
}

// the region's own operands (sampler_known.hip), for the steps and for the start blend (the one caller whose mask is optional)
static int check_region(const char* who, const StepArgs& a, bool mask_optional) {
    const KnownOperands& k = *a.known;
    LAVIE_CHECK(k.known, "%s: region->known is null", who);
    LAVIE_CHECK(k.mask || mask_optional, "%s: region->mask is null", who);
    LAVIE_CHECK(__builtin_isfinite(k.a) && __builtin_isfinite(k.s), "%s: region->a_next=%g / s_next=%g is not finite", who, (double)k.a,
                (double)k.s);
    LAVIE_CHECK(k.s == 0.f || k.noise, "%s: region->noise_known is null but s_next=%g", who, (double)k.s);
    LAVIE_CHECK(a.channels >= 1 && a.inner >= 1, "%s: region->channels=%d inner=%lld must be >= 1", who, a.channels, (long long)a.inner);
    const long long plane = a.inner <= (1ll << 40) ? (long long)a.channels * a.inner : 0;
    LAVIE_CHECK(a.n >= 1 && plane > 0 && a.n % plane == 0, "%s: n=%lld is not a whole number of videos of channels=%d x inner=%lld", who,
                (long long)a.n, a.channels, (long long)a.inner);
    if (a.inner % 8 == 0) {                 // the eight-elements-per-lane form
        if (int rc = check_aligned(who, "region->known", k.known)) return rc;
        if (int rc = check_aligned(who, "region->mask", k.mask)) return rc;
        if (int rc = check_aligned(who, "region->noise_known", k.s != 0.f ? k.noise : nullptr)) return rc;
    }
    return 0;
}

// scalars = false: the three plain five-coefficient entries take their scalars as they come, as they always have
static int check_step(const char* who, const StepArgs& a, bool scalars = true) {
    const bool aux_used = a.multistep || (a.c.c4 != 0.f && !a.key);     // the history is always written; the noise is read when sigma != 0 (and no key makes it)
    const void* const t[4] = {a.eps, a.x, a.model_in, aux_used ? a.aux : nullptr};
    const char* const names[4] = {"eps", "x", "model_in", a.multistep ? "x0_prev" : "noise"};
    for (int i = 0; i < 3; ++i) LAVIE_CHECK(t[i], "%s: null argument: %s is null", who, names[i]);
    if (a.multistep) LAVIE_CHECK(a.aux, "%s: null argument: x0_prev is null", who);
    else LAVIE_CHECK(!aux_used || a.aux, "%s: noise is null but sigma=%g", who, (double)a.c.c4);
    LAVIE_CHECK(a.n >= 1, "%s: n=%lld must be >= 1", who, (long long)a.n);
    if (scalars)
        if (int rc = check_coefficients(who, a.c, a.in_scale, a.multistep ? "c_prev" : "sigma")) return rc;
    if (a.known)
        if (int rc = check_region(who, a, false)) return rc;
    if (a.table && !a.known) {              // grid.y = the latents of `per` elements; around known latents it is the region's planes
        LAVIE_CHECK(a.per >= 2 && a.per <= (1ll << 40), "%s: per=%lld must be >= 2", who, (long long)a.per);
        LAVIE_CHECK(a.n % a.per == 0, "%s: n=%lld is not a whole number of latents of per=%lld", who, (long long)a.n, (long long)a.per);
        LAVIE_CHECK(a.n / a.per <= 65535, "%s: n / per = %lld latents, at most 65535 fit one launch", who, (long long)(a.n / a.per));
    }
    if (a.eps_pag) {                        // perturbed-attention guidance (sampler_pag.hip): the third operand's scale
        LAVIE_CHECK(!a.known && !a.table, "%s: pag_scale is not combined with a known region or a guidance table", who);
        LAVIE_CHECK(__builtin_isfinite(a.pag_scale), "%s: pag_scale (%g) is not finite", who, (double)a.pag_scale);
        LAVIE_CHECK(a.pag_scale >= 0.f, "%s: pag_scale=%g must be >= 0", who, (double)a.pag_scale);
    }
    // 16-byte accesses: the eight-element form of the kernel that will run.  The plain five-coefficient kernel has none; the plain
    // seeded one (StepArgs::key) neither: it takes eight elements per lane only where its tensors are aligned.  The plain
    // multistep kernel counts as one whatever n is (its vector body is empty under guidance with n % 8 != 0, the rule was never relaxed)
    const bool vec8 = a.known ? a.inner % 8 == 0 : a.table ? a.per % 8 == 0 : a.eps_pag ? a.n % 8 == 0 : a.multistep;
    if (vec8) {
        for (int i = 0; i < 4; ++i)
            if (int rc = check_aligned(who, names[i], t[i])) return rc;
        if (int rc = check_aligned(who, "eps (its perturbed part)", a.eps_pag)) return rc;
    }
    return 0;
}

static StepArgs step_args(bool multistep, bool cfg, const void* eps, float* x, const float* aux, void* model_in, long long n, float guidance,
                          float k_x, float k_eps, float c_x0, float c_xt, float c4, float in_scale, const float* table = nullptr,
                          long long per = 0) {
    StepArgs a{};
    a.multistep = multistep; a.cfg = cfg;
    a.eps = H(eps); a.x = x; a.aux = const_cast<float*>(aux); a.model_in = H(model_in); a.n = n;     // the noise is only read
    a.c = StepCoef{guidance, k_x, k_eps, c_x0, c_xt, c4}; a.in_scale = in_scale;
    a.table = table; a.per = per;
    return a;
}

static int run_step(const char* who, const StepArgs& a, void* stream, bool scalars = true) {
    if (int rc = check_step(who, a, scalars)) return rc;
    return launch_step(a, S(stream));
}

// perturbed-attention guidance: eps / model_in hold one part more than the plain namesake's, the perturbed prediction last
static int run_step_pag(const char* who, StepArgs a, float pag_scale, void* stream) {
    if (a.eps && a.n >= 1 && a.n <= (1ll << 40)) a.eps_pag = a.eps + (a.cfg ? 2 : 1) * a.n;      // (else check_step refuses the call)
    a.pag_scale = pag_scale;
    return run_step(who, a, stream);
}

static int run_step_known(const char* who, StepArgs a, const lavie_known_region* region, void* stream) {
    KnownOperands k;
    if (int rc = fill_region(who, region, &k, &a)) return rc;
    return run_step(who, a, stream);
}

int lavie_cfg_ddpm_step(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float guidance,
                        float k_x, float k_eps, float c_x0, float c_xt, float sigma, void* stream) {
    return run_step("cfg_ddpm_step", step_args(false, true, eps2, x, noise, model_in2, n, guidance, k_x, k_eps, c_x0, c_xt, sigma, 1.0f),
                    stream, false);
}

int lavie_cfg_sampler_step(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float guidance,
                           float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, void* stream) {
    return run_step("cfg_sampler_step", step_args(false, true, eps2, x, noise, model_in2, n, guidance, k_x, k_eps, c_x0, c_xt, sigma,
                                                  next_input_scale), stream, false);
}

int lavie_sampler_step(const void* eps, float* x, const float* noise, void* model_in, long long n, float k_x, float k_eps,
                       float c_x0, float c_xt, float sigma, float next_input_scale, void* stream) {
    return run_step("sampler_step", step_args(false, false, eps, x, noise, model_in, n, 1.0f, k_x, k_eps, c_x0, c_xt, sigma,
                                              next_input_scale), stream, false);
}

int lavie_cfg_multistep_step(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, float guidance, float k_x,
                             float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale, void* stream) {
    return run_step("cfg_multistep_step", step_args(true, true, eps2, x, x0_prev, model_in2, n, guidance, k_x, k_eps, c_x0, c_xt, c_prev,
                                                    next_input_scale), stream);
}

int lavie_multistep_step(const void* eps, float* x, float* x0_prev, void* model_in, long long n, float k_x, float k_eps,
                         float c_x0, float c_xt, float c_prev, float next_input_scale, void* stream) {
    return run_step("multistep_step", step_args(true, false, eps, x, x0_prev, model_in, n, 1.0f, k_x, k_eps, c_x0, c_xt, c_prev,
                                                next_input_scale), stream);
}

int lavie_cfg_pag_sampler_step(const void* eps3, float* x, const float* noise, void* model_in3, long long n, float guidance, float k_x,
                               float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, float pag_scale, void* stream) {
    return run_step_pag("cfg_pag_sampler_step", step_args(false, true, eps3, x, noise, model_in3, n, guidance, k_x, k_eps, c_x0, c_xt, sigma,
                                                          next_input_scale), pag_scale, stream);
}

int lavie_pag_sampler_step(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float k_x, float k_eps, float c_x0,
                           float c_xt, float sigma, float next_input_scale, float pag_scale, void* stream) {
    return run_step_pag("pag_sampler_step", step_args(false, false, eps2, x, noise, model_in2, n, 1.0f, k_x, k_eps, c_x0, c_xt, sigma,
                                                      next_input_scale), pag_scale, stream);
}

int lavie_cfg_pag_multistep_step(const void* eps3, float* x, float* x0_prev, void* model_in3, long long n, float guidance, float k_x,
                                 float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale, float pag_scale,
                                 void* stream) {
    return run_step_pag("cfg_pag_multistep_step", step_args(true, true, eps3, x, x0_prev, model_in3, n, guidance, k_x, k_eps, c_x0, c_xt,
                                                            c_prev, next_input_scale), pag_scale, stream);
}

int lavie_pag_multistep_step(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, float k_x, float k_eps, float c_x0,
                             float c_xt, float c_prev, float next_input_scale, float pag_scale, void* stream) {
    return run_step_pag("pag_multistep_step", step_args(true, false, eps2, x, x0_prev, model_in2, n, 1.0f, k_x, k_eps, c_x0, c_xt, c_prev,
                                                        next_input_scale), pag_scale, stream);
}

int lavie_cfg_sampler_step_known(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float guidance,
                                 float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, void* stream,
                                 const lavie_known_region* region) {
    return run_step_known("cfg_sampler_step_known", step_args(false, true, eps2, x, noise, model_in2, n, guidance, k_x, k_eps, c_x0, c_xt,
                                                              sigma, next_input_scale), region, stream);
}

int lavie_sampler_step_known(const void* eps, float* x, const float* noise, void* model_in, long long n, float k_x, float k_eps,
                             float c_x0, float c_xt, float sigma, float next_input_scale, void* stream,
                             const lavie_known_region* region) {
    return run_step_known("sampler_step_known", step_args(false, false, eps, x, noise, model_in, n, 1.0f, k_x, k_eps, c_x0, c_xt, sigma,
                                                          next_input_scale), region, stream);
}

int lavie_cfg_multistep_step_known(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, float guidance,
                                   float k_x, float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale,
                                   void* stream, const lavie_known_region* region) {
    return run_step_known("cfg_multistep_step_known", step_args(true, true, eps2, x, x0_prev, model_in2, n, guidance, k_x, k_eps, c_x0,
                                                                c_xt, c_prev, next_input_scale), region, stream);
}

int lavie_multistep_step_known(const void* eps, float* x, float* x0_prev, void* model_in, long long n, float k_x, float k_eps,
                               float c_x0, float c_xt, float c_prev, float next_input_scale, void* stream,
                               const lavie_known_region* region) {
    return run_step_known("multistep_step_known", step_args(true, false, eps, x, x0_prev, model_in, n, 1.0f, k_x, k_eps, c_x0, c_xt,
                                                            c_prev, next_input_scale), region, stream);
}

int lavie_known_blend_f32(float* x, void* model_in, int dup, long long n, float input_scale, void* stream,
                          const lavie_known_region* region) {
    const char* who = "known_blend";
    StepArgs a{};
    KnownOperands k;
    a.x = x; a.model_in = H(model_in); a.n = n;
    if (int rc = fill_region(who, region, &k, &a)) return rc;
    LAVIE_CHECK(x, "%s: x is null", who);
    LAVIE_CHECK(model_in, "%s: model_in is null", who);
    LAVIE_CHECK(__builtin_isfinite(input_scale), "%s: input_scale (%g) is not finite", who, (double)input_scale);
    if (int rc = check_region(who, a, true)) return rc;
    if (a.inner % 8 == 0) {
        if (int rc = check_aligned(who, "x", x)) return rc;
        if (int rc = check_aligned(who, "model_in", model_in)) return rc;
    }
    return launch_known_blend(x, a.model_in, dup != 0, n, input_scale, k.known, k.mask, k.noise, a.channels, a.inner, k.a, k.s, S(stream));
}

// The fused step over overlapping frame windows (sampler_window.hip).  Everything is checked here, on the host, before a table entry
// is dereferenced or anything is launched; each refusal names its argument.
static int window_step(const char* who, const lavie_window_step_args* a, const float* table, void* stream, const NoiseKey* key = nullptr) {
    LAVIE_CHECK(a, "%s: args is null", who);
    LAVIE_CHECK(a->struct_size == (int)sizeof(lavie_window_step_args),
                "%s: args->struct_size=%d but this library's lavie_window_step_args has %d bytes: the binding's struct layout is "
                "out of date", who, a->struct_size, (int)sizeof(lavie_window_step_args));
    LAVIE_CHECK(a->family == 0 || a->family == 1, "%s: family=%d must be 0 (five-coefficient) or 1 (multistep)", who, a->family);
    LAVIE_CHECK(a->P >= 1 && a->C >= 1 && a->F >= 1 && a->hw >= 1, "%s: P=%d C=%d F=%d hw=%lld must be >= 1", who, a->P, a->C, a->F, a->hw);
    LAVIE_CHECK((long long)a->P * a->C * a->F <= 65535, "%s: P C F = %lld planes, at most 65535 fit one launch", who,
                (long long)a->P * a->C * a->F);
    LAVIE_CHECK(a->hw <= (1ll << 40), "%s: hw=%lld is out of range", who, a->hw);
    LAVIE_CHECK(a->W >= 1 && a->W <= LAVIE_WINDOW_MAX_WINDOWS, "%s: W=%d outside 1..%d", who, a->W, LAVIE_WINDOW_MAX_WINDOWS);
    LAVIE_CHECK(a->L >= 1 && a->L <= LAVIE_WINDOW_MAX_LENGTH, "%s: L=%d outside 1..%d", who, a->L, LAVIE_WINDOW_MAX_LENGTH);
    LAVIE_CHECK(a->starts_host, "%s: starts_host is null", who);
    LAVIE_CHECK(a->profile_host, "%s: profile_host is null", who);
    LAVIE_CHECK(a->eps_host, "%s: eps_host is null", who);
    LAVIE_CHECK(a->model_in_host, "%s: model_in_host is null", who);
    const int* st = a->starts_host;
    LAVIE_CHECK(st[0] >= 0, "%s: starts[0]=%d is negative", who, st[0]);
    for (int w = 1; w < a->W; ++w)
        LAVIE_CHECK(st[w] > st[w - 1], "%s: starts[%d]=%d is not above starts[%d]=%d: starts must be strictly ascending", who, w, st[w],
                    w - 1, st[w - 1]);
    LAVIE_CHECK((long long)st[a->W - 1] + a->L <= a->F, "%s: starts[%d]=%d + L=%d runs past F=%d", who, a->W - 1, st[a->W - 1], a->L, a->F);
    for (int f = 0, lo = 0; f < a->F; ++f) {            // lo: the first window that may still cover f
        while (lo < a->W && st[lo] + a->L <= f) ++lo;
        int cover = 0;
        for (int w = lo; w < a->W && st[w] <= f; ++w) ++cover;
        LAVIE_CHECK(cover >= 1, "%s: frame %d is uncovered by the windows (starts, L=%d)", who, f, a->L);
        LAVIE_CHECK(cover <= LAVIE_WINDOW_MAX_COVER, "%s: frame %d has a cover count of %d windows, at most %d (starts, L=%d)", who, f, cover,
                    LAVIE_WINDOW_MAX_COVER, a->L);
    }
    for (int i = 0; i < a->L; ++i)
        LAVIE_CHECK(__builtin_isfinite(a->profile_host[i]) && a->profile_host[i] > 0.f, "%s: profile[%d]=%g must be finite and > 0", who, i,
                    (double)a->profile_host[i]);
    for (int w = 0; w < a->W; ++w) {
        LAVIE_CHECK(a->eps_host[w], "%s: eps[%d] is null", who, w);
        LAVIE_CHECK(a->model_in_host[w], "%s: model_in[%d] is null", who, w);
    }
    LAVIE_CHECK(a->x, "%s: x is null", who);
    const StepCoef c{a->guidance, a->k_x, a->k_eps, a->c_x0, a->c_xt, a->c4};
    if (int rc = check_coefficients(who, c, a->next_input_scale, "c4")) return rc;
    LAVIE_CHECK(!key || a->family == 0, "%s: family=%d: the multistep family draws no noise and takes no noise key", who, a->family);
    LAVIE_CHECK(!key || (key->count == a->P && key->per == (long long)a->C * a->F * a->hw), "%s: key->count=%d per=%lld, the clip has P=%d "
                "latents of C F hw=%lld elements", who, key ? key->count : 0, key ? key->per : 0ll, a->P, (long long)a->C * a->F * a->hw);
    const bool aux_used = a->family == 1 || (a->c4 != 0.f && !key);
    LAVIE_CHECK(!aux_used || a->aux, "%s: aux is null (%s)", who, a->family == 1 ? "the multistep family's x0_prev" : "the step's noise, c4 != 0");
    // byte ranges: x, aux, then eps[w], then model_in[w]; a written range (x, aux, model_in) may overlap nothing, eps may overlap eps
    const unsigned long long clip = (unsigned long long)a->P * a->C * a->F * a->hw * 4;
    const unsigned long long win = (unsigned long long)(a->cfg ? 2 : 1) * a->P * a->C * a->L * a->hw * 2;
    const int nr = 2 + 2 * a->W;
    auto base = [&](int i) { return (uintptr_t)(i == 0 ? (const void*)a->x : i == 1 ? (const void*)a->aux : i < 2 + a->W ? a->eps_host[i - 2] : a->model_in_host[i - 2 - a->W]); };
    auto bytes = [&](int i) { return i < 2 ? clip : win; };
    auto label = [&](int i, char* buf, size_t n) {
        if (i == 0) snprintf(buf, n, "x");
        else if (i == 1) snprintf(buf, n, "aux");
        else if (i < 2 + a->W) snprintf(buf, n, "eps[%d]", i - 2);
        else snprintf(buf, n, "model_in[%d]", i - 2 - a->W);
    };
    for (int i = 0; i < nr; ++i) {
        if (i == 1 && !aux_used) continue;
        for (int j = i + 1; j < nr; ++j) {
            if (j == 1 && !aux_used) continue;
            const bool both_read_only = i >= 2 && i < 2 + a->W && j >= 2 && j < 2 + a->W;
            if (both_read_only) continue;
            const bool overlap = base(i) < base(j) + bytes(j) && base(j) < base(i) + bytes(i);
            char bi[32], bj[32];
            label(i, bi, sizeof bi);
            label(j, bj, sizeof bj);
            LAVIE_CHECK(!overlap, "%s: %s and %s overlap (aliasing)", who, bi, bj);
        }
    }
    if (a->hw % 8 == 0)
        for (int i = 0; i < nr; ++i) {
            if (i == 1 && !aux_used) continue;
            char bi[32];
            label(i, bi, sizeof bi);
            if (int rc = check_aligned(who, bi, (void*)base(i))) return rc;
        }
    WindowStepParams p{};
    p.multistep = a->family == 1;
    p.cfg = a->cfg != 0;
    p.P = a->P; p.C = a->C; p.F = a->F; p.hw = a->hw; p.W = a->W; p.L = a->L;
    p.starts = a->starts_host;
    p.profile = a->profile_host;
    p.eps = reinterpret_cast<const half_t* const*>(a->eps_host);
    p.model_in = reinterpret_cast<half_t* const*>(a->model_in_host);
    p.x = a->x;
    p.aux = a->aux;
    p.c = c;
    p.in_scale = a->next_input_scale;
    p.table = table;
    p.key = key;
    return launch_window_step(p, S(stream));
}

int lavie_window_step(const lavie_window_step_args* a, void* stream) { return window_step("window_step", a, nullptr, stream); }

// ---- Seeded engine noise (philox.h, sampler_noise.hip).
int lavie_philox4x32_host(const unsigned int* key, const unsigned int* counter, unsigned int* out) {
    LAVIE_CHECK(key && counter && out, "philox4x32_host: null argument");
    uint32_t w[4];
    philox4x32_10(key[0], key[1], counter[0], counter[1], counter[2], counter[3], w);
    for (int i = 0; i < 4; ++i) out[i] = w[i];
    return 0;
}

// the caller's key -> the kernel argument; a null key or one of another layout is refused before a field is read
static int fill_key(const char* who, const lavie_noise_key* k, NoiseKey* key) {
    LAVIE_CHECK(k, "%s: key is null", who);
    LAVIE_CHECK(k->struct_size == (int)sizeof(lavie_noise_key),
                "%s: key->struct_size=%d but this library's lavie_noise_key has %d bytes: the binding's struct layout is out of date", who,
                k->struct_size, (int)sizeof(lavie_noise_key));
    LAVIE_CHECK(k->count >= 1 && k->count <= LAVIE_NOISE_MAX_SEEDS, "%s: key->count=%d outside 1..%d", who, k->count, LAVIE_NOISE_MAX_SEEDS);
    LAVIE_CHECK(k->seeds_host, "%s: key->seeds_host is null", who);
    LAVIE_CHECK(k->per >= 1 && k->per <= (1ll << 40), "%s: key->per=%lld must be in 1..2^40", who, k->per);
    *key = NoiseKey{};
    for (int p = 0; p < k->count; ++p) key->seed[p] = k->seeds_host[p];
    key->draw = k->draw; key->per = k->per; key->count = k->count;
    return 0;
}

int lavie_philox_normal_f32(float* out, const unsigned long long* seeds_host, int P, long long per, long long first_element,
                            unsigned long long draw, void* stream) {
    const char* who = "philox_normal";
    LAVIE_CHECK(out, "%s: out is null", who);
    LAVIE_CHECK(seeds_host, "%s: seeds_host is null", who);
    LAVIE_CHECK(P >= 1 && P <= LAVIE_NOISE_MAX_SEEDS, "%s: P=%d outside 1..%d", who, P, LAVIE_NOISE_MAX_SEEDS);
    LAVIE_CHECK(per >= 1 && per <= (1ll << 40), "%s: per=%lld must be in 1..2^40", who, per);
    LAVIE_CHECK(first_element >= 0 && first_element <= (1ll << 62) - per, "%s: first_element=%lld must be >= 0 and first_element + per <= 2^62",
                who, first_element);
    LAVIE_CHECK(((uintptr_t)out & 3) == 0, "%s: out at %p is not 4-byte aligned", who, (const void*)out);
    NoiseKey key{};
    for (int p = 0; p < P; ++p) key.seed[p] = seeds_host[p];
    key.draw = draw; key.per = per; key.count = P;
    return launch_philox_normal(out, key, first_element, S(stream));
}

static int run_step_seeded(const char* who, StepArgs a, const lavie_noise_key* k, void* stream) {
    NoiseKey key;
    if (int rc = fill_key(who, k, &key)) return rc;
    LAVIE_CHECK(a.n == key.count * key.per, "%s: n=%lld is not key->count=%d latents of key->per=%lld elements", who, (long long)a.n, key.count,
                key.per);
    a.key = &key;
    return run_step(who, a, stream, false);        // the scalars as they come, as the plain entries these mirror take them
}

int lavie_sampler_step_seeded(const void* eps, float* x, void* model_in, long long n, float k_x, float k_eps, float c_x0, float c_xt,
                              float sigma, float next_input_scale, void* stream, const lavie_noise_key* key) {
    return run_step_seeded("sampler_step_seeded", step_args(false, false, eps, x, nullptr, model_in, n, 1.0f, k_x, k_eps, c_x0, c_xt, sigma,
                                                            next_input_scale), key, stream);
}

int lavie_cfg_sampler_step_seeded(const void* eps2, float* x, void* model_in2, long long n, float guidance, float k_x, float k_eps,
                                  float c_x0, float c_xt, float sigma, float next_input_scale, void* stream, const lavie_noise_key* key) {
    return run_step_seeded("cfg_sampler_step_seeded", step_args(false, true, eps2, x, nullptr, model_in2, n, guidance, k_x, k_eps, c_x0, c_xt,
                                                                sigma, next_input_scale), key, stream);
}

int lavie_window_step_seeded(const lavie_window_step_args* a, const lavie_noise_key* k, void* stream) {
    NoiseKey key;
    if (int rc = fill_key("window_step_seeded", k, &key)) return rc;
    return window_step("window_step_seeded", a, nullptr, stream, &key);
}

// Test hook: the launchers' own refusals of a noise key beside an operand that has no seeded form.  No C entry can form these
// combinations (the seeded entries take no region, table or perturbed part), so the hook builds the launcher's record itself and
// hands back what the launcher answers.  The key holds no latent (count 0): whatever the launcher decides, nothing is launched.
int lavie_debug_noise_key_refusal(int combine) {
    static float f32[8];
    static half_t f16[8];
    NoiseKey key{};
    key.per = 8;
    if (combine >= 1 && combine <= 4) {
        StepArgs a{};
        KnownOperands k{f32, f32, f32, 1.f, 0.f};
        a.cfg = true; a.eps = f16; a.x = f32; a.model_in = f16; a.n = 8; a.c = StepCoef{7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.f}; a.in_scale = 1.f;
        a.key = &key;
        if (combine == 1) { a.known = &k; a.channels = 1; a.inner = 8; }
        if (combine == 2) { a.table = f32; a.per = 8; }
        if (combine == 3) a.eps_pag = f16;
        if (combine == 4) { a.multistep = true; a.aux = f32; }
        return launch_step(a, nullptr);
    }
    if (combine == 5 || combine == 6) {
        static const int starts[1] = {0};
        static const float profile[1] = {1.f};
        const half_t* eps[1] = {f16};
        half_t* model_in[1] = {f16};
        WindowStepParams p{};
        p.cfg = true; p.P = 1; p.C = 1; p.F = 1; p.hw = 8; p.W = 1; p.L = 1;
        p.starts = starts; p.profile = profile; p.eps = eps; p.model_in = model_in; p.x = f32; p.aux = f32;
        p.c = StepCoef{7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.f}; p.in_scale = 1.f;
        p.key = &key;
        if (combine == 5) p.table = f32;
        if (combine == 6) p.multistep = true;
        return launch_window_step(p, nullptr);
    }
    LAVIE_CHECK(false, "debug_noise_key_refusal: combine=%d outside 1..6", combine);
    return 0;
}

// ---- The denoising objective evaluated forward (denoise_loss.hip): the noised model input and the loss against the regenerated target.
static int fill_denoise(const char* who, const lavie_denoise_args* a, const lavie_noise_key* k, NoiseKey* key, NoiseLevels* lv,
                        OffsetNoise* off) {
    LAVIE_CHECK(a, "%s: args is null", who);
    LAVIE_CHECK(a->struct_size == (int)sizeof(lavie_denoise_args),
                "%s: args->struct_size=%d but this library's lavie_denoise_args has %d bytes: the binding's struct layout is out of date", who,
                a->struct_size, (int)sizeof(lavie_denoise_args));
    if (int rc = fill_key(who, k, key)) return rc;
    LAVIE_CHECK(a->x0_dtype == 0 || a->x0_dtype == 1, "%s: x0_dtype=%d outside 0..1", who, a->x0_dtype);
    LAVIE_CHECK(a->x0, "%s: x0 is null", who);
    LAVIE_CHECK(((uintptr_t)a->x0 & (a->x0_dtype ? 3 : 1)) == 0, "%s: x0 at %p is not aligned to its element", who, a->x0);
    LAVIE_CHECK(a->a_host && a->s_host, "%s: %s is null", who, a->a_host ? "s_host" : "a_host");
    LAVIE_CHECK(a->offset_hw >= 0 && (a->offset_hw == 0 || key->per % a->offset_hw == 0), "%s: offset_hw=%lld must be 0 or divide per=%lld",
                who, a->offset_hw, key->per);
    *lv = NoiseLevels{};
    for (int p = 0; p < key->count; ++p) {
        LAVIE_CHECK(__builtin_isfinite(a->a_host[p]) && __builtin_isfinite(a->s_host[p]), "%s: level %d (a=%g, s=%g) is not finite", who, p,
                    (double)a->a_host[p], (double)a->s_host[p]);
        lv->a[p] = a->a_host[p];
        lv->s[p] = a->s_host[p];
    }
    *off = OffsetNoise{0.f, 0ull, 0ll};
    if (a->offset_hw != 0) {
        LAVIE_CHECK(__builtin_isfinite(a->offset_coef), "%s: offset_coef (%g) is not finite", who, (double)a->offset_coef);
        *off = OffsetNoise{a->offset_coef, a->offset_draw, a->offset_hw};
    }
    return 0;
}

int lavie_noisy_latents_seeded(const lavie_denoise_args* a, const lavie_noise_key* k, void* model_in, void* stream) {
    const char* who = "noisy_latents_seeded";
    NoiseKey key;
    NoiseLevels lv;
    OffsetNoise off;
    if (int rc = fill_denoise(who, a, k, &key, &lv, &off)) return rc;
    LAVIE_CHECK(model_in, "%s: model_in is null", who);
    LAVIE_CHECK(((uintptr_t)model_in & 1) == 0, "%s: model_in at %p is not 2-byte aligned", who, model_in);
    return launch_noisy_latents(a->x0, a->x0_dtype == 1, static_cast<half_t*>(model_in), key, lv, off, S(stream));
}

long long lavie_denoising_loss_workspace_floats(int P, long long per) {
    if (P < 1 || per < 1 || per > (1ll << 40)) return -1;
    return (long long)P * denoising_loss_chunks(per);
}

int lavie_denoising_loss_f32(const lavie_denoise_args* a, const lavie_noise_key* k, const void* pred, int kind, float* out, float* workspace,
                             long long workspace_floats, void* stream) {
    const char* who = "denoising_loss";
    NoiseKey key;
    NoiseLevels lv;
    OffsetNoise off;
    if (int rc = fill_denoise(who, a, k, &key, &lv, &off)) return rc;
    LAVIE_CHECK(pred, "%s: pred is null", who);
    LAVIE_CHECK(((uintptr_t)pred & 1) == 0, "%s: pred at %p is not 2-byte aligned", who, pred);
    LAVIE_CHECK(kind >= 0 && kind <= 2, "%s: kind=%d outside 0..2", who, kind);
    LAVIE_CHECK(out, "%s: out is null", who);
    LAVIE_CHECK(workspace, "%s: workspace is null", who);
    LAVIE_CHECK((((uintptr_t)out | (uintptr_t)workspace) & 3) == 0, "%s: out / workspace is not 4-byte aligned", who);
    const long long need = lavie_denoising_loss_workspace_floats(key.count, key.per);
    LAVIE_CHECK(workspace_floats >= need, "%s: workspace_floats=%lld, P chunks = %lld needed", who, workspace_floats, need);
    return launch_denoising_loss(static_cast<const half_t*>(pred), a->x0, a->x0_dtype == 1, key, lv, off, kind, workspace, out, S(stream));
}

// ---- Guidance from a per-latent table (sampler_guidance.hip): the table itself, then the five steps that read it.
long long lavie_guidance_partials_floats(int latents, long long per) {
    if (latents < 1 || per < 2 || per > (1ll << 40)) return -1;
    return (long long)latents * guidance_chunks(per) * 4;
}

int lavie_guidance_table(const lavie_guidance_table_args* a, void* stream) {
    const char* who = "guidance_table";
    LAVIE_CHECK(a, "%s: args is null", who);
    LAVIE_CHECK(a->struct_size == (int)sizeof(lavie_guidance_table_args),
                "%s: args->struct_size=%d but this library's lavie_guidance_table_args has %d bytes: the binding's struct layout is "
                "out of date", who, a->struct_size, (int)sizeof(lavie_guidance_table_args));
    LAVIE_CHECK(a->W >= 1 && a->W <= LAVIE_WINDOW_MAX_WINDOWS, "%s: W=%d outside 1..%d", who, a->W, LAVIE_WINDOW_MAX_WINDOWS);
    LAVIE_CHECK(a->P >= 1 && (long long)a->W * a->P <= 65535, "%s: P=%d: W P must be in 1..65535", who, a->P);
    LAVIE_CHECK(a->per >= 2 && a->per <= (1ll << 40), "%s: per=%lld must be >= 2 (an unbiased deviation needs two elements)", who, a->per);
    LAVIE_CHECK(a->eps_host, "%s: eps_host is null", who);
    for (int w = 0; w < a->W; ++w) {
        LAVIE_CHECK(a->eps_host[w], "%s: eps[%d] is null", who, w);
        LAVIE_CHECK(a->per % 8 != 0 || ((uintptr_t)a->eps_host[w] & 15) == 0, "%s: eps[%d] at %p is not 16-byte aligned", who, w, a->eps_host[w]);
    }
    LAVIE_CHECK(__builtin_isfinite(a->guidance), "%s: guidance (%g) is not finite", who, (double)a->guidance);
    LAVIE_CHECK(a->rescale >= 0.f && a->rescale <= 1.f, "%s: rescale=%g must be in [0, 1]", who, (double)a->rescale);
    LAVIE_CHECK(a->table, "%s: table is null", who);
    if (a->rescale != 0.f) {
        const long long need = lavie_guidance_partials_floats(a->W * a->P, a->per);
        LAVIE_CHECK(a->partials, "%s: partials is null but rescale=%g", who, (double)a->rescale);
        LAVIE_CHECK(a->partials_floats >= need, "%s: partials_floats=%lld, W P chunks 4 = %lld needed", who, a->partials_floats, need);
        LAVIE_CHECK(((uintptr_t)a->partials & 15) == 0, "%s: partials at %p is not 16-byte aligned", who, (const void*)a->partials);
    }
    LAVIE_CHECK(((uintptr_t)a->moments & 7) == 0, "%s: moments at %p is not 8-byte aligned", who, (const void*)a->moments);
    return launch_guidance_table(reinterpret_cast<const half_t* const*>(a->eps_host), a->W, a->P, a->per, a->guidance_dev, a->guidance,
                                 a->rescale, a->partials, a->table, a->moments, S(stream));
}

int lavie_cfg_sampler_step_scaled(const void* eps2, float* x, const float* noise, void* model_in2, long long n, const float* table,
                                  long long per, float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale,
                                  void* stream) {
    LAVIE_CHECK(table, "cfg_sampler_step_scaled: table is null");
    return run_step("cfg_sampler_step_scaled", step_args(false, true, eps2, x, noise, model_in2, n, 1.0f, k_x, k_eps, c_x0, c_xt, sigma,
                                                         next_input_scale, table, per), stream);
}

int lavie_cfg_multistep_step_scaled(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, const float* table,
                                    long long per, float k_x, float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale,
                                    void* stream) {
    LAVIE_CHECK(table, "cfg_multistep_step_scaled: table is null");
    return run_step("cfg_multistep_step_scaled", step_args(true, true, eps2, x, x0_prev, model_in2, n, 1.0f, k_x, k_eps, c_x0, c_xt,
                                                           c_prev, next_input_scale, table, per), stream);
}

int lavie_cfg_sampler_step_known_scaled(const void* eps2, float* x, const float* noise, void* model_in2, long long n, const float* table,
                                        float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, void* stream,
                                        const lavie_known_region* region) {
    LAVIE_CHECK(table, "cfg_sampler_step_known_scaled: table is null");
    return run_step_known("cfg_sampler_step_known_scaled", step_args(false, true, eps2, x, noise, model_in2, n, 1.0f, k_x, k_eps, c_x0,
                                                                     c_xt, sigma, next_input_scale, table), region, stream);
}

int lavie_cfg_multistep_step_known_scaled(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, const float* table,
                                          float k_x, float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale,
                                          void* stream, const lavie_known_region* region) {
    LAVIE_CHECK(table, "cfg_multistep_step_known_scaled: table is null");
    return run_step_known("cfg_multistep_step_known_scaled", step_args(true, true, eps2, x, x0_prev, model_in2, n, 1.0f, k_x, k_eps, c_x0,
                                                                       c_xt, c_prev, next_input_scale, table), region, stream);
}

// ---- the UniPC step (sampler_unipc.hip): every refusal on the host, before any HIP call, naming its argument
static int run_unipc(const char* who, bool cfg, const void* eps, float* x, float* x_last, float* m1, float* m2, void* model_in,
                     long long n, const float* table, long long per, const lavie_unipc_coeffs& k, void* stream) {
    LAVIE_CHECK(k.struct_size == (int)sizeof(lavie_unipc_coeffs),
                "%s: coeffs.struct_size=%d but this library's lavie_unipc_coeffs has %d bytes: the binding's struct layout is out of "
                "date", who, k.struct_size, (int)sizeof(lavie_unipc_coeffs));
    const void* const t[6] = {eps, x, x_last, m1, m2, model_in};
    const char* const names[6] = {"eps", "x", "x_last", "m1", "m2", "model_in"};
    for (int i = 0; i < 6; ++i) LAVIE_CHECK(t[i], "%s: null argument: %s is null", who, names[i]);
    LAVIE_CHECK(n >= 1 && n <= (1ll << 40), "%s: n=%lld must be >= 1", who, n);
    const float s[11] = {k.guidance, k.k_x, k.k_eps, k.c_l, k.c_0, k.c_1, k.c_2, k.p_x, k.p_0, k.p_1, k.next_input_scale};
    const char* const snames[11] = {"guidance", "k_x", "k_eps", "c_l", "c_0", "c_1", "c_2", "p_x", "p_0", "p_1", "next_input_scale"};
    for (int i = 0; i < 11; ++i) LAVIE_CHECK(__builtin_isfinite(s[i]), "%s: %s (%g) is not finite", who, snames[i], (double)s[i]);
    if (table) {
        LAVIE_CHECK(per >= 2 && per <= (1ll << 40), "%s: per=%lld must be >= 2", who, per);
        LAVIE_CHECK(n % per == 0, "%s: n=%lld is not a whole number of latents of per=%lld", who, n, per);
        LAVIE_CHECK(n / per <= 65535, "%s: n / per = %lld latents, at most 65535 fit one launch", who, n / per);
    }
    // the four fp32 tensors are each read and rewritten at the same element only, so none may share a byte with another
    for (int i = 1; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) {
            const uintptr_t a = (uintptr_t)t[i], b = (uintptr_t)t[j], bytes = (uintptr_t)n * 4;
            LAVIE_CHECK(a + bytes <= b || b + bytes <= a, "%s: %s and %s overlap", who, names[i], names[j]);
        }
    if ((table ? per : n) % 8 == 0)          // the eight-elements-per-lane form: 16-byte accesses
        for (int i = 0; i < 6; ++i)
            if (int rc = check_aligned(who, names[i], t[i])) return rc;
    UnipcArgs a{};
    a.cfg = cfg; a.eps = H(eps); a.x = x; a.x_last = x_last; a.m1 = m1; a.m2 = m2; a.model_in = H(model_in); a.n = n;
    a.c = UnipcCoef{table ? 1.0f : k.guidance, k.k_x, k.k_eps, k.c_l, k.c_0, k.c_1, k.c_2, k.p_x, k.p_0, k.p_1, k.next_input_scale,
                    k.corr != 0};
    a.table = table; a.per = per;
    return launch_unipc_step(a, S(stream));
}

int lavie_unipc_step(const void* eps, float* x, float* x_last, float* m1, float* m2, void* model_in, long long n,
                     lavie_unipc_coeffs coeffs, void* stream) {
    return run_unipc("unipc_step", false, eps, x, x_last, m1, m2, model_in, n, nullptr, 0, coeffs, stream);
}

int lavie_cfg_unipc_step(const void* eps2, float* x, float* x_last, float* m1, float* m2, void* model_in2, long long n,
                         lavie_unipc_coeffs coeffs, void* stream) {
    return run_unipc("cfg_unipc_step", true, eps2, x, x_last, m1, m2, model_in2, n, nullptr, 0, coeffs, stream);
}

int lavie_cfg_unipc_step_scaled(const void* eps2, float* x, float* x_last, float* m1, float* m2, void* model_in2, long long n,
                                const float* table, long long per, lavie_unipc_coeffs coeffs, void* stream) {
    LAVIE_CHECK(table, "cfg_unipc_step_scaled: table is null");
    return run_unipc("cfg_unipc_step_scaled", true, eps2, x, x_last, m1, m2, model_in2, n, table, per, coeffs, stream);
}

int lavie_window_step_scaled(const lavie_window_step_args* a, const float* table, void* stream) {
    const char* who = "window_step_scaled";
    LAVIE_CHECK(table, "%s: table is null", who);
    LAVIE_CHECK(!a || a->cfg != 0, "%s: cfg=0: the table holds guidance scales, the call must be guided", who);
    return window_step(who, a, table, stream);
}

int lavie_latents_to_scaled_model_input1(const float* x, void* model_in, long long n, float input_scale, void* stream) {
    LAVIE_CHECK(x && model_in && n > 0, "latents_to_scaled_model_input1: bad arguments");
    return launch_f32_to_f16_scaled(x, H(model_in), n, input_scale, S(stream));
}

int lavie_latents_to_model_input(const float* x, void* model_in2, long long n, void* stream) {
    LAVIE_CHECK(x && model_in2 && n > 0, "latents_to_model_input: bad arguments");
    return launch_f32_to_f16_dup2(x, H(model_in2), n, 1.0f, S(stream));
}

int lavie_latents_to_scaled_model_input(const float* x, void* model_in2, long long n, float input_scale, void* stream) {
    LAVIE_CHECK(x && model_in2 && n > 0, "latents_to_scaled_model_input: bad arguments");
    return launch_f32_to_f16_dup2(x, H(model_in2), n, input_scale, S(stream));
}

// Every switch below changes which kernels a forward enqueues: each bumps the process-wide debug epoch, which is part of
// the captured graph's key (engine.h GraphKey::debug_epoch), so a replay never runs a selection made under other switches.
int lavie_debug_force_tile(int mode) {
    if (int rc = igemm_force_tile(mode)) return rc;     // a rejected mode changes nothing
    bump_debug_epoch();
    return 0;
}
int lavie_debug_force_splits(int s) { bump_debug_epoch(); igemm_force_splits(s); return 0; }
int lavie_debug_fused_mask(int mask) {
    LAVIE_CHECK((mask & ~0x177) == 0, "fused_mask: 0x%x sets a bit other than 0, 1, 2, 4, 5, 6, 8", mask);
    bump_debug_epoch();
    set_fused_mask(mask);
    return 0;
}
int lavie_debug_temporal_budget(int bytes) { bump_debug_epoch(); temporal_set_budget(bytes); return 0; }
int lavie_debug_rowfuse_grid(int max_workgroups) {
    if (int rc = rowfuse_set_grid_cap(max_workgroups)) return rc;     // a rejected value changes nothing
    bump_debug_epoch();
    return 0;
}
long long lavie_debug_gn_producer_count(void) { return (long long)lavie::gn_producer_count(); }

// ---- producer-side norm statistics at operator level (tests/statcheck.py): additive entries, the ABI number stays.  None of them
// changes which kernels a forward enqueues, so none bumps the debug epoch.
int lavie_debug_op_statistics(float* colstat, long long colstat_floats, float* rowstat, long long rowstat_floats) {
    LAVIE_CHECK(colstat_floats >= 0 && rowstat_floats >= 0, "op_statistics: negative buffer size");
    const bool cs = colstat && colstat_floats > 0, rs = rowstat && rowstat_floats > 0;
    g_sink_cs = cs ? colstat : nullptr; g_sink_cs_floats = cs ? colstat_floats : 0;
    g_sink_rs = rs ? rowstat : nullptr; g_sink_rs_floats = rs ? rowstat_floats : 0;
    return 0;
}
int lavie_debug_op_statistics_plan(int colstat, int rowstat) {
    g_plan_cs = colstat != 0;
    g_plan_rs = rowstat != 0;
    return 0;
}
int lavie_debug_op_statistics_last(lavie_op_statistics_info* out) {
    LAVIE_CHECK(out, "op_statistics_last: out is null");
    LAVIE_CHECK(out->struct_size == (int)sizeof(lavie_op_statistics_info),
                "op_statistics_last: out->struct_size=%d but this library's lavie_op_statistics_info has %d bytes: the binding's struct "
                "layout is out of date", out->struct_size, (int)sizeof(lavie_op_statistics_info));
    LAVIE_CHECK(g_stats_last.struct_size != 0, "op_statistics_last: no operator-level GEMM launch so far");
    *out = g_stats_last;
    return 0;
}

// one producer-statistics descriptor of lavie_group_norm_stats_f16 -> GnColStat, after the checks that keep the fold's reads inside
// `partials` whichever path launch_group_norm then takes
static int gn_descriptor(const char* which, const lavie_gn_producer_stats* d, int NB, int P, GnColStat* cs) {
    *cs = GnColStat();
    if (!d) return 0;
    LAVIE_CHECK(d->struct_size == (int)sizeof(lavie_gn_producer_stats),
                "group_norm_stats: %s->struct_size=%d but this library's lavie_gn_producer_stats has %d bytes: the binding's struct layout "
                "is out of date", which, d->struct_size, (int)sizeof(lavie_gn_producer_stats));
    LAVIE_CHECK(d->partials, "group_norm_stats: %s->partials is null", which);
    LAVIE_CHECK(d->C > 0 && d->rows > 0 && d->nsets >= 1 && d->set_blocks >= 1 && d->span > 0,
                "group_norm_stats: %s has C=%d rows=%d nsets=%d set_blocks=%d span=%d, all must be >= 1", which, d->C, d->rows, d->nsets,
                d->set_blocks, d->span);
    const long long need = (long long)d->nsets * d->set_blocks * 2 * d->C;
    LAVIE_CHECK(d->partials_floats >= need, "group_norm_stats: %s->partials_floats=%lld, %d sets of %d blocks of %d channels need %lld", which,
                d->partials_floats, d->nsets, d->set_blocks, d->C, need);
    const long long per_domain = (long long)d->rows * d->nsets;
    LAVIE_CHECK(P % per_domain != 0 || (long long)NB * (P / per_domain) <= d->set_blocks,
                "group_norm_stats: %s describes %d blocks per set, %d domains of %lld need %lld", which, d->set_blocks, NB, P / per_domain,
                (long long)NB * (P / per_domain));
    cs->partials = d->partials; cs->C = d->C; cs->rows = d->rows; cs->nsets = d->nsets; cs->set_blocks = d->set_blocks; cs->span = d->span;
    return 0;
}
int lavie_group_norm_stats_f16(const void* x1, int C1, const void* x2, int C2, int NB, int P, int groups, const float* gamma,
                               const float* beta, float eps, int silu, float* stats_ws, void* y, const lavie_gn_producer_stats* cs1,
                               const lavie_gn_producer_stats* cs2, void* stream) {
    LAVIE_CHECK(x1 && gamma && beta && stats_ws && y, "group_norm_stats: null tensor");
    LAVIE_CHECK(NB > 0 && P > 0 && groups > 0, "group_norm_stats: empty problem");
    if (!x2) C2 = 0;
    GnColStat a, b;
    if (int rc = gn_descriptor("cs1", cs1, NB, P, &a)) return rc;
    if (int rc = gn_descriptor("cs2", x2 ? cs2 : nullptr, NB, P, &b)) return rc;
    return launch_group_norm(H(x1), C1, H(x2), C2, NB, P, groups, gamma, beta, eps, silu != 0, stats_ws, H(y), S(stream), cs1 ? &a : nullptr,
                             x2 && cs2 ? &b : nullptr);
}
int lavie_rowstat_finalize_f32(const float* partials, int slots, int M, int row_len, float eps, float* out, void* stream) {
    LAVIE_CHECK(partials && out, "rowstat_finalize: null tensor");
    LAVIE_CHECK(slots >= 1 && M >= 1 && row_len >= 1, "rowstat_finalize: slots=%d M=%d row_len=%d must be >= 1", slots, M, row_len);
    LAVIE_CHECK(__builtin_isfinite(eps) && eps >= 0.f, "rowstat_finalize: eps=%g must be finite and >= 0", (double)eps);
    return launch_rowstat_finalize(partials, slots, M, row_len, eps, out, S(stream));
}

int lavie_profile_begin(unsigned mask, int max_events) { return profile_begin(mask, max_events); }

int lavie_profile_end(void* stream, long long* launches_host, double* ms_host, double* flops_host, double* bytes_host) {
    LAVIE_CHECK(launches_host && ms_host && flops_host && bytes_host, "profile_end: null output");
    return profile_end(S(stream), launches_host, ms_host, flops_host, bytes_host);
}

int lavie_unet_config_size(void) { return (int)sizeof(lavie_unet_config); }

int lavie_unet_create(const lavie_unet_config* cfg, lavie_unet_t* out) {
    LAVIE_CHECK(cfg && out, "unet_create: null argument");
    // read only the first int until the caller's layout is known to be this build's
    LAVIE_CHECK(cfg->struct_size == (int)sizeof(lavie_unet_config),
                "unet_create: cfg->struct_size=%d but this library's lavie_unet_config has %d bytes (ABI %d): the binding's struct "
                "layout is out of date", cfg->struct_size, (int)sizeof(lavie_unet_config), LAVIE_ABI_VERSION);
    LAVIE_CHECK(cfg->num_levels >= 1 && cfg->num_levels <= LAVIE_MAX_LEVELS, "unet_create: num_levels=%d", cfg->num_levels);
    lavie_unet_s* h = new (std::nothrow) lavie_unet_s(*cfg);
    LAVIE_CHECK(h != nullptr, "unet_create: out of host memory");
    if (int rc = h->net.validate_config()) {
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

int lavie_unet_destroy(lavie_unet_t h) {
    delete h;
    return 0;
}

int lavie_unet_num_params(lavie_unet_t h) { return h ? (int)h->net.params().size() : -1; }

int lavie_unet_param_info(lavie_unet_t h, int i, const char** name, long long* numel) {
    LAVIE_CHECK(h && i >= 0 && i < (int)h->net.params().size(), "param_info: index %d out of range", i);
    if (name) *name = h->net.params()[i].name.c_str();
    if (numel) *numel = h->net.params()[i].numel;
    return 0;
}

int lavie_unet_set_param(lavie_unet_t h, const char* name, const void* data_f16, long long numel) {
    LAVIE_CHECK(h && name, "set_param: null argument");
    return h->net.set_param(name, data_f16, numel);
}

int lavie_unet_finalize(lavie_unet_t h, void* stream) {
    LAVIE_CHECK(h, "finalize: null handle");
    return h->net.finalize(S(stream));
}

int lavie_unet_prepare(lavie_unet_t h, int B, int F, int Hh, int W, int ctx_len) {
    LAVIE_CHECK(h, "prepare: null handle");
    return h->net.prepare(B, F, Hh, W, ctx_len);
}

int lavie_unet_cache_context(lavie_unet_t h, const void* ctx, int B, int ctx_len, void* stream) {
    LAVIE_CHECK(h, "cache_context: null handle");
    return h->net.cache_context(H(ctx), B, ctx_len, S(stream));
}

int lavie_unet_lora_set(lavie_unet_t h, const char* name, const void* base_f16, const float* A, const float* B, int r, float scale,
                        void* stream) {
    LAVIE_CHECK(h, "lora_set: null handle");
    return h->net.lora_set(name, H(base_f16), A, B, r, scale, S(stream));
}
int lavie_unet_lora_clear(lavie_unet_t h, const char* name, void* stream) {
    LAVIE_CHECK(h, "lora_clear: null handle");
    return h->net.lora_clear(name, S(stream));
}
int lavie_unet_lora_set_slot(lavie_unet_t h, int slot, const char* name, const void* base_f16, const float* A, const float* B, int r,
                             float scale, void* stream) {
    LAVIE_CHECK(h, "lora_set_slot: null handle");
    return h->net.lora_set_slot(slot, name, H(base_f16), A, B, r, scale, S(stream));
}
int lavie_unet_lora_clear_slot(lavie_unet_t h, int slot, const char* name, void* stream) {
    LAVIE_CHECK(h, "lora_clear_slot: null handle");
    return h->net.lora_clear_slot(slot, name, S(stream));
}
int lavie_unet_lora_set_slot_weight(lavie_unet_t h, int slot, float weight) {
    LAVIE_CHECK(h, "lora_set_slot_weight: null handle");
    return h->net.lora_set_slot_weight(slot, weight);
}
int lavie_unet_lora_set_scale(lavie_unet_t h, float scale) {
    LAVIE_CHECK(h, "lora_set_scale: null handle");
    return h->net.lora_set_scale(scale);
}
int lavie_unet_lora_apply(lavie_unet_t h, void* stream) {
    LAVIE_CHECK(h, "lora_apply: null handle");
    return h->net.lora_apply(S(stream));
}

int lavie_unet_set_cfg_shared_input(lavie_unet_t h, int on) {
    LAVIE_CHECK(h, "set_cfg_shared_input: null handle");
    h->net.set_cfg_shared_input(on != 0);
    return 0;
}
int lavie_unet_set_freeu(lavie_unet_t h, float s1, float s2, float b1, float b2) {
    LAVIE_CHECK(h, "set_freeu: null handle");
    return h->net.set_freeu(s1, s2, b1, b2);
}
int lavie_unet_set_pag(lavie_unet_t h, const char* const* layers_host, int n_layers, int perturbed) {
    LAVIE_CHECK(h, "set_pag: null handle");
    return h->net.set_pag(layers_host, n_layers, perturbed);
}
int lavie_unet_set_ln_fold(lavie_unet_t h, int on) {
    LAVIE_CHECK(h, "set_ln_fold: null handle");
    h->net.set_ln_fold(on != 0);
    return 0;
}

long long lavie_unet_weight_bytes(lavie_unet_t h) { return h ? h->net.weight_bytes() : -1; }
long long lavie_unet_workspace_bytes(lavie_unet_t h) { return h ? h->net.workspace_bytes() : -1; }

int lavie_unet_forward(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx, void* out, int B,
                       int F, int Hh, int W, int ctx_len, void* stream) {
    LAVIE_CHECK(h, "forward: null handle");
    return h->net.forward(H(sample), timesteps, H(ctx), H(out), B, F, Hh, W, ctx_len, S(stream), nullptr);
}

int lavie_unet_forward_graph(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx, void* out, int B,
                             int F, int Hh, int W, int ctx_len, void* stream) {
    LAVIE_CHECK(h, "forward_graph: null handle");
    return h->net.forward_graph(H(sample), timesteps, H(ctx), H(out), B, F, Hh, W, ctx_len, S(stream));
}

int lavie_unet_forward_labels(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx,
                              const int* class_labels_host, void* out, int B, int F, int Hh, int W, int ctx_len, void* stream) {
    LAVIE_CHECK(h && class_labels_host, "forward_labels: null handle / labels");
    return h->net.forward(H(sample), timesteps, H(ctx), H(out), B, F, Hh, W, ctx_len, S(stream), class_labels_host);
}

int lavie_unet_set_layer_cache(lavie_unet_t h, int depth) {
    LAVIE_CHECK(h, "set_layer_cache: null handle");
    return h->net.set_layer_cache(depth);
}
long long lavie_unet_layer_cache_bytes(lavie_unet_t h) { return h ? h->net.layer_cache_bytes() : -1; }

int lavie_unet_forward_cached(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx, const int* class_labels_host,
                              void* out, int B, int F, int Hh, int W, int ctx_len, int mode, void* stream) {
    LAVIE_CHECK(h, "forward_cached: null handle");
    LAVIE_CHECK(mode >= LAVIE_LAYER_CACHE_OFF && mode <= LAVIE_LAYER_CACHE_REUSE, "forward_cached: mode=%d must be 0 (off), 1 (refresh) or 2 (reuse)",
                mode);
    return h->net.forward(H(sample), timesteps, H(ctx), H(out), B, F, Hh, W, ctx_len, S(stream), class_labels_host, mode);
}

int lavie_unet_resnet_forward(lavie_unet_t h, const char* prefix, const void* x1, int C1, const void* x2, int C2,
                              const float* temb, void* y, int B, int F, int Hh, int W, void* stream) {
    LAVIE_CHECK(h && prefix && x1 && temb && y, "resnet_forward: null argument");
    return h->net.resnet_forward(prefix, H(x1), C1, H(x2), C2, temb, H(y), B, F, Hh, W, S(stream));
}

int lavie_unet_transformer_forward(lavie_unet_t h, const char* prefix, void* x_inout, const void* ctx, int B, int F, int Hh,
                                   int W, int ctx_len, void* stream) {
    LAVIE_CHECK(h && prefix && x_inout && ctx, "transformer_forward: null argument");
    return h->net.transformer_forward(prefix, H(x_inout), H(ctx), B, F, Hh, W, ctx_len, S(stream));
}

// ---- text encoder (text_encoder.hip, text_engine.cpp)
int lavie_causal_attention_f16(const void* qkv, int ld, void* o, int ldo, int NB, int L, int heads, int dh, float scale, void* stream) {
    return launch_causal_attention(H(qkv), ld, H(o), ldo, NB, L, heads, dh, scale, S(stream));
}

int lavie_token_embed_f16(const int* ids_dev, const void* tok_table, const void* pos_table, void* out, int B, int L, int C, int V,
                          void* stream) {
    return launch_token_embed(ids_dev, H(tok_table), H(pos_table), H(out), B, L, C, V, S(stream));
}

int lavie_act_f16(void* x, long long n, int kind, void* stream) { return launch_act(H(x), n, kind, S(stream)); }

int lavie_text_config_size(void) { return (int)sizeof(lavie_text_config); }

int lavie_text_create(const lavie_text_config* cfg, lavie_text_t* out) { return encoder_create("text", cfg, out); }
int lavie_text_destroy(lavie_text_t h) { return encoder_destroy(h); }
int lavie_text_num_params(lavie_text_t h) { return encoder_num_params(h); }
int lavie_text_param_info(lavie_text_t h, int i, const char** name, long long* numel) { return encoder_param_info("text", h, i, name, numel); }
int lavie_text_set_param(lavie_text_t h, const char* name, const void* data_f16, long long numel) {
    return encoder_set_param("text", h, name, data_f16, numel);
}
int lavie_text_finalize(lavie_text_t h, void* stream) { return encoder_finalize("text", h, stream); }
long long lavie_text_workspace_bytes(lavie_text_t h, int B, int L) { return encoder_workspace_bytes("text", h, B, L); }

int lavie_text_encode(lavie_text_t h, const int* ids_dev, int B, int L, void* out_f16, void* stream) {
    LAVIE_CHECK(h, "text_encode: null handle");
    return h->enc.encode(ids_dev, B, L, out_f16, S(stream));
}

// ---- image conditioning (image_encoder.hip, image_engine.cpp)
int lavie_short_attention_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int NB, int Lq,
                              int Lk, int heads, int dh, float scale, void* stream) {
    return launch_short_attention(H(q), ldq, H(k), ldk, H(v), ldv, H(o), ldo, NB, Lq, Lk, heads, dh, scale, false, S(stream));
}

int lavie_patch_embed_k(int P) { return P >= 1 && P <= 64 ? patch_embed_k(P) : -1; }

long long lavie_patch_embed_workspace_bytes(int B, int S_, int P) { return patch_embed_workspace_bytes(B, S_, P); }

int lavie_pack_patch_embed_f16(const void* w, void* out, int C, int P, void* stream) {
    return launch_pack_patch_embed(H(w), H(out), C, P, S(stream));
}

int lavie_patch_embed_f16(const void* pixel_values, int x_dtype, const void* wp, const void* class_embedding, const void* pos_table,
                          void* out, void* workspace, int B, int S_, int P, int C, void* stream) {
    LAVIE_CHECK(x_dtype == 0 || x_dtype == 1, "patch_embed: x_dtype=%d (0 = fp16, 1 = fp32)", x_dtype);
    return launch_patch_embed(pixel_values, x_dtype == 1, H(wp), H(class_embedding), H(pos_table), H(out), H(workspace), B, S_, P, C,
                              S(stream));
}

int lavie_relu_f16(void* x, long long n, void* stream) { return launch_relu(H(x), n, S(stream)); }

int lavie_vision_config_size(void) { return (int)sizeof(lavie_vision_config); }

int lavie_vision_create(const lavie_vision_config* cfg, lavie_vision_t* out) { return encoder_create("vision", cfg, out); }
int lavie_vision_destroy(lavie_vision_t h) { return encoder_destroy(h); }
int lavie_vision_num_params(lavie_vision_t h) { return encoder_num_params(h); }
int lavie_vision_param_info(lavie_vision_t h, int i, const char** name, long long* numel) { return encoder_param_info("vision", h, i, name, numel); }
int lavie_vision_set_param(lavie_vision_t h, const char* name, const void* data_f16, long long numel) {
    return encoder_set_param("vision", h, name, data_f16, numel);
}
int lavie_vision_finalize(lavie_vision_t h, void* stream) { return encoder_finalize("vision", h, stream); }
long long lavie_vision_workspace_bytes(lavie_vision_t h, int B) { return encoder_workspace_bytes("vision", h, B); }

int lavie_vision_encode(lavie_vision_t h, const void* pixel_values, int x_dtype, int B, void* out_f16, void* stream) {
    LAVIE_CHECK(h, "vision_encode: null handle");
    return h->enc.encode(pixel_values, x_dtype, B, out_f16, S(stream));
}

int lavie_mapper_config_size(void) { return (int)sizeof(lavie_mapper_config); }

int lavie_mapper_create(const lavie_mapper_config* cfg, lavie_mapper_t* out) { return encoder_create("mapper", cfg, out); }
int lavie_mapper_destroy(lavie_mapper_t h) { return encoder_destroy(h); }
int lavie_mapper_num_params(lavie_mapper_t h) { return encoder_num_params(h); }
int lavie_mapper_param_info(lavie_mapper_t h, int i, const char** name, long long* numel) { return encoder_param_info("mapper", h, i, name, numel); }
int lavie_mapper_set_param(lavie_mapper_t h, const char* name, const void* data_f16, long long numel) {
    return encoder_set_param("mapper", h, name, data_f16, numel);
}
int lavie_mapper_finalize(lavie_mapper_t h, void* stream) { return encoder_finalize("mapper", h, stream); }
long long lavie_mapper_workspace_bytes(lavie_mapper_t h, int B) { return encoder_workspace_bytes("mapper", h, B); }

int lavie_mapper_encode(lavie_mapper_t h, const void* image_feats, int Bi, const void* text, int B, void* out, int ld_out_rows, int row0,
                        void* stream) {
    LAVIE_CHECK(h, "mapper_encode: null handle");
    return h->enc.encode(image_feats, Bi, text, B, out, ld_out_rows, row0, S(stream));
}

// the mapper's first launch: its target rows plus their positions
int lavie_add_rows_f16(const void* x, const void* pos, void* out, int B, int L, int C, void* stream) {
    return launch_add_rows(H(x), H(pos), H(out), B, L, C, S(stream));
}

// ---- CLIP image processor, feature heads, CLIPSIM (clip_engine.cpp, clip_preprocess.hip, clip_embed.hip)
int lavie_clip_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out) {
    return clip_resample_table_host(in, out, xmin_out, count_out, coeff_out);
}

long long lavie_clip_preprocess_workspace_bytes(int B, int H, int W, int size, int crop) {
    return clip_preprocess_workspace_bytes(B, H, W, size, crop);
}

int lavie_clip_preprocess_u8(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype,
                             const lavie_clip_preprocess_config* cfg, void* workspace, long long workspace_bytes, void* stream) {
    static const lavie_clip_preprocess_config clip = {(int)sizeof(lavie_clip_preprocess_config), 224, 224,
                                                      {0.48145466f, 0.4578275f, 0.40821073f}, {0.26862954f, 0.26130258f, 0.27577711f}};
    if (!cfg) cfg = &clip;
    LAVIE_CHECK(cfg->struct_size == (int)sizeof(lavie_clip_preprocess_config),
                "clip_preprocess: cfg->struct_size=%d but this library's lavie_clip_preprocess_config has %d bytes: the binding's struct "
                "layout is out of date", cfg->struct_size, (int)sizeof(lavie_clip_preprocess_config));
    return clip_preprocess(in_u8, B, H, W, row_pitch, image_pitch, out, out_dtype, cfg->size, cfg->crop, cfg->mean, cfg->std, workspace,
                           workspace_bytes, S(stream));
}

int lavie_clip_embed_f16(const void* x, int B, int L, int C, const int* ids_dev, int eos_token_id, int row, const float* ln_gamma,
                         const float* ln_beta, float eps, const void* w, int D, int normalize, float* out, void* stream) {
    return launch_clip_embed(H(x), B, L, C, ids_dev, eos_token_id, row, ln_gamma, ln_beta, eps, H(w), D, normalize != 0, out, S(stream));
}

int lavie_clip_similarity_f32(const float* img, const float* txt, float* out, int N, int P, int D, int frames, float scale, void* stream) {
    return launch_clip_similarity(img, txt, out, N, P, D, frames, scale, S(stream));
}

// ---- FVD: 3-D convolutions, the R3D-18 engine, the video processor (conv3d.hip, r3d_engine.cpp, clip_engine.cpp)
long long lavie_conv3d_packed_halfs(int Cout, int Cin, int kt, int kh, int kw) { return conv3d_packed_halfs(Cout, Cin, kt, kh, kw); }

int lavie_conv3d_pack(const void* w_f16, void* out_f16, int Cout, int Cin, int kt, int kh, int kw, void* stream) {
    return launch_conv3d_pack(H(w_f16), H(out_f16), Cout, Cin, kt, kh, kw, S(stream));
}

// the pack lavie_r3d_finalize runs for every conv: the BatchNorm behind it folded in
int lavie_conv3d_fold_pack_f32(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, double eps,
                               void* out_f16, float* shift_f32, int Cout, int Cin, int kt, int kh, int kw, void* stream) {
    return launch_conv3d_fold_pack(w, gamma, beta, mean, var, eps, H(out_f16), shift_f32, Cout, Cin, kt, kh, kw, S(stream));
}

int lavie_conv3d_f16(const void* x, const void* wp, const float* bias, const void* residual, int relu, void* y, int N, int T, int H_, int W,
                     int Cin, int Cout, int ksize, int stride, void* stream) {
    return launch_conv3d(H(x), H(wp), bias, H(residual), relu != 0, H(y), N, T, H_, W, Cin, Cout, ksize, stride, S(stream));
}

int lavie_conv3d_stem_f16(const void* pixels, int x_dtype, long long stride_n, long long stride_t, long long stride_c, const void* wp,
                          const float* bias, int relu, void* y, int N, int T, int H_, int W, void* stream) {
    LAVIE_CHECK(x_dtype == 0 || x_dtype == 1, "conv3d_stem: x_dtype=%d (0 = fp16, 1 = fp32)", x_dtype);
    return launch_conv3d_stem(pixels, x_dtype == 1, stride_n, stride_t, stride_c, H(wp), bias, relu != 0, H(y), N, T, H_, W, S(stream));
}

int lavie_mean_rows_f32(const void* x, float* out, int N, int rows, int C, void* stream) {
    return launch_mean_rows(H(x), out, N, rows, C, S(stream));
}

int lavie_r3d_create(lavie_r3d_t* out) {
    LAVIE_CHECK(out, "r3d_create: null argument");
    lavie_r3d_s* h = new (std::nothrow) lavie_r3d_s();
    LAVIE_CHECK(h != nullptr, "r3d_create: out of host memory");
    *out = h;
    return 0;
}
int lavie_r3d_destroy(lavie_r3d_t h) { return encoder_destroy(h); }
int lavie_r3d_num_params(lavie_r3d_t h) { return encoder_num_params(h); }
int lavie_r3d_param_info(lavie_r3d_t h, int i, const char** name, long long* numel) { return encoder_param_info("r3d", h, i, name, numel); }
int lavie_r3d_set_param(lavie_r3d_t h, const char* name, const void* data_f32, long long numel) {
    return encoder_set_param("r3d", h, name, data_f32, numel);
}
int lavie_r3d_finalize(lavie_r3d_t h, void* stream) { return encoder_finalize("r3d", h, stream); }
long long lavie_r3d_workspace_bytes(lavie_r3d_t h, int N, int T, int H_, int W) { return encoder_workspace_bytes("r3d", h, N, T, H_, W); }

int lavie_r3d_features(lavie_r3d_t h, const void* pixels, int x_dtype, long long stride_n, long long stride_t, long long stride_c, int N,
                       int T, int H_, int W, float* out_f32, void* workspace, long long workspace_bytes, void* stream) {
    LAVIE_CHECK(h, "r3d_features: null handle");
    return h->enc.features(pixels, x_dtype, stride_n, stride_t, stride_c, N, T, H_, W, out_f32, workspace, workspace_bytes, S(stream));
}

int lavie_video_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out) {
    return video_resample_table_host(in, out, xmin_out, count_out, coeff_out);
}

long long lavie_video_preprocess_workspace_bytes(int B, int H_, int W, int crop, int size) {
    return video_preprocess_workspace_bytes(B, H_, W, crop, size);
}

int lavie_video_preprocess_u8(const void* in_u8, int B, int H_, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype,
                              int crop, int size, const float* mean3, const float* std3, void* workspace, long long workspace_bytes,
                              void* stream) {
    return video_preprocess(in_u8, B, H_, W, row_pitch, image_pitch, out, out_dtype, crop, size, mean3, std3, workspace, workspace_bytes,
                            S(stream));
}

}  // extern "C"
