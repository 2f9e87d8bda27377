// Internal launcher declarations (host side).  Every launcher enqueues on `stream`, performs no
// allocation or synchronisation (hipGraph-capturable), and returns 0 or a negative status with
// the message available through lavie::get_error().
#pragma once
#include "common.h"
#include "igemm.h"
#include "philox.h"

namespace lavie {

// ---- norm.hip
// GroupNorm (+SiLU): statistics pass (per-slab partials), finalize (mean, rstd), apply.  `ws` is
// gn_workspace_floats(NB, groups) floats of scratch, reusable by the next call on the same stream.
size_t gn_workspace_floats(int NB, int groups);
// Producer-side statistics of one GroupNorm input tensor: what IgemmParams::colstat_out received from the kernel that stored the
// tensor (igemm.h: per (row block, channel) sum and sum of squares of the rounded fp16 values).  rows == 0 / partials == nullptr =
// none.  Parity-form upsample conv: nsets = 4 sets of set_blocks source-row blocks (a block's rows lie in ONE frame).
struct GnColStat {
    const float* partials = nullptr;
    int C = 0;            // channels of the tensor
    int rows = 0;         // rows per block
    int nsets = 1;
    int set_blocks = 0;   // blocks per set
    int span = 0;         // the rows of a block lie inside ONE aligned run of `span` tensor rows (contiguous blocks: = rows; 2-D conv
                          // tiles: one frame; temporal-conv tiles: one video): a statistics domain must be a whole number of spans
};
// What the launch of `p` under `plan` left in `buf` (p.colstat_out; p.splits as igemm_run set it): the one place that turns a plan into
// a description, for the engine (run_igemm) and the operator-level statistics sink (api.cpp) alike.
inline GnColStat gn_colstat_describe(const IgemmParams& p, const IgemmPlan& plan, const float* buf) {
    GnColStat cs;
    cs.partials = buf;
    cs.C = p.N;
    cs.rows = plan.colstat_rows;
    cs.span = plan.colstat_span;
    if (p.par_ups && p.splits == 1) { cs.nsets = 4; cs.set_blocks = p.M / 4 / plan.colstat_rows; }   // source-row blocks per output parity
    else { cs.nsets = 1; cs.set_blocks = cdiv(p.M, plan.colstat_rows); }                            // (split-K: the reduce kernel walks output rows)
    return cs;
}
// Blocks the launch stores, tile padding included: the 128-row and ping-pong kernels store every wave tile of their last row tile, also
// one whose rows all lie past M (it holds zeros: rows past M contribute nothing), so a buffer needs up to one block more than the
// nsets * set_blocks a consumer reads (engine.cpp colstat_floats has the headroom).
inline size_t gn_colstat_blocks_stored(const IgemmParams& p, const IgemmPlan& plan) {
    if (plan.colstat_rows <= 0) return 0;
    if (p.splits > 1 || (plan.kernel != IGEMM_TILE && plan.kernel != IGEMM_PP)) return (size_t)cdiv(p.M, plan.colstat_rows);
    const int bm = plan.kernel == IGEMM_TILE ? 128 : 160;
    return (size_t)cdiv(p.M, bm) * (bm / plan.colstat_rows);
}
// cs1 / cs2 (optional): statistics of x1 / x2 from their producers.  When both tensors have them and every block lies inside one
// statistics domain (P %% (rows * nsets) == 0), the statistics pass over the tensor and its finalize launch are replaced by ONE small
// fold of the partials; otherwise the two-pass path runs.
int launch_group_norm(const half_t* x1, int C1, const half_t* x2, int C2, int NB, int P, int groups, const float* gamma,
                      const float* beta, float eps, bool silu, float* ws, half_t* y, hipStream_t stream,
                      const GnColStat* cs1 = nullptr, const GnColStat* cs2 = nullptr, float* ab_out = nullptr);
// ab_out (optional, [NB][C1 + C2][2] floats): statistics only — instead of the apply pass (y is not written) the normalisation is
// handed on as per-(batch, channel) pairs (a, b), y = a x + b, for a consumer that applies it in registers (launch_proj_qkv)
long gn_producer_count();     // GroupNorm launches so far whose statistics came from the producers' epilogues (test hook)
int launch_layernorm(const half_t* x, const float* gamma, const float* beta, half_t* y, int rows, int C, float eps,
                     hipStream_t stream);

// ---- attention.hip : softmax(scale q k^T) v, heads packed along the channel axis
struct AttnParams {
    const half_t* q; int ldq;        // [NBq * Lq, ...] rows; head h at columns h*dh
    const half_t* k; int ldk;        // [NBkv * Lk, ...]
    const half_t* v; int ldv;
    half_t* o; int ldo;              // [NBq * Lq, heads*dh]
    int NBq, Lq, Lk, heads, dh;
    int kv_batch_div;                // kv batch index = q batch index / kv_batch_div (text ctx shared by the frames)
    float scale;
    // sparse-causal self-attention (interpolation/models/attention.py:609-665): sc_frames > 0 => batch entry (b, f) reads
    // keys [0, Lk/2) from frame (b, 0) and keys [Lk/2, Lk) from frame (b, max(f-1, 0)); Lk = 2 * Lq, kv_batch_div = 1
    int sc_frames = 0;
};
int launch_attention(const AttnParams& p, hipStream_t stream);
// attention_wide.hip: head dims 256 / 512, called by launch_attention (which checks the arguments and profiles the launch)
int launch_attention_wide(const AttnParams& p, hipStream_t stream);

// ---- temporal_attention.hip
struct TemporalParams {
    const half_t* qkv; int ld;       // [(b f) d, 3C]: q | k | v per token, token order (b, f, pixel)
    half_t* o; int ldo;              // [(b f) d, C]
    int B, F, D, heads, dh;          // D = pixels per frame
    const float* bias;               // [heads, F, F] relative-position bias (query i, key j)
    const float* rot_cos;            // [F, rot_dim/2]
    const float* rot_sin;
    int rot_dim;
    float scale;
};
int launch_temporal_attention(const TemporalParams& p, hipStream_t stream);
void temporal_set_budget(int bytes);   // tuning knob: LDS bytes per workgroup

// ---- elementwise.hip
int launch_timestep_sinusoid(const float* t, float* out, int B, int dim, hipStream_t stream);
// out[b, n] = act_out(sum_k act_in(in[b, k]) * W[n, k] + bias[n]);  act: 0 none, 1 SiLU
int launch_gemv(const float* in, const half_t* W, const float* bias, float* out, int B, int N, int K, int act_in,
                int act_out, hipStream_t stream);
// x [B, Cin, F, H, W] (NCFHW fp16) -> y [(B F) H W, Cout] channels-last, 3x3 pad 1; w packed [3*3*Cin][Cout]
int launch_conv_in(const half_t* x, const half_t* wp, const float* bias, half_t* y, int B, int Cin, int F, int H, int W,
                   int Cout, hipStream_t stream);
// x [(B F) H W, Cin] channels-last -> y [B, Cout, F, H, W] NCFHW fp16, 3x3 pad 1; w packed [Cout][3*3][Cin]
int launch_conv_out(const half_t* x, const half_t* wp, const float* bias, half_t* y, int B, int Cin, int F, int H, int W,
                    int Cout, hipStream_t stream);
// ---- conv_edge.hip : the narrow-channel ends of the VAE (operator level only; the engine keeps launch_conv_in / launch_conv_out)
// x [N, Cin <= 8, H, W] (NCHW, fp16 or fp32) -> y [N H W, Cout] channels-last fp16, 3x3 pad 1; tap_bias [9][Cout] or nullptr: added
// for the taps inside the image; wp from launch_pack_conv_edge_in (9 * roundup(Cin, 2) * Cout halfs)
int launch_conv_edge_in(const void* x, bool x_f32, const half_t* wp, const float* bias, const float* tap_bias, half_t* y, int N, int Cin,
                        int H, int W, int Cout, hipStream_t stream);
int launch_pack_conv_edge_in(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream);
// x [N H W, Cin] channels-last fp16 -> y [N, Cout <= 8, H, W] (NCHW, fp16 or fp32), 3x3 pad 1; wp from launch_pack_conv_edge_out
// (conv_edge_out_image_halfs(Cin) halfs; 0 = Cin not served)
int launch_conv_edge_out(const half_t* x, const half_t* wp, const float* bias, void* y, bool y_f32, int N, int Cin, int H, int W, int Cout,
                         hipStream_t stream);
int launch_pack_conv_edge_out(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream);
long long conv_edge_out_image_halfs(int Cin);
// ---- the fused scheduler steps (elementwise.hip, sampler_known.hip, sampler_guidance.hip, sampler_pag.hip): StepArgs is the one description of a step
// from the C entry points down to the launch.  Per element, fp32 (pipeline_videogen.py:679-683, scheduling_dpmsolver_multistep.py):
//   eps = cfg ? eps_u + g (eps_c - eps_u) : eps_u;  x0 = kx x - ke eps
//   five-coefficient family: x' = c0 x0 + ct x + sigma noise                     (aux = the step's noise, read when c4 = sigma != 0)
//   multistep family (DPM-Solver++ 2M): D = cp != 0 ? x0 + cp (x0 - x0_prev) : x0;  x' = c0 D + ct x;  x0_prev <- x0
//                                                                                 (aux = x0_prev, read when c4 = cp != 0, always written)
//   x <- x' in place; model_in <- fp16(x' in_scale), [2, n] = both guidance halves with cfg (eps is [2, n] then as well).
//   known != nullptr: x' = select(mask, x', a known + s noise) inside the step (sampler_known.hip); n = P * channels * inner.
//   table != nullptr (cfg only): (g, rescale factor f) per latent from table[P][2] and eps = f eps (sampler_guidance.hip); n = P per
//   (with `known` the latent is the plane's video and `per` is not read).
//   eps_pag != nullptr (sampler_pag.hip; not with `known` / `table`): perturbed-attention guidance.  eps holds one part more, [neg |
//   prompt | perturbed] with cfg, [prompt | perturbed] without; eps_pag = its last part.  e = cfg ? fma(g, ec - eu, eu) : ec, then
//   eps = pag_scale != 0 ? fma(pag_scale, ec - ep, e) : e; model_in gets the ONE fp16 value in all three (two) parts.
//   key != nullptr (sampler_noise.hip; plain five-coefficient steps only): noise[i] = the normal of (key->seed[i / per], key->draw,
//   i % per) made in registers (philox.h), read when sigma != 0; aux is not read.  Eight elements per lane when key->per % 8 == 0.
//   Every tensor must be 16-byte aligned where the eight-element form runs: the multistep family without `known` / `table`, inner % 8
//   == 0 with `known`, per % 8 == 0 with `table` alone, n % 8 == 0 with `eps_pag` (checked by the C entry points).
struct StepCoef { float guidance, kx, ke, c0, ct, c4; };     // c4: sigma (five-coefficient family) or c_prev (multistep family)
struct KnownOperands { const float* known; const float* mask; const float* noise; float a, s; };     // mask == nullptr: 1 everywhere (blend only)
struct StepArgs {
    bool multistep, cfg;
    const half_t* eps; float* x; float* aux;          // aux: the step's noise (five-coefficient) or x0_prev (multistep)
    half_t* model_in; int64_t n;
    StepCoef c; float in_scale;                       // c.guidance = 1 without cfg and with a table
    const KnownOperands* known; int channels; int64_t inner;   // known == nullptr: no region
    const float* table; int64_t per;                            // table == nullptr: scalar guidance
    const half_t* eps_pag; float pag_scale;                     // eps_pag == nullptr: no perturbed-attention guidance
    const NoiseKey* key;    // philox.h; nullptr: no key.  Plain five-coefficient steps only (launch_step refuses it with known / table /
                            // eps_pag): with c4 != 0 the noise is made in registers and aux may be null; n = key->count * key->per
};
int launch_step(const StepArgs& a, hipStream_t stream);              // picks the file by (known, table, eps_pag)
int launch_step_plain(const StepArgs& a, hipStream_t stream);        // elementwise.hip
int launch_step_known(const StepArgs& a, hipStream_t stream);        // sampler_known.hip
int launch_step_scaled(const StepArgs& a, hipStream_t stream);       // sampler_guidance.hip
int launch_step_pag(const StepArgs& a, hipStream_t stream);          // sampler_pag.hip
int launch_step_seeded(const StepArgs& a, hipStream_t stream);       // sampler_noise.hip (StepArgs::key)
// ---- sampler_unipc.hip : the UniPC predictor-corrector step (scheduling_unipc_multistep.py), a family of its own: three fp32
// history buffers (the previous corrected sample and the two previous x0 predictions) instead of StepArgs::aux.  Per element:
//   m = kx x - ke eps;  xc = corr ? cl x_last + c0 m + c1 m1 + c2 m2 : x;  x' = px xc + p0 m + p1 m1
//   x_last <- xc;  m2 <- m1;  m1 <- m;  x <- x';  model_in <- fp16(x' in_scale)      (rounding points: the file's header)
// cfg: eps / model_in are [2, n]; table != nullptr (cfg only): (g, f) per latent of `per` elements, n = P per.
struct UnipcCoef { float guidance, kx, ke, cl, c0, c1, c2, px, p0, p1, in_scale; int corr; };
struct UnipcArgs {
    bool cfg;
    const half_t* eps; float* x; float* x_last; float* m1; float* m2; half_t* model_in; int64_t n;
    UnipcCoef c;
    const float* table; int64_t per;
};
int launch_unipc_step(const UnipcArgs& a, hipStream_t stream);
// ---- sampler_noise.hip : out [P, per] fp32, row p = the normals of elements first .. first + per - 1 of latent (key.seed[p], key.draw)
// (philox.h); key.count = P <= kNoiseMaxSeeds, key.per = per.  The eight-element form runs when first % 4 == 0, per % 8 == 0 and out
// is 16-byte aligned, else every lane makes one element: the same bits.
int launch_philox_normal(float* out, const NoiseKey& key, long long first, hipStream_t stream);
// ---- denoise_loss.hip : the ends of the denoising objective evaluated forward.  lv.a[p] = sqrt(abar_t), lv.s[p] = sqrt(1 - abar_t) of
// latent p; off.hw != 0: offset noise, n += coef m with m the normal of element e / hw of (key.seed[p], off.draw) (hw divides key.per).
//   launch_noisy_latents: model_in fp16 [P, per] = once-rounded fma(s, n, a x0); x0 [P, per] fp32 or fp16.
//   launch_denoising_loss: out fp32 [P] = mean over the latent of (pred - target)^2, target by `kind`; partials holds
//   key.count * denoising_loss_chunks(key.per) floats.  Two launches, fixed order of additions.
struct NoiseLevels { float a[kNoiseMaxSeeds]; float s[kNoiseMaxSeeds]; };
struct OffsetNoise { float coef; unsigned long long draw; long long hw; };
constexpr int kLossEpsilon = 0, kLossVPrediction = 1, kLossSample = 2;
constexpr int kLossChunk = 2048;
int64_t denoising_loss_chunks(int64_t per);
int launch_noisy_latents(const void* x0, bool x0_f32, half_t* model_in, const NoiseKey& key, const NoiseLevels& lv, const OffsetNoise& off,
                         hipStream_t stream);
int launch_denoising_loss(const half_t* pred, const void* x0, bool x0_f32, const NoiseKey& key, const NoiseLevels& lv, const OffsetNoise& off,
                          int kind, float* partials, float* out, hipStream_t stream);
// ---- clip_preprocess.hip : the two passes of Pillow's 8-bit bicubic resampling over the rows and columns a centre crop keeps, and
// the normalisation by table.  The tables (device int32: first tap, tap count, [crop, ksize] coefficients per kept output; lut = 768
// fp32) are made by clip_engine.cpp.  mid: uint8 [B, rows, crop, 3], source rows row0 .. row0 + rows - 1; ymin is relative to row0.
int launch_clip_resample_h(const uint8_t* in, long long row_pitch, long long image_pitch, uint8_t* mid, int B, int row0, int rows, int crop,
                           const int* xmin, const int* cnt, const int* coeff, int ksize, hipStream_t stream);
int launch_clip_resample_v(const uint8_t* mid, void* out, bool out_f32, int B, int rows, int crop, const int* ymin, const int* cnt,
                           const int* coeff, int ksize, const float* lut, hipStream_t stream);
// ---- clip_engine.cpp : the host side of the image processor (geometry, refusals, tables in double, the cache of uploaded tables)
int clip_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out);     // returns ksize, or -1
long long clip_preprocess_workspace_bytes(int B, int H, int W, int size, int crop);
int clip_preprocess(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype, int size,
                    int crop, const float* mean3, const float* std3, void* workspace, long long workspace_bytes, hipStream_t stream);
// ---- clip_embed.hip : out fp32 [B, D] = normalise?(W LN?(x[b, row_b, :])); x fp16 [B, L, C], W fp16 [D, C]; ids_dev (int32 [B, L]) picks
// the row as CLIPTextTransformer does, otherwise `row`; gamma / beta fp32 [C] or both null.  C, D multiples of 128 up to 2048.
constexpr int kClipEmbedMaxWidth = 2048;
int launch_clip_embed(const half_t* x, int B, int L, int C, const int* ids_dev, int eos_token_id, int row, const float* gamma, const float* beta,
                      float eps, const half_t* W, int D, bool normalize, float* out, hipStream_t stream);
// frames == 0: out [N, P] = scale <img_n, txt_p>; frames >= 1 (N = P frames): out [P] = (100 / frames) sum_f <img_{p frames + f}, txt_p>
int launch_clip_similarity(const float* img, const float* txt, float* out, int N, int P, int D, int frames, float scale, hipStream_t stream);
// ---- clip_engine.cpp : the video processor of the FVD evaluator: centre crop of `crop` pixels FIRST, then Pillow's
// 8-bit bilinear resize of the cropped square to size x size, then the table; new host tables in front of the two kernels above
int video_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out);    // returns ksize, or -1
long long video_preprocess_workspace_bytes(int B, int H, int W, int crop, int size);
int video_preprocess(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype, int crop,
                     int size, const float* mean3, const float* std3, void* workspace, long long workspace_bytes, hipStream_t stream);
// ---- conv3d.hip : nn.Conv3d of the video ResNet on channels-last fp16 rows [N, T, H, W, C] (the file's header).  Packed weights
// [Cout][kpad], k = tap * Cin + ci, kpad = taps * Cin rounded up to 64 (conv3d_packed_halfs = Cout * kpad, -1 for a refused shape).
// fold_pack: fp32 weights with the following BatchNorm folded in (scale in double, one fp16 rounding; shift fp32 [Cout]).
long long conv3d_packed_halfs(int Cout, int Cin, int kt, int kh, int kw);
int launch_conv3d_pack(const half_t* w, half_t* out, int Cout, int Cin, int kt, int kh, int kw, hipStream_t stream);
int launch_conv3d_fold_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, double eps,
                            half_t* out, float* shift, int Cout, int Cin, int kt, int kh, int kw, hipStream_t stream);
// output extents floor((n - 1) / stride) + 1 of the geometries that are built; anything else is refused by name
int conv3d_out_shape(int T, int H, int W, int ksize, int stride, int* To, int* Ho, int* Wo);
int conv3d_stem_out_shape(int T, int H, int W, int* To, int* Ho, int* Wo);
// y = relu?(conv(x) + bias + R): ksize 3 (pad 1, stride 1 | 2) or 1 (stride 2); Cin, Cout in {64, 128, 256, 512}; R [rows out, Cout] or
// null, may alias y
int launch_conv3d(const half_t* x, const half_t* wp, const float* bias, const half_t* R, bool relu, half_t* y, int N, int T, int H, int W,
                  int Cin, int Cout, int ksize, int stride, hipStream_t stream);
// the (3,7,7) / (1,2,2) / (1,3,3) stem, 3 -> 64: pixel (n, t, c, h, w) at px[n stride_n + t stride_t + c stride_c + h W + w]
int launch_conv3d_stem(const void* px, bool px_f32, long long stride_n, long long stride_t, long long stride_c, const half_t* wp,
                       const float* bias, bool relu, half_t* y, int N, int T, int H, int W, hipStream_t stream);
int launch_mean_rows(const half_t* x, float* out, int N, int rows, int C, hipStream_t stream);
int launch_add_class_emb_silu(float* emb, const half_t* table, const int* labels_host, int B, int N, hipStream_t stream);
int launch_f32_to_f16_dup2(const float* x, half_t* out2, int64_t n, float in_scale, hipStream_t stream);
int launch_f32_to_f16_scaled(const float* x, half_t* out, int64_t n, float in_scale, hipStream_t stream);
// ---- sampler_known.hip : the blend that starts a run around known latents (the steps around them: StepArgs::known)
// x <- select(mask, x, a_next known + s_next noise_known) (mask == nullptr: mask = 1 everywhere); model_in = fp16(x in_scale), twice when dup
int launch_known_blend(float* x, half_t* model_in, bool dup, int64_t n, float in_scale, const float* known, const float* mask,
                       const float* noise_known, int channels, int64_t inner, float a_next, float s_next, hipStream_t stream);
// ---- sampler_window.hip : the same steps over overlapping frame windows of one long clip.  x / aux [P, C, F, hw] fp32 (aux: the
//   step's noise, or x0_prev when multistep); window w covers frames [starts[w], starts[w] + L) and owns eps[w] (read) and
//   model_in[w] (written), fp16 [nb, C, L, hw], nb = 2 P with cfg.  Per element the windows' (guided) predictions are averaged with
//   weights profile[f - starts[w]] normalised over the covering windows, then the family's plain step runs on the whole clip and
//   every covering window receives fp16(x' in_scale).  starts / profile / eps / model_in are HOST arrays, copied into the kernel
//   arguments.  The caller (lavie_window_step) has validated the schedule: sorted starts inside the clip, every frame covered by
//   1..kWindowMaxCover windows; with hw % 8 == 0 every tensor must be 16-byte aligned.
constexpr int kWindowMaxWindows = 32, kWindowMaxLength = 64, kWindowMaxCover = 4;
struct WindowStepParams {
    bool multistep, cfg;
    int P, C, F;
    int64_t hw;
    int W, L;
    const int* starts;
    const float* profile;
    const half_t* const* eps;
    half_t* const* model_in;
    float* x;
    float* aux;
    StepCoef c;
    float in_scale;
    const float* table;     // nullptr, or [W][P][2] (guidance, rescale factor) per window and latent (sampler_guidance.hip); needs cfg
    const NoiseKey* key;    // nullptr, or the step's noise made in registers (five-coefficient family, no table): aux may be null;
                            // an element's index is its index in the WHOLE clip [C, F, hw] (key->per = C F hw), so the windows do not enter it
};
int launch_window_step(const WindowStepParams& a, hipStream_t stream);
// ---- sampler_guidance.hip : guidance scale and guidance-rescale factor per latent, from device memory.
//   launch_guidance_table: eps[w] = fp16 [2 P, per] of window w (W = 1 without windows); writes partials (guidance_chunks(per) * 4
//   floats per latent, untouched when phi == 0), table[W][P] = (g_p, f_p) and, if given, moments[W][P] = the four double sums
//   (ec, ec^2, e, e^2).  g_p = guidance_dev[p] (device, may be nullptr) or `guidance`.  Two launches (one when phi == 0).
//   The scaled steps (StepArgs::table) are the guided plain steps with (g, f) = table[i / per] and eps = f e.
constexpr int kGuidanceChunk = 2048;
int64_t guidance_chunks(int64_t per);
int launch_guidance_table(const half_t* const* eps, int W, int P, int64_t per, const float* guidance_dev, float guidance, float phi,
                          float* partials, float* table, double* moments, hipStream_t stream);
int launch_fill_relpos_bias(const half_t* emb, const int* buckets, float* out, int heads, int F, hipStream_t stream);

// ---- elementwise.hip : one-off weight repacking at load time
// chunked = true: K order (64-channel slab, tap, channel) for the implicit GEMM; false: (tap, channel) for conv_out
int launch_pack_conv3x3(const half_t* w, half_t* out, int Cout, int Cin, int ld_out, int col0, bool chunked,
                        hipStream_t stream);
int launch_pack_conv3x3_parity(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream);   // [4][Cout][4 Cin], see elementwise.hip
int launch_pack_conv_taps(const half_t* w, half_t* out, int Cout, int Cin, int taps, int ld_out, int col0, bool chunked,
                          hipStream_t stream);
int launch_copy_rows(const half_t* src, int ld_src, half_t* dst, int ld_dst, int rows, int cols, int col0,
                     hipStream_t stream);
int launch_pack_geglu_rows(const half_t* w, half_t* out, int N, int K, hipStream_t stream);
int launch_pack_geglu_bias(const half_t* b, float* out, int N, hipStream_t stream);
int launch_f16_to_f32(const half_t* src, float* dst, int64_t n, hipStream_t stream);
int launch_add_f16_to_f32(const half_t* a, const half_t* b, float* dst, int64_t n, hipStream_t stream);
int launch_pack_conv_in(const half_t* w, half_t* out, int Cout, int Cin, hipStream_t stream);
// LayerNorm folding: W' = W * gamma (fp16), s = row sums of W', b' = W beta (+ bias)
int launch_ln_fold(const half_t* W, const float* gamma, const float* beta, const half_t* bias, half_t* Wout, float* s_out,
                   float* b_out, int N, int K, hipStream_t stream);
int launch_pack_geglu_vec(const float* in, float* out, int N, hipStream_t stream);

// ---- rowfuse.hip : row-resident fused transformer sub-blocks (weights streamed through LDS, rows in registers)
// Workgroups of a row-resident launch over `work` tiles (or pixels): min(work, 256), or min(work, cap) under the test hook
// lavie_debug_rowfuse_grid.  The kernels read gridDim.x and nothing else about the grid, so a cap of 3 walks a 50-tile input through
// the passes a 256-workgroup launch reaches only past 2048 tiles.  rowfuse_set_grid_cap: 0 = automatic, 1..256; else an error, unchanged.
int rowfuse_grid(int work);
int rowfuse_set_grid_cap(int max_workgroups);
bool geglu_mlp_supported(int C);
size_t geglu_mlp_image_bytes(int C);
size_t geglu_mlp_bias_floats(int C);
int pack_geglu_mlp(const half_t* w1, const half_t* b1, const half_t* w2, int C, half_t* img, float* b1img, hipStream_t stream);
// y = x + W2 (h * gelu(g)) + b2, (h, g) = W1 LN(x) + b1; y may alias x
// stats_out (optional, [M, 2]): (mean, rstd) of every output row for a LayerNorm-folded GEMM that consumes y (eps as the input norm's)
int launch_geglu_mlp(const half_t* x, half_t* y, int M, int C, const half_t* img, const float* b1img, const float* gamma,
                     const float* beta, const float* b2, float eps, hipStream_t stream, float* stats_out = nullptr);

// x' = x + to_out(attn_temp(LN(x))) for clips of exactly 16 frames, rows in (b f) d order; y may alias x
bool temporal_block_supported(int C, int heads, int F, int rot_dim);
size_t temporal_block_image_bytes(int C);
int pack_temporal_block(const half_t* wq, const half_t* wk, const half_t* wv, const half_t* wo, int C, half_t* img, hipStream_t stream);
int launch_temporal_block(const half_t* x, half_t* y, int B, int F, int D, int C, int heads, const half_t* img,
                          const float* gamma, const float* beta, const float* bo, const float* relbias, const float* rot_cos,
                          const float* rot_sin, int rot_dim, float scale, float eps, hipStream_t stream);

// ---- rowfuse_pin.hip: tx = proj_in(GroupNorm(x)), qkv = [to_q | to_k | to_v](LayerNorm(tx)) in one kernel (C = 320); GroupNorm comes in
// as the (a, b) pairs of launch_group_norm(..., ab_out), one set per `rows_per_domain` rows (a frame)
bool proj_qkv_supported(int C);
size_t proj_qkv_image_bytes(int C);
int pack_proj_qkv(const half_t* wpin, const half_t* wqkv, int C, half_t* img, hipStream_t stream);
int launch_proj_qkv(const half_t* x, const float* gn_ab, int rows_per_domain, const half_t* img, const float* bpin, const float* ln_g,
                    const float* ln_b, float eps, half_t* tx, half_t* qkv, int M, int C, hipStream_t stream);

// ---- rowfuse_cross.hip: x'' = x' + to_out2(attn2(LN2(x'), K, V)), x' = x + to_out1(att), K / V of the text context streamed
// with the weights (one image per video: pack once per model, bind once per context); y may alias x
// Two variants with images of their own layout, told apart by the 16-key tiles per head: short = 5 (1..80 keys), long = 10 (81..160)
enum CrossVariant { CROSS_NONE = -1, CROSS_SHORT = 0, CROSS_LONG = 1 };
constexpr int kCrossVariants = 2;
CrossVariant cross_block_variant(int C, int heads, int ctx_len, int rows_per_batch);     // the variant that serves the shape, or none
size_t cross_block_image_bytes(CrossVariant v);
int pack_cross_block(CrossVariant v, const half_t* wo1, const half_t* wq2, const half_t* wo2, int C, half_t* tmpl, hipStream_t stream);
int bind_cross_block(CrossVariant v, const half_t* tmpl, const half_t* kv, int B, int L, int C, half_t* img, hipStream_t stream);
int launch_cross_block(CrossVariant v, const half_t* att, const half_t* x, half_t* y, int M, int rows_per_batch, int C, int heads,
                       const half_t* img, const float* bo1, const float* gamma, const float* beta, const float* bo2, int L, float scale,
                       float eps, hipStream_t stream);

// ---- lora.hip: out[n, k] = fp16_rne(W0[n, k] + scale * sum_{j < r} B[n, j] A[j, k]), W0 / out fp16 [N, K], A fp32 [r, K], B fp32 [N, r];
// fp32 accumulation in ascending j, no atomics (deterministic); K % 8 == 0, W0 / out / A 16-byte aligned; out may alias W0
constexpr int kLoraMaxRank = 128;
int launch_lora_merge(const half_t* W0, const float* A, const float* B, half_t* out, int N, int K, int r, float scale,
                      hipStream_t stream);
// Several adapters in one pass: t = float(W0); t = fmaf(scale_i, (B_i A_i)[n, k], t) for the terms in list order, each B_i A_i by the
// chain above; out = fp16_rne(t), a conversion of the finished fp32 sum.  A term with scale 0 is skipped; with none left out = W0, with
// one left the call IS launch_lora_merge.  W0 read and out written once per element whatever n_terms is; same constraints per term;
// out may alias W0
constexpr int kLoraMaxTerms = 8;
struct LoraTerm {
    const float* A;     // [r, K]
    const float* B;     // [N, r]
    int r;
    float scale;
};
int launch_lora_merge_multi(const half_t* W0, const LoraTerm* terms, int n_terms, half_t* out, int N, int K, hipStream_t stream);

// ---- freeu.hip: FreeU on the two operands of a decoder concat (diffusers apply_freeu / fourier_filter): h_out = h with channels
// [0, C_h / 2) scaled by b; skip_out = skip with the modes ky in {0, -1} x kx in {0, -1} of every image's 2-D spectrum scaled by s
// (per image and channel: out = in + (s - 1) / (H W) sum_k [cos phi_k A_k + sin phi_k B_k] from seven fp32 mode sums).  h [(n y x), C_h],
// skip [(n y x), C2] fp16, C_h % 16 == 0, C2 % 8 == 0, 16-byte aligned; h_out / skip_out may alias their inputs (in place: the upper half
// of h is not touched).  s == 1 / b == 1: that tensor keeps its bits (copied when out of place), no sums run.  workspace:
// freeu_workspace_floats() floats (unused when s == 1).  At most two launches: the sums (a workgroup walks slabs_per_run slabs of
// kFreeuSlab pixels of 64 channels of one image; `runs` partials per image, folded in ascending order by the apply kernel) and the apply.
constexpr int kFreeuSlab = 32, kFreeuMaxRuns = 8, kFreeuMinRunSlabs = 4, kFreeuSums = 7;
struct FreeuGeom { int P, nslabs, slabs_per_run, runs; };
FreeuGeom freeu_geom(int H, int W);                 // from the image size alone: an image's sums do not depend on the batch around it
size_t freeu_workspace_floats(int C2, int NI, int H, int W);
int launch_freeu(const half_t* h, int C_h, const half_t* skip, int C2, int NI, int H, int W, float b, float s, half_t* h_out,
                 half_t* skip_out, float* workspace, hipStream_t stream);

// ---- freq_mix.hip: FreeInit's frequency mix on `images` fp32 volumes [F, H, W]:
//   out = r z + Re IFFT3(filter .* FFT3(a x0 + s e0 - r z)), filter real [F, H, W] in FFT-native order and even in frequency (the host
//   takes the even part), shared by all images; model_in (may be nullptr) receives fp16(out in_scale), rounded once, in `dup` copies
//   `dup_stride` elements apart.  A separable direct fp32 DFT in six launches, twiddles from fp64 host tables; out may alias x0.
//   workspace: freq_mix_workspace_floats() floats, 8-byte aligned.  Fixed summation order, no atomics: bit-reproducible, and an image
//   has the bits of its single-image call.
constexpr int kFreqMixMaxF = 256, kFreqMixMaxHW = 128, kFreqMixMaxImages = 65535;
struct FreqMixParams {
    const float *x0, *e0, *z, *filter;
    float a, s, r;
    float* out;
    half_t* model_in;
    int dup;
    int64_t dup_stride;
    float in_scale;
    float* workspace;
    int images, F, H, W;
};
bool freq_mix_supported(int images, int F, int H, int W);
size_t freq_mix_workspace_floats(int images, int F, int H, int W);      // 0 for an unsupported shape
int launch_freq_mix(const FreqMixParams& p, hipStream_t stream);

// ---- text_encoder.hip: what a CLIP text transformer needs beyond LayerNorm and Linear
// Causal self-attention over packed rows qkv [NB L, ld] (q | k | v, heads side by side, each heads * dh wide): row b L + i attends to
// rows b L + j, j <= i; o [NB L, ldo].  1 <= L <= kCausalMaxL, dh 32 or 64, ld and ldo multiples of 8, both tensors 16-byte aligned.
// One workgroup per (batch entry, head), K and V in LDS, one pass; an entry has the bits of its single-entry call.
constexpr int kCausalMaxL = 128;
int launch_causal_attention(const half_t* qkv, int ld, half_t* o, int ldo, int NB, int L, int heads, int dh, float scale, hipStream_t stream);
// out [B L, C] = fp16(float(tok[ids[r]]) + float(pos[r % L])), one rounding; ids int32 [B L] on the device, clamped into [0, V) by the
// kernel (a caller that can see the ids validates them first); tok [V, C], pos [>= L, C]; C % 8 == 0, tables and out 16-byte aligned
int launch_token_embed(const int* ids, const half_t* tok, const half_t* pos, half_t* out, int B, int L, int C, int V, hipStream_t stream);
// x[0, n) <- act(x) in place, fp32 arithmetic, one rounding: kind 0 = x sigmoid(1.702 x) (CLIP's quick_gelu), 1 = erf-GELU (gelu_erf_f)
int launch_act(half_t* x, int64_t n, int kind, hipStream_t stream);

// ---- image_encoder.hip: what the CLIP vision tower and the image mapper need beyond the text encoder's operators
// Bidirectional attention over short sequences: o [NB Lq, ldo] = softmax_j(scale q_i k_j) v_j, j < Lk; q [NB Lq, ldq], k [NB Lk, ldk],
// v [NB Lk, ldv], heads side by side in the first heads * dh columns of each.  1 <= Lq, Lk <= kShortMaxL, dh 32 or 64, pitches multiples
// of 8, 16-byte aligned tensors.  kv_shared: every entry reads the keys and values of entry 0 (k, v hold one entry).  K and V of a head
// in LDS, one pass; an entry has the bits of its single-entry call.
constexpr int kShortMaxL = 320;
int launch_short_attention(const half_t* q, int ldq, const half_t* k, int ldk, const half_t* v, int ldv, half_t* o, int ldo, int NB, int Lq,
                           int Lk, int heads, int dh, float scale, bool kv_shared, hipStream_t stream);
// CLIPVisionEmbeddings.  px [B, 3, S, S] NCHW (fp16 or fp32), S = G P; out [B, 1 + G^2, C]: row 0 = fp16(cls + pos[0]), row 1 + g =
// patch g (row-major over the grid) through the bias-free P x P stride-P conv + pos[1 + g], fp32 sum, one rounding.  wp: the conv
// weight [C, 3 P^2] zero-padded to patch_embed_k(P) columns (launch_pack_patch_embed); cols: patch_embed_workspace_bytes(B, S, P) of
// workspace (the gathered patches).  C a multiple of 128 up to 2048.  One gather launch + one pinned GEMM per image.
int patch_embed_k(int P);
long long patch_embed_workspace_bytes(int B, int S, int P);      // -1 for a geometry that is refused
int launch_pack_patch_embed(const half_t* w, half_t* out, int C, int P, hipStream_t stream);
int launch_patch_embed(const void* px, bool px_f32, const half_t* wp, const half_t* cls, const half_t* pos, half_t* out, half_t* cols, int B,
                       int S, int P, int C, hipStream_t stream);
// out [B L, C] = fp16(float(x[r]) + float(pos[r % L])), one rounding; C % 8 == 0, 16-byte aligned tensors
int launch_add_rows(const half_t* x, const half_t* pos, half_t* out, int B, int L, int C, hipStream_t stream);
// x[0, n) <- max(x, 0) in place, exact: a negative value becomes +0, everything else keeps its bits (torch.relu)
int launch_relu(half_t* x, int64_t n, hipStream_t stream);

// host-only helper (no GPU): T5-style bucket of (query i, key j), attention.py:681-699
void relpos_bucket_table(int F, int num_buckets, int max_distance, int* out);

}  // namespace lavie
