// Host-side denoiser: owns packed weights + workspace and enqueues one UNet forward on a stream.
#pragma once
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lavie_hip.h"
#include "common.h"
#include "ops.h"
#include "weight_parts.h"

namespace lavie {

// Bump allocator over hipMalloc'd chunks (weights) or one fixed block (workspace).
class DeviceArena {
public:
    ~DeviceArena();
    int init_fixed(size_t bytes);                 // one block, alloc() fails when exhausted
    void init_virtual() { virtual_ = true; }      // no memory: only tracks the high-water mark
    void* alloc(size_t bytes);                    // 256-B aligned; nullptr on failure
    size_t mark() const { return off_; }
    void release(size_t mark) { off_ = mark; }
    size_t peak() const { return peak_; }
    size_t total_bytes() const { return total_; }
    void free_all();

private:
    std::vector<void*> chunks_;
    char* cur_ = nullptr;
    size_t cap_ = 0, off_ = 0, peak_ = 0, total_ = 0;
    bool fixed_ = false, virtual_ = false;
    static constexpr size_t kChunk = 512ull << 20;
};

struct NormW { float* g = nullptr; float* b = nullptr; int C = 0; };
struct LinW { half_t* w = nullptr; float* b = nullptr; int N = 0, K = 0; };

struct ResnetW {
    std::string prefix;
    int cin = 0, cout = 0;
    bool shortcut = false;
    NormW n1, n2;
    half_t* w1 = nullptr; float* b1 = nullptr;      // [cout][9*cin]
    half_t* w2 = nullptr; float* b2 = nullptr;      // [cout][9*cout (+ cin)] ; b2 = conv2.bias (+ shortcut.bias)
    int ldw2 = 0;
    int temb_off = 0;                               // column of this block inside the fused time_emb_proj output
    float eps = 0.f;                                // GroupNorm eps; 0 = the model's norm_eps
};

// ResnetBlock3DCNN (vsr/models/resnet.py:220-315): GroupNorm + SiLU -> (T,1,1) conv -> GroupNorm + SiLU -> (3,1,1) conv
struct TemporalResW {
    bool present = false;
    int taps1 = 3;
    NormW n1, n2;
    half_t* w1 = nullptr; float* b1 = nullptr;      // [C][taps1 * C]
    half_t* w2 = nullptr; float* b2 = nullptr;      // [C][3 * C]
};

// A projection that consumes a LayerNorm of the block's residual stream, in both forms: plain (w, b) behind an explicit LayerNorm,
// and with the norm folded in: W' = W * gamma (fp16), s = row sums of W', b' = W beta (+ bias)
struct TransformerW;
struct LnProj {
    NormW TransformerW::* ln;                       // the norm it sits behind
    int N = 0;                                      // output columns ([N][C] weights)
    half_t* w = nullptr; float* b = nullptr;
    half_t* fw = nullptr; float* fs = nullptr; float* fb = nullptr;
};

struct TransformerW {
    std::string prefix;
    int C = 0;
    // VSR variant (lavie_unet_config::vsr_blocks / only_cross_attention)
    TemporalResW tres;                              // `resblock_temporal`, runs before the block's residual is taken
    bool attn1_cross = false;                       // attn1 attends to the text context: qkv1 is to_q alone, wkv1 [2C][cross_dim]
    half_t* wkv1 = nullptr;
    NormW gn, ln1, ln2, lnt, ln3;
    LinW pin, pout;
    LnProj qkv1{&TransformerW::ln1}; LinW o1;       // to_q | to_k | to_v rows
    LnProj q2{&TransformerW::ln2}; half_t* wkv2 = nullptr; LinW o2;
    LnProj qkvt{&TransformerW::lnt}; LinW ot;
    half_t* relemb = nullptr;                       // [buckets][heads] fp16 (state-dict tensor)
    LnProj ff1{&TransformerW::ln3}; LinW ff2;       // ff1 in GEGLU-interleaved row order
    // row-resident fused sub-blocks (rowfuse.hip), built where the width has a kernel (level 0: C = 320)
    half_t* ff_img = nullptr; float* ff_b1img = nullptr;    // norm3 -> GEGLU feed-forward -> + residual in one kernel
    half_t* tb_img = nullptr;                               // norm_temp -> q|k|v -> temporal attention -> to_out -> + residual
    // attn1.to_out -> norm2 -> attn2 -> + residual: weight part of the image (rowfuse_cross.hip), per variant; the long one (81..160
    // keys) is built by the first long cache_context
    half_t* xb_tmpl[kCrossVariants] = {nullptr, nullptr};
    half_t* pq_img = nullptr;                               // GroupNorm -> proj_in -> norm1 -> q|k|v (rowfuse_pin.hip, round 4)
};

struct SamplerW { half_t* w = nullptr; float* b = nullptr; int C = 0;
                  half_t* wpar = nullptr; };    // upsamplers: the four parity weight sets [4][C][4 C] (igemm_patch.hip MODE 3)

// TemporalModule3D (vsr/models/temporal_module.py:65-178): ResnetBlock3DCNN (5,1,1) -> ResnetBlock3D -> 1x1 shift conv
struct TemporalModuleW {
    std::string prefix;
    int C = 0;
    TemporalResW t;
    int t_temb_off = 0;                             // column of resblocks_3d_t.time_emb_proj inside the fused projection
    ResnetW s;
    LinW shift;
};

struct Route;    // the switches that decide which kernels a call runs, as one value (engine.cpp)
struct FwdCtx;   // per-call state (engine.cpp): stream, workspace, shape, the call's Route, its frame tables, the state of the text cache

// An activation of the forward: [rows, C] fp16 and the GroupNorm statistics its producer left.  Every tensor a GroupNorm may read
// has a small buffer next to it (same workspace lifetime); the GEMM that writes the tensor fills the buffer and describes it in `cs`,
// and the description travels with the tensor, never keyed by address (workspace addresses are reused).  An input is a const Act&
// (a second, optional one a const Act*); an output is an Act* whose p and csbuf the caller has set and whose cs the producer
// fills; a step that works in place takes an Act&.
struct Act {
    half_t* p = nullptr;
    int C = 0;
    GnColStat cs;                                   // empty: the producer left none, a GroupNorm runs its statistics pass
    float* csbuf = nullptr;                         // where a producer of p leaves them; nullptr: it is asked for none
};

// per-F tables, built once per clip length and kept (the VSR chunk driver alternates F = 8 and F = 5)
struct FrameTables {
    float* rot_cos = nullptr; float* rot_sin = nullptr;
    std::vector<float*> relbias;                    // one [heads, F, F] per transformer
};

// One registered low-rank adapter target (lavie_unet_lora_*): the projection's rows inside the packed weights and what they are
// rebuilt from: one base copy, and per registry slot the adapter that slot holds on this target.  Every buffer is the engine's own:
// the caller's tensors are copied at registration.
struct LoraSlot {
    float* A = nullptr;                             // [r][K] fp32
    float* B = nullptr;                             // [N][r] fp32
    int r = 0;                                      // 0: the slot has no entry here
    float scale = 1.f;                              // per-target scale (alpha / r); the factor is (global * slot weight) * this
};
struct LoraEntry {
    int ti = -1;                                    // transformer block
    half_t* dst = nullptr;                          // the projection's [N][K] rows inside qkv1 / wkv1 / o1 / q2 / wkv2 / o2 / qkvt / ot
    int N = 0, K = 0;
    half_t* base = nullptr;                         // copy of the base weight
    LoraSlot slot[kLoraMaxTerms];
    bool empty() const {                            // no slot left: the next apply writes the base back and drops the entry
        for (const LoraSlot& s : slot) if (s.r) return false;
        return true;
    }
};

class UNet {
public:
    explicit UNet(const lavie_unet_config& cfg);
    ~UNet();
    int validate_config();
    const std::vector<ParamTable::Param>& params() const { return table_.params(); }
    int set_param(const char* name, const void* data, long long numel) { return table_.set("set_param", "", name, data, numel); }
    int finalize(hipStream_t stream);
    int prepare(int B, int F, int H, int W, int ctx_len);
    // layer_cache: LAVIE_LAYER_CACHE_OFF (the plain forward), _REFRESH (the full walk, filling the layer cache) or _REUSE (the
    // shallow walk on the cached activation); see set_layer_cache
    int forward(const half_t* sample, const float* timesteps, const half_t* ctx, half_t* out, int B, int F, int H, int W,
                int ctx_len, hipStream_t stream, const int* class_labels_host, int layer_cache = 0);
    int resnet_forward(const char* prefix, const half_t* x1, int C1, const half_t* x2, int C2, const float* temb, half_t* y,
                       int B, int F, int H, int W, hipStream_t stream);
    int transformer_forward(const char* prefix, half_t* x, const half_t* ctx, int B, int F, int H, int W, int ctx_len,
                            hipStream_t stream);
    // Text K/V of every transformer block for one context tensor, computed once and reused by every forward that is called
    // with the SAME ctx pointer and shape (the denoise loop passes one context for all of its steps); ctx == nullptr clears.
    int cache_context(const half_t* ctx, int B, int ctx_len, hipStream_t stream);
    // forward() replayed from a hipGraph: the first call with a new (pointers, shape) tuple runs eagerly (tables, kernel
    // attributes), the second captures the enqueue of one forward on `stream` and launches the instantiated graph, later
    // calls with the same tuple replay it.  Tensor CONTENTS may change between calls, addresses may not.  Falls back to the
    // eager forward while kernel profiling is active (events cannot be recorded into a capture).
    int forward_graph(const half_t* sample, const float* timesteps, const half_t* ctx, half_t* out, int B, int F, int H, int W,
                      int ctx_len, hipStream_t stream);
    long long weight_bytes() const { return (long long)weights_.total_bytes(); }
    long long workspace_bytes() const { return (long long)ws_.total_bytes(); }
    void set_ln_fold(bool on) { ln_fold_ = on; ++graph_gen_; }
    void set_cfg_shared_input(bool on) { cfg_shared_input_ = on; ++graph_gen_; }
    // FreeU (freeu.hip) in front of every resnet of up blocks 0 and 1: stage i scales the first half of the running activation's
    // channels by b[i] and the skip's lowest modes by s[i]; (1, 1) = the stage launches nothing.  Values must be finite and > 0.
    int set_freeu(float s1, float s2, float b1, float b2);
    // Perturbed-attention guidance (Ahn et al.; diffusers' PAG pipelines): in the transformers whose prefix starts with an entry of
    // `layers` (followed by '.' or the end), attn1 of the last `perturbed` batch entries is the identity map on values,
    // to_out(to_v(norm1(x))): the softmax runs on the leading entries only and the V columns are copied for the rest.  n_layers == 0
    // or perturbed == 0: off.  Refused, nothing changed: an entry that selects nothing, a selected block whose attn1 is not the plain
    // spatial self-attention, perturbed < 0.  While on, set_cfg_shared_input is ignored (the perturbed entries differ from the first
    // self-attention on) and a forward needs B > perturbed.
    int set_pag(const char* const* layers, int n_layers, int perturbed);
    // Layer cache (DeepCache): depth d in 1..layers_per_block puts cut A behind layer d - 1 of down level 0 and cut B in
    // front of layer layers_per_block - d of the last up block; a refresh forward keeps the running activation at B, a reuse forward
    // runs only the steps in front of A and behind B on it.  0 = off, the cache is freed.  Any call marks a held cache invalid.
    int set_layer_cache(int depth);
    long long layer_cache_bytes() const { return (long long)lc_bytes_; }
    // Low-rank adapters on the attention projections (to_q / to_k / to_v / to_out.0 of attn1 / attn2 / attn_temp).  set / clear /
    // set_scale only record (the set copies the caller's tensors on `stream`); apply merges every target of the blocks touched since
    // the last apply and re-derives those blocks' images in place: device addresses never change, captured graphs stay valid.
    int lora_set(const char* name, const half_t* base, const float* A, const float* B, int r, float scale, hipStream_t stream);
    int lora_clear(const char* name, hipStream_t stream);
    int lora_set_scale(float scale);
    // The same per registry slot (set / clear above are slot 0) and the slot's blend weight: apply serves, per target, the slots that
    // hold an entry for it in ascending order in one merge, W0 + sum (global * weight_slot * scale) B A
    int lora_set_slot(int slot, const char* name, const half_t* base, const float* A, const float* B, int r, float scale,
                      hipStream_t stream);
    int lora_clear_slot(int slot, const char* name, hipStream_t stream);
    int lora_set_slot_weight(int slot, float weight);
    int lora_apply(hipStream_t stream);

private:
    void build_param_list();
    int pack_model(hipStream_t s);                  // finalize's body: everything it allocates and enqueues
    // a listed tensor into a fresh piece of the weight arena: n floats converted from fp16 / n halves copied
    int pack_f32(const std::string& key, size_t n, float** out, hipStream_t s);
    int pack_copy(const std::string& key, size_t n, half_t** out, hipStream_t s);
    int pack_norm(const std::string& prefix, int C, NormW* out, hipStream_t s);
    int pack_linear(const std::string& prefix, int N, int K, bool bias, LinW* out, hipStream_t s);
    int pack_resnet(ResnetW* r, hipStream_t s);
    int pack_transformer(TransformerW* t, hipStream_t s);
    int derive_transformer(const TransformerW& t, hipStream_t s);
    int lora_target(const char* name, int* ti, int* attn, int* proj) const;
    void lora_free(LoraSlot& s);
    int pack_temporal_res(const std::string& prefix, int C, int taps1, TemporalResW* out, hipStream_t s);
    int run_temporal_res(FwdCtx& c, const TemporalResW& r, const Act& x, Act* y, int D, const float* bias2, int ldb2);
    int run_temporal_module(FwdCtx& c, const TemporalModuleW& m, const Act& x, Act* y, const float* tproj, int ld_tproj, int H, int W);
    int pack_sampler(const std::string& prefix, int C, SamplerW* out, hipStream_t s, bool up = false);
    int ensure_tables(int F, hipStream_t s);
    // THE per-call state of a call that enters with this shape and context: every entry point builds it here (Route = the switches
    // in force, `pag` = pag_route() where the call runs attn1), and so do prepare()'s dry runs (`planned`: the Route it enumerates)
    FwdCtx call_ctx(hipStream_t s, DeviceArena* ws, int B, int F, int H, int W, const half_t* ctx, int ctx_len, int pag,
                    const Route* planned = nullptr) const;

    int run(FwdCtx& c, const half_t* sample, const float* timesteps, const half_t* ctx, half_t* out);
    // x2: the skip tensor concatenated behind x1, or nullptr.  norm1 takes the statistics x1 / x2 carry; conv2's epilogue leaves y's
    int run_resnet(FwdCtx& c, const ResnetW& r, const Act& x1, const Act* x2, const float* tproj, int ld_tproj, Act* y, int H, int W);
    // Sequences the launches of one block from its route (engine.cpp block_route(): decided once per call from c.route, the shape and
    // whether the text K / V are cached and bound).  In place on x: its statistics feed the block's per-frame GroupNorm and are
    // replaced by those of the block output (proj_out's epilogue).  shared_prefix: the part in front of the text cross-attention runs
    // on the first half of the batch
    int run_transformer(FwdCtx& c, const TransformerW& t, Act& x, const half_t* ctx, int H, int W, bool shared_prefix = false);
    int run_conv(FwdCtx& c, const Act& x, const SamplerW& w, Act* y, int Hi, int Wi, int stride, int ups);

    struct GraphKey {
        const void *sample = nullptr, *t = nullptr, *ctx = nullptr, *out = nullptr, *kv_ctx = nullptr;
        int B = 0, F = 0, H = 0, W = 0, L = 0;
        unsigned long gen = 0;          // bumped by everything that changes what a forward enqueues (workspace, caches, modes)
        unsigned long debug_epoch = 0;  // process-wide: bumped by every lavie_debug_* kernel-selection switch (api.cpp)
        hipStream_t stream = nullptr;
        bool operator==(const GraphKey& o) const {
            return sample == o.sample && t == o.t && ctx == o.ctx && out == o.out && kv_ctx == o.kv_ctx && B == o.B && F == o.F &&
                   H == o.H && W == o.W && L == o.L && gen == o.gen && debug_epoch == o.debug_epoch && stream == o.stream;
        }
    };
    void drop_graph();
    GraphKey graph_seen_, graph_key_;
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t graph_exec_ = nullptr;
    hipStream_t cap_stream_ = nullptr;              // capture only: nothing ever executes on it
    unsigned long graph_gen_ = 0;

    lavie_unet_config cfg_;
    ParamTable table_;                              // the state-dict tensors, lent by set_param until finalize has packed them
    bool finalized_ = false;
    // The two per-handle switches of a call's Route: read by call_ctx() and by prepare(), nowhere below.
    // the caller promises sample[b] == sample[b + B/2] (classifier-free guidance on duplicated latents): the layers in front of
    // the first text cross-attention are computed for the first half and copied
    bool cfg_shared_input_ = false;
    bool ln_fold_ = true;                           // LayerNorm folded into the producer / consumer GEMM epilogues
    float freeu_s_[2] = {1.f, 1.f}, freeu_b_[2] = {1.f, 1.f};      // set_freeu: read by run() in the up walk (decoder only)
    std::vector<char> pag_sel_;                     // set_pag: per transformer, attn1 perturbed; empty = off
    int pag_perturbed_ = 0;                         // trailing batch entries it applies to; read where a call enters, as the switches above
    int pag_route(const char* who, int B) const;    // the Route::pag of a call on B entries (0 = off), or -1 after refusing B <= perturbed
    // layer cache (set_layer_cache): ONE hipMalloc'd block outside the workspace, sized by prepare() for its shape: the activation at
    // cut B [rows(0), C] fp16 and its statistics buffer.  lc_act_ is the tensor as its producer in the last refresh forward left it;
    // lc_key_ = (B, F, H, W, ctx_len, depth) of that forward, all 0 = invalid
    int lc_depth_ = 0;
    void* lc_block_ = nullptr;
    size_t lc_bytes_ = 0;
    Act lc_act_;
    int lc_key_[6] = {0, 0, 0, 0, 0, 0};
    int lc_shape_[4] = {0, 0, 0, 0};                // B, F, H, W of the latest prepare()
    int lc_channels(int depth) const { return cfg_.block_out_channels[depth == cfg_.layers_per_block ? 1 : 0]; }
    int ensure_layer_cache();                       // (re)allocates the block for lc_shape_ and lc_depth_; invalidates on a change

    DeviceArena weights_, ws_;
    // packed model
    half_t* conv_in_w_ = nullptr; float* conv_in_b_ = nullptr;
    half_t* conv_out_w_ = nullptr; float* conv_out_b_ = nullptr;
    NormW norm_out_;
    LinW time1_, time2_, tproj_;                    // tproj_: all ResnetBlock3D.time_emb_proj stacked
    std::vector<ResnetW> resnets_;                  // execution order
    std::vector<TransformerW> transformers_;
    std::vector<SamplerW> downs_, ups_;
    std::vector<TemporalModuleW> tmods_;            // VSR: down 0..L-1, mid, up 0..L-1
    half_t* class_emb_ = nullptr;                   // [num_class_embeds][time_embed_dim] fp16 (state-dict tensor)
    half_t* zero_page_ = nullptr;
    std::unordered_map<int, FrameTables> tables_;   // by F (ensure_tables)
    // cached text K/V (cache_context): one [B * ctx_len, 2C] buffer per transformer (attn2; attn1 on VSR cross levels)
    std::vector<half_t*> kv2_cache_, kv1_cache_;
    size_t kv_cache_rows_ = 0;                      // rows the buffers were allocated for
    // fused text cross-attention: per transformer with a template image, [B] images = weights + this context's K / V
    std::vector<half_t*> xb_img_;
    int kv_cache_B_ = 0;                            // videos the image buffers were allocated for
    bool xb_bound_ = false;                         // images hold the cached context (its length fits the kernel)
    size_t xb_img_bytes_ = 0;                       // bytes per video the image buffers were laid out for (short or long layout)
    void* xbl_block_ = nullptr;                     // ONE hipMalloc'd block behind every long template, kept for the model's life
    int ensure_long_templates(hipStream_t stream);
    void* kv_block_ = nullptr;                      // ONE hipMalloc'd block behind every K/V cache buffer: freed and reallocated on growth
    const half_t* kv_ctx_ = nullptr;
    int kv_B_ = 0, kv_len_ = 0;
    // low-rank adapter registry (lora_*), ordered by name so apply enqueues the same sequence every time
    std::map<std::string, LoraEntry> lora_;
    float lora_scale_ = 1.f;                        // global adapter scale
    float lora_weight_[kLoraMaxTerms] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};    // per-slot blend weight
    std::vector<char> lora_dirty_;                  // per transformer: touched since the last apply
};

}  // namespace lavie
