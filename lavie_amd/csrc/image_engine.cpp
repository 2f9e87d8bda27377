// CLIPVisionTransformer (transformers modeling_clip.py) up to last_hidden_state and the fork's MappingNetwork
// (base/pipelines/mapping.py:61-97 of the reference: nn.TransformerDecoder, post-norm, ReLU) on the engine's operators.
// Vision, on rows x [B T, C]:   x = pre_layrnorm(embeddings(pixels)); per layer
//   h = LN1(x); qkv = h Wqkv^T + b; h = attention(q, k, v); x = h Wo^T + bo + x; h = LN2(x); m = act(h W1^T + b1); x = m W2^T + b2 + x
//   (post_layernorm belongs to the pooled output and is not applied to last_hidden_state)
// Mapper, on rows x [B So, C]:  mem = image Wimg^T + b + image_pos; x = text + text_pos; per layer
//   qkv = x Wsa^T + b; a = attention(q, k, v); t = a Wo^T + bo + x; x = norm1(t)
//   a = x Wq^T + bq; kv = mem Wkv^T + bkv; t = attention(a, k, v); a = t Wo'^T + bo' + x; x = norm2(a)
//   m = relu(x W1^T + b1); t = m W2^T + b2 + x; x = norm3(t)          (no final norm)
// Every tensor between two launches is fp16; a residual is added to the fp32 sum of its GEMM before the one rounding.  All GEMMs run
// the pinned plan (pinned_linear.h); every other launch works row by row or (entry, head) by (entry, head): an image's and a
// prompt's block has the same bits at every batch size and position.
#include "image_engine.h"

#include <math.h>

#include "ops.h"
#include "pinned_linear.h"

namespace lavie {

#define RUN(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

namespace {

constexpr size_t H = sizeof(half_t);

// hands out 256-byte pieces of a block; with base = nullptr it only counts
struct Carver {
    char* base;
    size_t used = 0;
    template <class T>
    T* take(size_t count) {
        T* r = base ? (T*)(base + used) : nullptr;
        used += up256(count * sizeof(T));
        return r;
    }
};

int copy16(half_t* dst, const half_t* src, size_t n, hipStream_t s) {
    LAVIE_HIP(hipMemcpyAsync(dst, src, n * H, hipMemcpyDeviceToDevice, s));
    return 0;
}

int check_batch(const char* who, int B) {
    LAVIE_CHECK(B >= 1 && B <= kImageMaxBatch, "%s: B=%d must be 1..%d", who, B, kImageMaxBatch);
    return 0;
}

}  // namespace

// ------------------------------------------------------------------ the parameter table
void ParamTable::add(const std::string& name, long long numel) {
    index_[name] = (int)params_.size();
    params_.push_back({name, numel, nullptr});
}

int ParamTable::set(const char* who, const char* prefix, const char* name, const void* data, long long numel) {
    std::string key = name;
    const std::string pre = prefix;
    if (!pre.empty() && key.compare(0, pre.size(), pre) != 0) key = pre + key;
    for (const std::string& ig : ignored_)
        if (key == ig) return 0;
    auto it = index_.find(key);
    LAVIE_CHECK(it != index_.end(), "%s: unknown state-dict key '%s'", who, name);
    Param& pi = params_[it->second];
    LAVIE_CHECK(pi.numel == numel, "%s: '%s' has %lld elements, expected %lld", who, name, numel, pi.numel);
    LAVIE_CHECK(data != nullptr, "%s: '%s' null data", who, name);
    pi.src = (const half_t*)data;
    return 0;
}

int ParamTable::all_set(const char* who) const {
    for (const Param& p : params_) LAVIE_CHECK(p.src != nullptr, "%s: '%s' was never set", who, p.name.c_str());
    return 0;
}

void ParamTable::release() {
    for (Param& p : params_) p.src = nullptr;      // the loan ends when the stream drains
}

// ------------------------------------------------------------------ the vision tower
static const char* kVis = "vision_model.";

VisionEncoder::VisionEncoder(const lavie_vision_config& cfg) : cfg_(cfg) {
    const long long C = cfg.hidden, I = cfg.intermediate;
    if (cfg.layers < 0 || cfg.layers > 1024 || cfg.patch_size < 1 || cfg.patch_size > 64 || cfg.image_size < 1 || cfg.image_size > 1024) return;
    const std::string v = kVis;
    table_.add(v + "embeddings.class_embedding", C);
    table_.add(v + "embeddings.patch_embedding.weight", C * 3 * cfg.patch_size * cfg.patch_size);
    table_.add(v + "embeddings.position_embedding.weight", (long long)tokens() * C);
    table_.add(v + "pre_layrnorm.weight", C);
    table_.add(v + "pre_layrnorm.bias", C);
    for (int i = 0; i < cfg.layers; ++i) {
        const std::string p = v + "encoder.layers." + std::to_string(i) + ".";
        for (const char* proj : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
            table_.add(p + "self_attn." + proj + ".weight", C * C);
            table_.add(p + "self_attn." + proj + ".bias", C);
        }
        table_.add(p + "layer_norm1.weight", C);
        table_.add(p + "layer_norm1.bias", C);
        table_.add(p + "mlp.fc1.weight", I * C);
        table_.add(p + "mlp.fc1.bias", I);
        table_.add(p + "mlp.fc2.weight", C * I);
        table_.add(p + "mlp.fc2.bias", C);
        table_.add(p + "layer_norm2.weight", C);
        table_.add(p + "layer_norm2.bias", C);
    }
    table_.ignore(v + "post_layernorm.weight");      // the pooled output's norm: not part of last_hidden_state
    table_.ignore(v + "post_layernorm.bias");
}

VisionEncoder::~VisionEncoder() {
    if (block_) (void)hipFree(block_);
}

int VisionEncoder::validate_config() const {
    const lavie_vision_config& c = cfg_;
    LAVIE_CHECK(c.hidden >= kPinBn && c.hidden % kPinBn == 0 && c.hidden <= 2048, "vision_create: hidden=%d must be a multiple of %d up to 2048",
                c.hidden, kPinBn);
    LAVIE_CHECK(c.intermediate >= kPinBn && c.intermediate % kPinBn == 0 && c.intermediate <= 16384,
                "vision_create: intermediate=%d must be a multiple of %d up to 16384", c.intermediate, kPinBn);
    LAVIE_CHECK(c.layers >= 1 && c.layers <= 64, "vision_create: layers=%d must be 1..64", c.layers);
    LAVIE_CHECK(c.heads >= 1 && c.hidden % c.heads == 0 && (c.hidden / c.heads == 32 || c.hidden / c.heads == 64),
                "vision_create: heads=%d gives a head dim of hidden / heads that is not 32 or 64 (hidden=%d)", c.heads, c.hidden);
    LAVIE_CHECK(c.patch_size >= 1 && c.patch_size <= 64, "vision_create: patch_size=%d must be 1..64", c.patch_size);
    LAVIE_CHECK(c.image_size >= c.patch_size && c.image_size <= 1024 && c.image_size % c.patch_size == 0,
                "vision_create: image_size=%d must be a multiple of patch_size=%d up to 1024", c.image_size, c.patch_size);
    LAVIE_CHECK(tokens() <= kShortMaxL, "vision_create: image_size=%d / patch_size=%d gives %d tokens, more than %d", c.image_size, c.patch_size,
                tokens(), kShortMaxL);
    LAVIE_CHECK(c.act == LAVIE_TEXT_ACT_QUICK_GELU || c.act == LAVIE_TEXT_ACT_GELU, "vision_create: act=%d is neither quick_gelu (0) nor gelu (1)",
                c.act);
    LAVIE_CHECK(isfinite(c.eps) && c.eps > 0.f, "vision_create: eps must be finite and > 0");
    return 0;
}

int VisionEncoder::set_param(const char* name, const void* data, long long numel) {
    LAVIE_CHECK(!finalized_, "vision_set_param: the handle is finalized");
    return table_.set("vision_set_param", kVis, name, data, numel);
}

int VisionEncoder::finalize(hipStream_t s) {
    LAVIE_CHECK(!finalized_, "vision_finalize: the handle is finalized already");
    RUN(table_.all_set("vision_finalize"));
    const size_t C = cfg_.hidden, I = cfg_.intermediate, T = tokens(), P = cfg_.patch_size, Kp = patch_embed_k(cfg_.patch_size);
    const long long ws = workspace_bytes(kImageMaxBatch);
    if (ws < 0) return -1;
    layers_.resize(cfg_.layers);
    auto carve = [&](char* base) {
        Carver c{base};
        wpatch_ = c.take<half_t>(C * Kp);
        cls_ = c.take<half_t>(C);
        pos_ = c.take<half_t>(T * C);
        preg_ = c.take<float>(C);
        preb_ = c.take<float>(C);
        for (Layer& l : layers_) {
            l.wqkv = c.take<half_t>(3 * C * C);
            l.wo = c.take<half_t>(C * C);
            l.w1 = c.take<half_t>(I * C);
            l.w2 = c.take<half_t>(C * I);
            l.bqkv = c.take<float>(3 * C);
            l.bo = c.take<float>(C);
            l.b1 = c.take<float>(I);
            l.b2 = c.take<float>(C);
            l.ln1g = c.take<float>(C);
            l.ln1b = c.take<float>(C);
            l.ln2g = c.take<float>(C);
            l.ln2b = c.take<float>(C);
        }
        return c.used;
    };
    const size_t weights = carve(nullptr);
    if (block_) { (void)hipFree(block_); block_ = nullptr; }      // a finalize that failed half way
    LAVIE_HIP(hipMalloc((void**)&block_, weights + (size_t)ws));
    carve(block_);
    ws_ = block_ + weights;
    const std::string v = kVis;
    auto src = [&](const std::string& n) { return table_.src(v + n); };
    auto to32 = [&](float* dst, const std::string& n, size_t count) { return launch_f16_to_f32(src(n), dst, (int64_t)count, s); };
    RUN(launch_pack_patch_embed(src("embeddings.patch_embedding.weight"), wpatch_, (int)C, (int)P, s));
    RUN(copy16(cls_, src("embeddings.class_embedding"), C, s));
    RUN(copy16(pos_, src("embeddings.position_embedding.weight"), T * C, s));
    RUN(to32(preg_, "pre_layrnorm.weight", C));
    RUN(to32(preb_, "pre_layrnorm.bias", C));
    for (int i = 0; i < cfg_.layers; ++i) {
        Layer& l = layers_[i];
        const std::string p = "encoder.layers." + std::to_string(i) + ".";
        const char* qkv[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            RUN(copy16(l.wqkv + j * C * C, src(p + "self_attn." + qkv[j] + ".weight"), C * C, s));
            RUN(to32(l.bqkv + j * C, p + "self_attn." + qkv[j] + ".bias", C));
        }
        RUN(copy16(l.wo, src(p + "self_attn.out_proj.weight"), C * C, s));
        RUN(to32(l.bo, p + "self_attn.out_proj.bias", C));
        RUN(copy16(l.w1, src(p + "mlp.fc1.weight"), I * C, s));
        RUN(to32(l.b1, p + "mlp.fc1.bias", I));
        RUN(copy16(l.w2, src(p + "mlp.fc2.weight"), C * I, s));
        RUN(to32(l.b2, p + "mlp.fc2.bias", C));
        RUN(to32(l.ln1g, p + "layer_norm1.weight", C));
        RUN(to32(l.ln1b, p + "layer_norm1.bias", C));
        RUN(to32(l.ln2g, p + "layer_norm2.weight", C));
        RUN(to32(l.ln2b, p + "layer_norm2.bias", C));
    }
    table_.release();
    finalized_ = true;
    return 0;
}

// x [M, C] | h [M, C] | wide [M, max(3 C, I)] | the gathered patches
long long VisionEncoder::workspace_bytes(int B) const {
    if (check_batch("vision_workspace_bytes", B)) return -1;
    const size_t M = (size_t)B * tokens(), C = cfg_.hidden, I = cfg_.intermediate, wide = 3 * C > I ? 3 * C : I;
    return (long long)(2 * up256(M * C * H) + up256(M * wide * H)) + patch_embed_workspace_bytes(B, cfg_.image_size, cfg_.patch_size);
}

int VisionEncoder::encode(const void* px, int x_dtype, int B, void* out, hipStream_t s) {
    LAVIE_CHECK(finalized_, "vision_encode: the handle is not finalized");
    LAVIE_CHECK(px != nullptr, "vision_encode: pixel_values is null");
    LAVIE_CHECK(out != nullptr, "vision_encode: out_f16 is null");
    LAVIE_CHECK(x_dtype == 0 || x_dtype == 1, "vision_encode: x_dtype=%d (0 = fp16, 1 = fp32)", x_dtype);
    RUN(check_batch("vision_encode", B));
    const int T = tokens(), M = B * T, C = cfg_.hidden, I = cfg_.intermediate, heads = cfg_.heads, dh = C / heads;
    const size_t mc = up256((size_t)M * C * H), wide_c = 3 * C > I ? 3 * C : I;
    half_t* x = (half_t*)ws_;
    half_t* h = (half_t*)(ws_ + mc);
    half_t* wide = (half_t*)(ws_ + 2 * mc);
    half_t* cols = (half_t*)(ws_ + 2 * mc + up256((size_t)M * wide_c * H));
    const float scale = 1.0f / sqrtf((float)dh);
    RUN(launch_patch_embed(px, x_dtype == 1, wpatch_, cls_, pos_, h, cols, B, cfg_.image_size, cfg_.patch_size, C, s));
    RUN(launch_layernorm(h, preg_, preb_, x, M, C, cfg_.eps, s));
    for (size_t i = 0; i < layers_.size(); ++i) {
        const Layer& l = layers_[i];
        half_t* last = i + 1 == layers_.size() ? (half_t*)out : x;      // the last residual sum is last_hidden_state
        RUN(launch_layernorm(x, l.ln1g, l.ln1b, h, M, C, cfg_.eps, s));
        RUN(pinned_linear(h, l.wqkv, l.bqkv, nullptr, wide, M, 3 * C, C, s));
        RUN(launch_short_attention(wide, 3 * C, wide + C, 3 * C, wide + 2 * C, 3 * C, h, C, B, T, T, heads, dh, scale, false, s));
        RUN(pinned_linear(h, l.wo, l.bo, x, x, M, C, C, s));
        RUN(launch_layernorm(x, l.ln2g, l.ln2b, h, M, C, cfg_.eps, s));
        RUN(pinned_linear(h, l.w1, l.b1, nullptr, wide, M, I, C, s));
        RUN(launch_act(wide, (int64_t)M * I, cfg_.act, s));
        RUN(pinned_linear(wide, l.w2, l.b2, x, last, M, C, I, s));
    }
    return 0;
}

// ------------------------------------------------------------------ the mapper
ImageMapper::ImageMapper(const lavie_mapper_config& cfg) : cfg_(cfg) {
    const long long C = cfg.output_dim, D = cfg.input_dim, FF = cfg.dim_feedforward;
    if (cfg.layers < 0 || cfg.layers > 1024) return;
    table_.add("image_pos_embedding", (long long)cfg.seq_in * C);
    table_.add("text_pos_embedding", (long long)cfg.seq_out * C);
    table_.add("image_proj.weight", C * D);
    table_.add("image_proj.bias", C);
    for (int i = 0; i < cfg.layers; ++i) {
        const std::string p = "transformer_decoder.layers." + std::to_string(i) + ".";
        for (const char* att : {"self_attn", "multihead_attn"}) {
            table_.add(p + att + ".in_proj_weight", 3 * C * C);
            table_.add(p + att + ".in_proj_bias", 3 * C);
            table_.add(p + att + ".out_proj.weight", C * C);
            table_.add(p + att + ".out_proj.bias", C);
        }
        table_.add(p + "linear1.weight", FF * C);
        table_.add(p + "linear1.bias", FF);
        table_.add(p + "linear2.weight", C * FF);
        table_.add(p + "linear2.bias", C);
        for (const char* n : {"norm1", "norm2", "norm3"}) {
            table_.add(p + n + ".weight", C);
            table_.add(p + n + ".bias", C);
        }
    }
    table_.ignore("text_proj.weight");      // built and saved by the reference, never used by its forward
    table_.ignore("text_proj.bias");
}

ImageMapper::~ImageMapper() {
    if (block_) (void)hipFree(block_);
}

int ImageMapper::validate_config() const {
    const lavie_mapper_config& c = cfg_;
    LAVIE_CHECK(c.input_dim >= IGEMM_BK && c.input_dim % IGEMM_BK == 0 && c.input_dim <= 16384,
                "mapper_create: input_dim=%d must be a multiple of %d up to 16384", c.input_dim, IGEMM_BK);
    LAVIE_CHECK(c.output_dim >= kPinBn && c.output_dim % kPinBn == 0 && c.output_dim <= 2048,
                "mapper_create: output_dim=%d must be a multiple of %d up to 2048", c.output_dim, kPinBn);
    LAVIE_CHECK(c.layers >= 1 && c.layers <= 64, "mapper_create: layers=%d must be 1..64", c.layers);
    LAVIE_CHECK(c.heads >= 1 && c.output_dim % c.heads == 0 && (c.output_dim / c.heads == 32 || c.output_dim / c.heads == 64),
                "mapper_create: heads=%d gives a head dim of output_dim / heads that is not 32 or 64 (output_dim=%d)", c.heads, c.output_dim);
    LAVIE_CHECK(c.dim_feedforward >= kPinBn && c.dim_feedforward % kPinBn == 0 && c.dim_feedforward <= 16384,
                "mapper_create: dim_feedforward=%d must be a multiple of %d up to 16384", c.dim_feedforward, kPinBn);
    LAVIE_CHECK(c.seq_in >= 1 && c.seq_in <= kShortMaxL, "mapper_create: seq_in=%d must be 1..%d", c.seq_in, kShortMaxL);
    LAVIE_CHECK(c.seq_out >= 1 && c.seq_out <= kShortMaxL, "mapper_create: seq_out=%d must be 1..%d", c.seq_out, kShortMaxL);
    LAVIE_CHECK(isfinite(c.eps) && c.eps > 0.f, "mapper_create: eps must be finite and > 0");
    return 0;
}

int ImageMapper::set_param(const char* name, const void* data, long long numel) {
    LAVIE_CHECK(!finalized_, "mapper_set_param: the handle is finalized");
    return table_.set("mapper_set_param", "", name, data, numel);
}

int ImageMapper::finalize(hipStream_t s) {
    LAVIE_CHECK(!finalized_, "mapper_finalize: the handle is finalized already");
    RUN(table_.all_set("mapper_finalize"));
    const size_t C = cfg_.output_dim, D = cfg_.input_dim, FF = cfg_.dim_feedforward;
    const long long ws = workspace_bytes(kImageMaxBatch);
    if (ws < 0) return -1;
    layers_.resize(cfg_.layers);
    auto carve = [&](char* base) {
        Carver c{base};
        wimg_ = c.take<half_t>(C * D);
        ipos_ = c.take<half_t>((size_t)cfg_.seq_in * C);
        tpos_ = c.take<half_t>((size_t)cfg_.seq_out * C);
        bimg_ = c.take<float>(C);
        for (Layer& l : layers_) {
            l.sa_in = c.take<half_t>(3 * C * C);
            l.sa_out = c.take<half_t>(C * C);
            l.ca_in = c.take<half_t>(3 * C * C);
            l.ca_out = c.take<half_t>(C * C);
            l.w1 = c.take<half_t>(FF * C);
            l.w2 = c.take<half_t>(C * FF);
            l.sa_inb = c.take<float>(3 * C);
            l.sa_outb = c.take<float>(C);
            l.ca_inb = c.take<float>(3 * C);
            l.ca_outb = c.take<float>(C);
            l.b1 = c.take<float>(FF);
            l.b2 = c.take<float>(C);
            for (float** n : {&l.n1g, &l.n1b, &l.n2g, &l.n2b, &l.n3g, &l.n3b}) *n = c.take<float>(C);
        }
        return c.used;
    };
    const size_t weights = carve(nullptr);
    if (block_) { (void)hipFree(block_); block_ = nullptr; }
    LAVIE_HIP(hipMalloc((void**)&block_, weights + (size_t)ws));
    carve(block_);
    ws_ = block_ + weights;
    auto src = [&](const std::string& n) { return table_.src(n); };
    auto to32 = [&](float* dst, const std::string& n, size_t count) { return launch_f16_to_f32(src(n), dst, (int64_t)count, s); };
    RUN(copy16(wimg_, src("image_proj.weight"), C * D, s));
    RUN(to32(bimg_, "image_proj.bias", C));
    RUN(copy16(ipos_, src("image_pos_embedding"), (size_t)cfg_.seq_in * C, s));
    RUN(copy16(tpos_, src("text_pos_embedding"), (size_t)cfg_.seq_out * C, s));
    for (int i = 0; i < cfg_.layers; ++i) {
        Layer& l = layers_[i];
        const std::string p = "transformer_decoder.layers." + std::to_string(i) + ".";
        RUN(copy16(l.sa_in, src(p + "self_attn.in_proj_weight"), 3 * C * C, s));
        RUN(to32(l.sa_inb, p + "self_attn.in_proj_bias", 3 * C));
        RUN(copy16(l.sa_out, src(p + "self_attn.out_proj.weight"), C * C, s));
        RUN(to32(l.sa_outb, p + "self_attn.out_proj.bias", C));
        RUN(copy16(l.ca_in, src(p + "multihead_attn.in_proj_weight"), 3 * C * C, s));
        RUN(to32(l.ca_inb, p + "multihead_attn.in_proj_bias", 3 * C));
        RUN(copy16(l.ca_out, src(p + "multihead_attn.out_proj.weight"), C * C, s));
        RUN(to32(l.ca_outb, p + "multihead_attn.out_proj.bias", C));
        RUN(copy16(l.w1, src(p + "linear1.weight"), FF * C, s));
        RUN(to32(l.b1, p + "linear1.bias", FF));
        RUN(copy16(l.w2, src(p + "linear2.weight"), C * FF, s));
        RUN(to32(l.b2, p + "linear2.bias", C));
        RUN(to32(l.n1g, p + "norm1.weight", C));
        RUN(to32(l.n1b, p + "norm1.bias", C));
        RUN(to32(l.n2g, p + "norm2.weight", C));
        RUN(to32(l.n2b, p + "norm2.bias", C));
        RUN(to32(l.n3g, p + "norm3.weight", C));
        RUN(to32(l.n3b, p + "norm3.bias", C));
    }
    table_.release();
    finalized_ = true;
    return 0;
}

// mem [B Si, C] | kv [B Si, 2 C] | x, t, a [B So, C] each | wide [B So, max(3 C, FF)]
long long ImageMapper::workspace_bytes(int B) const {
    if (check_batch("mapper_workspace_bytes", B)) return -1;
    const size_t Mi = (size_t)B * cfg_.seq_in, Mo = (size_t)B * cfg_.seq_out, C = cfg_.output_dim, FF = cfg_.dim_feedforward;
    const size_t wide = 3 * C > FF ? 3 * C : FF;
    return (long long)(up256(Mi * C * H) + up256(Mi * 2 * C * H) + 3 * up256(Mo * C * H) + up256(Mo * wide * H));
}

int ImageMapper::encode(const void* image_feats, int Bi, const void* text, int B, void* out, int ld_out_rows, int row0, hipStream_t s) {
    LAVIE_CHECK(finalized_, "mapper_encode: the handle is not finalized");
    LAVIE_CHECK(image_feats != nullptr, "mapper_encode: image_feats is null");
    LAVIE_CHECK(text != nullptr, "mapper_encode: text is null");
    LAVIE_CHECK(out != nullptr, "mapper_encode: out is null");
    RUN(check_batch("mapper_encode", B));
    LAVIE_CHECK(Bi == 1 || Bi == B, "mapper_encode: Bi=%d must be 1 or B=%d", Bi, B);
    const int Si = cfg_.seq_in, So = cfg_.seq_out, C = cfg_.output_dim, D = cfg_.input_dim, FF = cfg_.dim_feedforward;
    LAVIE_CHECK(row0 >= 0 && ld_out_rows >= 1 && (long long)row0 + So <= ld_out_rows,
                "mapper_encode: row0=%d + seq_out=%d rows do not fit ld_out_rows=%d", row0, So, ld_out_rows);
    const int heads = cfg_.heads, dh = C / heads, Mi = Bi * Si, Mo = B * So;
    // the carve of the workspace follows workspace_bytes(B): an encode at B uses no byte past it
    Carver c{ws_};
    const size_t wide_c = 3 * C > FF ? 3 * C : FF;
    half_t* mem = c.take<half_t>((size_t)B * Si * C);
    half_t* kv = c.take<half_t>((size_t)B * Si * 2 * C);
    half_t* x = c.take<half_t>((size_t)Mo * C);
    half_t* t = c.take<half_t>((size_t)Mo * C);
    half_t* a = c.take<half_t>((size_t)Mo * C);
    half_t* wide = c.take<half_t>((size_t)Mo * wide_c);
    const float scale = 1.0f / sqrtf((float)dh);
    const half_t* img = (const half_t*)image_feats;
    for (int b = 0; b < Bi; ++b)      // memory of image b: image_proj + bias + image positions, fp32 sum, one rounding
        RUN(pinned_linear(img + (size_t)b * Si * D, D, wimg_, bimg_, ipos_, C, mem + (size_t)b * Si * C, C, Si, C, D, s));
    RUN(launch_add_rows((const half_t*)text, tpos_, x, B, So, C, s));
    for (size_t i = 0; i < layers_.size(); ++i) {
        const Layer& l = layers_[i];
        // self-attention over the target rows
        RUN(pinned_linear(x, l.sa_in, l.sa_inb, nullptr, wide, Mo, 3 * C, C, s));
        RUN(launch_short_attention(wide, 3 * C, wide + C, 3 * C, wide + 2 * C, 3 * C, a, C, B, So, So, heads, dh, scale, false, s));
        RUN(pinned_linear(a, l.sa_out, l.sa_outb, x, t, Mo, C, C, s));
        RUN(launch_layernorm(t, l.n1g, l.n1b, x, Mo, C, cfg_.eps, s));
        // cross-attention: q from the target rows, k | v from the memory rows (in_proj rows [C, 3 C))
        RUN(pinned_linear(x, l.ca_in, l.ca_inb, nullptr, a, Mo, C, C, s));
        RUN(pinned_linear(mem, l.ca_in + (size_t)C * C, l.ca_inb + C, nullptr, kv, Mi, 2 * C, C, s));
        RUN(launch_short_attention(a, C, kv, 2 * C, kv + C, 2 * C, t, C, B, So, Si, heads, dh, scale, Bi == 1 && B > 1, s));
        RUN(pinned_linear(t, l.ca_out, l.ca_outb, x, a, Mo, C, C, s));
        RUN(launch_layernorm(a, l.n2g, l.n2b, x, Mo, C, cfg_.eps, s));
        // feed-forward
        RUN(pinned_linear(x, l.w1, l.b1, nullptr, wide, Mo, FF, C, s));
        RUN(launch_relu(wide, (int64_t)Mo * FF, s));
        RUN(pinned_linear(wide, l.w2, l.b2, x, t, Mo, C, FF, s));
        if (i + 1 < layers_.size()) {
            RUN(launch_layernorm(t, l.n3g, l.n3b, x, Mo, C, cfg_.eps, s));
        } else {
            for (int b = 0; b < B; ++b)      // the last norm writes the caller's rows; LayerNorm works row by row
                RUN(launch_layernorm(t + (size_t)b * So * C, l.n3g, l.n3b, (half_t*)out + ((size_t)b * ld_out_rows + row0) * C, So, C, cfg_.eps, s));
        }
    }
    return 0;
}

}  // namespace lavie
