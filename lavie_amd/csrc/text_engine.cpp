// CLIPTextModel (transformers modeling_clip.py: CLIPTextTransformer) on the engine's operators: token + position embedding, N pre-LN
// layers of causal self-attention and a two-layer MLP, the final LayerNorm.  Launches of one layer, on rows x [B L, C]:
//   h = LN1(x); qkv = h Wqkv^T + b; h = causal_attention(qkv); x = h Wo^T + bo + x; h = LN2(x); m = h W1^T + b1; act(m);
//   x = m W2^T + b2 + x
// Every tensor between two launches is fp16.  The GEMMs do NOT go through the planner: it chooses by (M, N, K) and M = B L moves with
// the batch.  They are launched with one fixed plan, the 128-row kernel at 128 columns and no split-K, under which an output
// element is the sum of its K products in an order that depends on K alone; every other launch works row by row or (batch entry, head)
// by (batch entry, head).  So a prompt's [L, C] block has the same bits at every batch size and position.
#include "text_engine.h"

#include <math.h>

#include "ops.h"
#include "pinned_linear.h"

namespace lavie {

#define RUN(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

TextEncoder::TextEncoder(const lavie_text_config& cfg) : cfg_(cfg) {
    const long long C = cfg.hidden, I = cfg.intermediate;
    auto add = [&](const std::string& name, long long numel) {
        index_[name] = (int)params_.size();
        params_.push_back({name, numel, nullptr});
    };
    if (cfg.layers < 0 || cfg.layers > 1024) return;      // validate_config refuses it; no list to build
    add("text_model.embeddings.token_embedding.weight", (long long)cfg.vocab_size * C);
    add("text_model.embeddings.position_embedding.weight", (long long)cfg.max_positions * C);
    for (int i = 0; i < cfg.layers; ++i) {
        const std::string p = "text_model.encoder.layers." + std::to_string(i) + ".";
        for (const char* proj : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
            add(p + "self_attn." + proj + ".weight", C * C);
            add(p + "self_attn." + proj + ".bias", C);
        }
        add(p + "layer_norm1.weight", C);
        add(p + "layer_norm1.bias", C);
        add(p + "mlp.fc1.weight", I * C);
        add(p + "mlp.fc1.bias", I);
        add(p + "mlp.fc2.weight", C * I);
        add(p + "mlp.fc2.bias", C);
        add(p + "layer_norm2.weight", C);
        add(p + "layer_norm2.bias", C);
    }
    add("text_model.final_layer_norm.weight", C);
    add("text_model.final_layer_norm.bias", C);
}

TextEncoder::~TextEncoder() {
    if (block_) (void)hipFree(block_);
}

int TextEncoder::validate_config() const {
    const lavie_text_config& c = cfg_;
    LAVIE_CHECK(c.vocab_size >= 1, "text_create: vocab_size=%d", c.vocab_size);
    LAVIE_CHECK(c.hidden >= kPinBn && c.hidden % kPinBn == 0 && c.hidden <= 2048, "text_create: hidden=%d must be a multiple of %d up to 2048",
                c.hidden, kPinBn);
    LAVIE_CHECK(c.intermediate >= kPinBn && c.intermediate % kPinBn == 0 && c.intermediate <= 16384,
                "text_create: intermediate=%d must be a multiple of %d up to 16384", c.intermediate, kPinBn);
    LAVIE_CHECK(c.layers >= 1 && c.layers <= 64, "text_create: layers=%d must be 1..64", c.layers);
    LAVIE_CHECK(c.heads >= 1 && c.hidden % c.heads == 0 && (c.hidden / c.heads == 32 || c.hidden / c.heads == 64),
                "text_create: heads=%d gives a head dim of hidden / heads that is not 32 or 64 (hidden=%d)", c.heads, c.hidden);
    LAVIE_CHECK(c.max_positions >= 1 && c.max_positions <= kCausalMaxL, "text_create: max_positions=%d must be 1..%d", c.max_positions,
                kCausalMaxL);
    LAVIE_CHECK(c.act == LAVIE_TEXT_ACT_QUICK_GELU || c.act == LAVIE_TEXT_ACT_GELU, "text_create: act=%d is neither quick_gelu (0) nor gelu (1)",
                c.act);
    LAVIE_CHECK(isfinite(c.eps) && c.eps > 0.f, "text_create: eps must be finite and > 0");
    return 0;
}

int TextEncoder::set_param(const char* name, const void* data, long long numel) {
    LAVIE_CHECK(!finalized_, "text_set_param: the handle is finalized");
    auto it = index_.find(name);
    LAVIE_CHECK(it != index_.end(), "text_set_param: unknown state-dict key '%s'", name);
    Param& pi = params_[it->second];
    LAVIE_CHECK(pi.numel == numel, "text_set_param: '%s' has %lld elements, expected %lld", name, numel, pi.numel);
    LAVIE_CHECK(data != nullptr, "text_set_param: '%s' null data", name);
    pi.src = (const half_t*)data;
    return 0;
}

const half_t* TextEncoder::src(const std::string& name) const { return params_[index_.at(name)].src; }

int TextEncoder::finalize(hipStream_t s) {
    LAVIE_CHECK(!finalized_, "text_finalize: the handle is finalized already");
    for (const Param& p : params_) LAVIE_CHECK(p.src != nullptr, "text_finalize: '%s' was never set", p.name.c_str());
    const size_t C = cfg_.hidden, I = cfg_.intermediate, V = cfg_.vocab_size, P = cfg_.max_positions, H = sizeof(half_t), F = sizeof(float);
    const size_t per_layer = up256(3 * C * C * H) + up256(C * C * H) + 2 * up256(I * C * H) + up256(3 * C * F) + 6 * up256(C * F) + up256(I * F);
    const size_t weights = up256(V * C * H) + up256(P * C * H) + 2 * up256(C * F) + cfg_.layers * per_layer;
    const long long ws = workspace_bytes(kTextMaxBatch, cfg_.max_positions);
    if (ws < 0) return -1;
    if (block_) { (void)hipFree(block_); block_ = nullptr; }      // a finalize that failed half way
    LAVIE_HIP(hipMalloc((void**)&block_, weights + (size_t)ws));
    char* cur = block_;
    auto take = [&](size_t bytes) { char* r = cur; cur += up256(bytes); return r; };
    auto copy16 = [&](half_t* dst, const std::string& name, size_t n) -> int {
        LAVIE_HIP(hipMemcpyAsync(dst, src(name), n * H, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    auto to32 = [&](float* dst, const std::string& name, size_t n) { return launch_f16_to_f32(src(name), dst, (int64_t)n, s); };
    tok_ = (half_t*)take(V * C * H);
    pos_ = (half_t*)take(P * C * H);
    lnfg_ = (float*)take(C * F);
    lnfb_ = (float*)take(C * F);
    RUN(copy16(tok_, "text_model.embeddings.token_embedding.weight", V * C));
    RUN(copy16(pos_, "text_model.embeddings.position_embedding.weight", P * C));
    RUN(to32(lnfg_, "text_model.final_layer_norm.weight", C));
    RUN(to32(lnfb_, "text_model.final_layer_norm.bias", C));
    layers_.resize(cfg_.layers);
    for (int i = 0; i < cfg_.layers; ++i) {
        Layer& l = layers_[i];
        const std::string p = "text_model.encoder.layers." + std::to_string(i) + ".";
        l.wqkv = (half_t*)take(3 * C * C * H);
        l.wo = (half_t*)take(C * C * H);
        l.w1 = (half_t*)take(I * C * H);
        l.w2 = (half_t*)take(C * I * H);
        l.bqkv = (float*)take(3 * C * F);
        l.bo = (float*)take(C * F);
        l.b1 = (float*)take(I * F);
        l.b2 = (float*)take(C * F);
        l.ln1g = (float*)take(C * F);
        l.ln1b = (float*)take(C * F);
        l.ln2g = (float*)take(C * F);
        l.ln2b = (float*)take(C * F);
        const char* qkv[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            RUN(copy16(l.wqkv + j * C * C, p + "self_attn." + qkv[j] + ".weight", C * C));
            RUN(to32(l.bqkv + j * C, p + "self_attn." + qkv[j] + ".bias", C));
        }
        RUN(copy16(l.wo, p + "self_attn.out_proj.weight", C * C));
        RUN(to32(l.bo, p + "self_attn.out_proj.bias", C));
        RUN(copy16(l.w1, p + "mlp.fc1.weight", I * C));
        RUN(to32(l.b1, p + "mlp.fc1.bias", I));
        RUN(copy16(l.w2, p + "mlp.fc2.weight", C * I));
        RUN(to32(l.b2, p + "mlp.fc2.bias", C));
        RUN(to32(l.ln1g, p + "layer_norm1.weight", C));
        RUN(to32(l.ln1b, p + "layer_norm1.bias", C));
        RUN(to32(l.ln2g, p + "layer_norm2.weight", C));
        RUN(to32(l.ln2b, p + "layer_norm2.bias", C));
    }
    ws_ = cur;
    for (Param& p : params_) p.src = nullptr;      // the loan ends when the stream drains
    finalized_ = true;
    return 0;
}

int TextEncoder::check_shape(const char* who, int B, int L) const {
    LAVIE_CHECK(B >= 1 && B <= kTextMaxBatch, "%s: B=%d must be 1..%d", who, B, kTextMaxBatch);
    LAVIE_CHECK(L >= 1 && L <= cfg_.max_positions, "%s: L=%d must be 1..max_positions=%d", who, L, cfg_.max_positions);
    return 0;
}

// x [M, C] | h [M, C] | wide [M, max(3 C, I)]
long long TextEncoder::workspace_bytes(int B, int L) const {
    if (check_shape("text_workspace_bytes", B, L)) return -1;
    const size_t M = (size_t)B * L, C = cfg_.hidden, I = cfg_.intermediate, wide = 3 * C > I ? 3 * C : I;
    return (long long)(2 * up256(M * C * sizeof(half_t)) + up256(M * wide * sizeof(half_t)));
}

int TextEncoder::encode(const int* ids, int B, int L, void* out, hipStream_t s) {
    LAVIE_CHECK(finalized_, "text_encode: the handle is not finalized");
    LAVIE_CHECK(ids != nullptr, "text_encode: ids_dev is null");
    LAVIE_CHECK(out != nullptr, "text_encode: out_f16 is null");
    RUN(check_shape("text_encode", B, L));
    const int M = B * L, C = cfg_.hidden, I = cfg_.intermediate, heads = cfg_.heads, dh = C / heads;
    half_t* x = (half_t*)ws_;
    half_t* h = (half_t*)(ws_ + up256((size_t)M * C * sizeof(half_t)));
    half_t* wide = (half_t*)(ws_ + 2 * up256((size_t)M * C * sizeof(half_t)));
    const float scale = 1.0f / sqrtf((float)dh);
    RUN(launch_token_embed(ids, tok_, pos_, x, B, L, C, cfg_.vocab_size, s));
    for (const Layer& l : layers_) {
        RUN(launch_layernorm(x, l.ln1g, l.ln1b, h, M, C, cfg_.eps, s));
        RUN(pinned_linear(h, l.wqkv, l.bqkv, nullptr, wide, M, 3 * C, C, s));
        RUN(launch_causal_attention(wide, 3 * C, h, C, B, L, heads, dh, scale, s));
        RUN(pinned_linear(h, l.wo, l.bo, x, x, M, C, C, s));
        RUN(launch_layernorm(x, l.ln2g, l.ln2b, h, M, C, cfg_.eps, s));
        RUN(pinned_linear(h, l.w1, l.b1, nullptr, wide, M, I, C, s));
        RUN(launch_act(wide, (int64_t)M * I, cfg_.act, s));
        RUN(pinned_linear(wide, l.w2, l.b2, x, x, M, C, I, s));
    }
    return launch_layernorm(x, lnfg_, lnfb_, (half_t*)out, M, C, cfg_.eps, s);
}

}  // namespace lavie
