// CLIPTextModel (transformers modeling_clip.py: CLIPTextTransformer) on the engine's operators: token + position embedding, N pre-LN
// layers of causal self-attention and a two-layer MLP (the CLIP layer of encoder_parts.h), the final LayerNorm.
// Every tensor between two launches is fp16.  The GEMMs do NOT go through the planner: it chooses by (M, N, K) and M = B L moves with
// the batch.  They are launched with one fixed plan, the 128-row kernel at 128 columns and no split-K, under which an output
// element is the sum of its K products in an order that depends on K alone; every other launch works row by row or (batch entry, head)
// by (batch entry, head).  So a prompt's [L, C] block has the same bits at every batch size and position.
#include "text_engine.h"

#include "ops.h"

namespace lavie {

static const std::string kText = "text_model.";

TextEncoder::TextEncoder(const lavie_text_config& cfg)
    : cfg_(cfg), shape_{cfg.hidden, cfg.intermediate, cfg.layers, cfg.heads, cfg.act, cfg.eps} {
    const long long C = cfg.hidden;
    if (cfg.layers < 0 || cfg.layers > 1024) return;      // validate_config refuses it; no list to build
    table_.add(kText + "embeddings.token_embedding.weight", (long long)cfg.vocab_size * C);
    table_.add(kText + "embeddings.position_embedding.weight", (long long)cfg.max_positions * C);
    for (int i = 0; i < cfg.layers; ++i) list_clip_layer(table_, kText + "encoder.layers." + std::to_string(i) + ".", shape_);
    table_.add(kText + "final_layer_norm.weight", C);
    table_.add(kText + "final_layer_norm.bias", C);
}

int TextEncoder::validate_config() const {
    const lavie_text_config& c = cfg_;
    LAVIE_CHECK(c.vocab_size >= 1, "text_create: vocab_size=%d", c.vocab_size);
    RUN(check_clip_shape("text_create", shape_));
    LAVIE_CHECK(c.max_positions >= 1 && c.max_positions <= kCausalMaxL, "text_create: max_positions=%d must be 1..%d", c.max_positions,
                kCausalMaxL);
    return 0;
}

// the names carry text_model. and only that spelling is taken: no prefix is added for the caller
int TextEncoder::set_param(const char* name, const void* data, long long numel) {
    RUN(check_open(block_, "text_set_param"));
    return table_.set("text_set_param", "", name, data, numel);
}

int TextEncoder::finalize(hipStream_t s) {
    RUN(check_open(block_, "text_finalize", " already"));
    RUN(table_.all_set("text_finalize"));
    const size_t C = cfg_.hidden, V = cfg_.vocab_size, P = cfg_.max_positions;
    layers_.resize(cfg_.layers);
    RUN(allocate(block_, workspace_bytes(kTextMaxBatch, cfg_.max_positions), [&](char* base) {
        Carver c{base};
        tok_ = c.take<half_t>(V * C);
        pos_ = c.take<half_t>(P * C);
        lnfg_ = c.take<float>(C);
        lnfb_ = c.take<float>(C);
        for (ClipLayer& l : layers_) carve_clip_layer(c, l, shape_);
        return c.used;
    }));
    RUN(copy16(tok_, table_.src(kText + "embeddings.token_embedding.weight"), V * C, s));
    RUN(copy16(pos_, table_.src(kText + "embeddings.position_embedding.weight"), P * C, s));
    RUN(launch_f16_to_f32(table_.src(kText + "final_layer_norm.weight"), lnfg_, (int64_t)C, s));
    RUN(launch_f16_to_f32(table_.src(kText + "final_layer_norm.bias"), lnfb_, (int64_t)C, s));
    for (int i = 0; i < cfg_.layers; ++i)
        RUN(pack_clip_layer(table_, kText + "encoder.layers." + std::to_string(i) + ".", layers_[i], shape_, s));
    table_.release();
    block_.finalized = true;
    return 0;
}

int TextEncoder::check_shape(const char* who, int B, int L) const {
    LAVIE_CHECK(B >= 1 && B <= kTextMaxBatch, "%s: B=%d must be 1..%d", who, B, kTextMaxBatch);
    LAVIE_CHECK(L >= 1 && L <= cfg_.max_positions, "%s: L=%d must be 1..max_positions=%d", who, L, cfg_.max_positions);
    return 0;
}

long long TextEncoder::workspace_bytes(int B, int L) const {
    if (check_shape("text_workspace_bytes", B, L)) return -1;
    Carver c{nullptr};
    carve_clip_workspace(c, (size_t)B * L, shape_);
    return (long long)c.used;
}

int TextEncoder::encode(const int* ids, int B, int L, void* out, hipStream_t s) {
    LAVIE_CHECK(block_.finalized, "text_encode: the handle is not finalized");
    LAVIE_CHECK(ids != nullptr, "text_encode: ids_dev is null");
    LAVIE_CHECK(out != nullptr, "text_encode: out_f16 is null");
    RUN(check_shape("text_encode", B, L));
    Carver c{block_.ws};
    const ClipWorkspace w = carve_clip_workspace(c, (size_t)B * L, shape_);
    RUN(launch_token_embed(ids, tok_, pos_, w.x, B, L, cfg_.hidden, cfg_.vocab_size, s));
    for (const ClipLayer& l : layers_) RUN(run_clip_layer(l, shape_, w, B, L, true, w.x, s));
    return launch_layernorm(w.x, lnfg_, lnfb_, (half_t*)out, B * L, cfg_.hidden, cfg_.eps, s);
}

}  // namespace lavie
