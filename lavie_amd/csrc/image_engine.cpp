// CLIPVisionTransformer (transformers modeling_clip.py) up to last_hidden_state and the fork's MappingNetwork
// (base/pipelines/mapping.py:61-97 of the reference: nn.TransformerDecoder, post-norm, ReLU) on the engine's operators.
// Vision, on rows x [B T, C]:   x = pre_layrnorm(embeddings(pixels)); then the CLIP layers of encoder_parts.h
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

namespace lavie {

namespace {

constexpr size_t H = sizeof(half_t);

int check_batch(const char* who, int B) {
    LAVIE_CHECK(B >= 1 && B <= kImageMaxBatch, "%s: B=%d must be 1..%d", who, B, kImageMaxBatch);
    return 0;
}

}  // namespace

// ------------------------------------------------------------------ the vision tower
static const std::string kVis = "vision_model.";

VisionEncoder::VisionEncoder(const lavie_vision_config& cfg)
    : cfg_(cfg), shape_{cfg.hidden, cfg.intermediate, cfg.layers, cfg.heads, cfg.act, cfg.eps} {
    const long long C = cfg.hidden;
    if (cfg.layers < 0 || cfg.layers > 1024 || cfg.patch_size < 1 || cfg.patch_size > 64 || cfg.image_size < 1 || cfg.image_size > 1024) return;
    table_.add(kVis + "embeddings.class_embedding", C);
    table_.add(kVis + "embeddings.patch_embedding.weight", C * 3 * cfg.patch_size * cfg.patch_size);
    table_.add(kVis + "embeddings.position_embedding.weight", (long long)tokens() * C);
    table_.add(kVis + "pre_layrnorm.weight", C);
    table_.add(kVis + "pre_layrnorm.bias", C);
    for (int i = 0; i < cfg.layers; ++i) list_clip_layer(table_, kVis + "encoder.layers." + std::to_string(i) + ".", shape_);
    table_.ignore(kVis + "post_layernorm.weight");      // the pooled output's norm: not part of last_hidden_state
    table_.ignore(kVis + "post_layernorm.bias");
}

int VisionEncoder::validate_config() const {
    const lavie_vision_config& c = cfg_;
    RUN(check_clip_shape("vision_create", shape_));
    LAVIE_CHECK(c.patch_size >= 1 && c.patch_size <= 64, "vision_create: patch_size=%d must be 1..64", c.patch_size);
    LAVIE_CHECK(c.image_size >= c.patch_size && c.image_size <= 1024 && c.image_size % c.patch_size == 0,
                "vision_create: image_size=%d must be a multiple of patch_size=%d up to 1024", c.image_size, c.patch_size);
    LAVIE_CHECK(tokens() <= kShortMaxL, "vision_create: image_size=%d / patch_size=%d gives %d tokens, more than %d", c.image_size, c.patch_size,
                tokens(), kShortMaxL);
    return 0;
}

int VisionEncoder::set_param(const char* name, const void* data, long long numel) {
    RUN(check_open(block_, "vision_set_param"));
    return table_.set("vision_set_param", kVis.c_str(), name, data, numel);
}

int VisionEncoder::finalize(hipStream_t s) {
    RUN(check_open(block_, "vision_finalize", " already"));
    RUN(table_.all_set("vision_finalize"));
    const size_t C = cfg_.hidden, T = tokens(), Kp = patch_embed_k(cfg_.patch_size);
    layers_.resize(cfg_.layers);
    RUN(allocate(block_, workspace_bytes(kImageMaxBatch), [&](char* base) {
        Carver c{base};
        wpatch_ = c.take<half_t>(C * Kp);
        cls_ = c.take<half_t>(C);
        pos_ = c.take<half_t>(T * C);
        preg_ = c.take<float>(C);
        preb_ = c.take<float>(C);
        for (ClipLayer& l : layers_) carve_clip_layer(c, l, shape_);
        return c.used;
    }));
    RUN(launch_pack_patch_embed(table_.src(kVis + "embeddings.patch_embedding.weight"), wpatch_, (int)C, cfg_.patch_size, s));
    RUN(copy16(cls_, table_.src(kVis + "embeddings.class_embedding"), C, s));
    RUN(copy16(pos_, table_.src(kVis + "embeddings.position_embedding.weight"), T * C, s));
    RUN(launch_f16_to_f32(table_.src(kVis + "pre_layrnorm.weight"), preg_, (int64_t)C, s));
    RUN(launch_f16_to_f32(table_.src(kVis + "pre_layrnorm.bias"), preb_, (int64_t)C, s));
    for (int i = 0; i < cfg_.layers; ++i)
        RUN(pack_clip_layer(table_, kVis + "encoder.layers." + std::to_string(i) + ".", layers_[i], shape_, s));
    table_.release();
    block_.finalized = true;
    return 0;
}

// the CLIP layers' workspace | the gathered patches
long long VisionEncoder::workspace_bytes(int B) const {
    if (check_batch("vision_workspace_bytes", B)) return -1;
    Carver c{nullptr};
    carve_clip_workspace(c, (size_t)B * tokens(), shape_);
    return (long long)c.used + patch_embed_workspace_bytes(B, cfg_.image_size, cfg_.patch_size);
}

int VisionEncoder::encode(const void* px, int x_dtype, int B, void* out, hipStream_t s) {
    LAVIE_CHECK(block_.finalized, "vision_encode: the handle is not finalized");
    LAVIE_CHECK(px != nullptr, "vision_encode: pixel_values is null");
    LAVIE_CHECK(out != nullptr, "vision_encode: out_f16 is null");
    LAVIE_CHECK(x_dtype == 0 || x_dtype == 1, "vision_encode: x_dtype=%d (0 = fp16, 1 = fp32)", x_dtype);
    RUN(check_batch("vision_encode", B));
    const int T = tokens(), C = cfg_.hidden;
    Carver c{block_.ws};
    const ClipWorkspace w = carve_clip_workspace(c, (size_t)B * T, shape_);
    half_t* cols = (half_t*)(block_.ws + c.used);
    RUN(launch_patch_embed(px, x_dtype == 1, wpatch_, cls_, pos_, w.h, cols, B, cfg_.image_size, cfg_.patch_size, C, s));
    RUN(launch_layernorm(w.h, preg_, preb_, w.x, B * T, C, cfg_.eps, s));
    for (size_t i = 0; i < layers_.size(); ++i)      // the last residual sum is last_hidden_state
        RUN(run_clip_layer(layers_[i], shape_, w, B, T, false, i + 1 == layers_.size() ? (half_t*)out : w.x, s));
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
    RUN(check_open(block_, "mapper_set_param"));
    return table_.set("mapper_set_param", "", name, data, numel);
}

int ImageMapper::finalize(hipStream_t s) {
    RUN(check_open(block_, "mapper_finalize", " already"));
    RUN(table_.all_set("mapper_finalize"));
    const size_t C = cfg_.output_dim, D = cfg_.input_dim, FF = cfg_.dim_feedforward;
    layers_.resize(cfg_.layers);
    RUN(allocate(block_, workspace_bytes(kImageMaxBatch), [&](char* base) {
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
    }));
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
    block_.finalized = true;
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
    LAVIE_CHECK(block_.finalized, "mapper_encode: the handle is not finalized");
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
    Carver c{block_.ws};
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
