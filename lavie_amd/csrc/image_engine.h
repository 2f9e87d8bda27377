// Image conditioning on the engine's operators: the objects behind lavie_vision_* (CLIPVisionTransformer up to
// last_hidden_state) and lavie_mapper_* (the fork's MappingNetwork).  Same lifecycle as TextEncoder (text_engine.h).
#pragma once
#include "encoder_parts.h"

namespace lavie {

constexpr int kImageMaxBatch = 16;

class VisionEncoder {
public:
    explicit VisionEncoder(const lavie_vision_config& cfg);

    int validate_config() const;
    const std::vector<ParamTable::Param>& params() const { return table_.params(); }
    int set_param(const char* name, const void* data_f16, long long numel);
    int finalize(hipStream_t s);
    long long workspace_bytes(int B) const;      // what encode(B) uses; -1 with a message for a batch it refuses
    int encode(const void* pixel_values, int x_dtype, int B, void* out_f16, hipStream_t s);
    int tokens() const { return cfg_.patch_size > 0 ? 1 + (cfg_.image_size / cfg_.patch_size) * (cfg_.image_size / cfg_.patch_size) : 0; }

private:
    lavie_vision_config cfg_;
    ClipShape shape_;
    ParamTable table_;
    WeightBlock block_;
    half_t *wpatch_ = nullptr, *cls_ = nullptr, *pos_ = nullptr;
    float *preg_ = nullptr, *preb_ = nullptr;
    std::vector<ClipLayer> layers_;
};

class ImageMapper {
public:
    explicit ImageMapper(const lavie_mapper_config& cfg);

    int validate_config() const;
    const std::vector<ParamTable::Param>& params() const { return table_.params(); }
    int set_param(const char* name, const void* data_f16, long long numel);
    int finalize(hipStream_t s);
    long long workspace_bytes(int B) const;
    int encode(const void* image_feats, int Bi, const void* text, int B, void* out, int ld_out_rows, int row0, hipStream_t s);

private:
    struct Layer {
        half_t *sa_in, *sa_out, *ca_in, *ca_out, *w1, *w2;      // in_proj [3 C, C]: q rows [0, C), k | v rows [C, 3 C)
        float *sa_inb, *sa_outb, *ca_inb, *ca_outb, *b1, *b2, *n1g, *n1b, *n2g, *n2b, *n3g, *n3b;
    };
    lavie_mapper_config cfg_;
    ParamTable table_;
    WeightBlock block_;
    half_t *wimg_ = nullptr, *ipos_ = nullptr, *tpos_ = nullptr;
    float* bimg_ = nullptr;
    std::vector<Layer> layers_;
};

}  // namespace lavie
