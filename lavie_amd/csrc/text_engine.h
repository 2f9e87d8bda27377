// CLIPTextModel on the engine's operators: the object behind lavie_text_*.
#pragma once
#include "encoder_parts.h"

namespace lavie {

constexpr int kTextMaxBatch = 16;

class TextEncoder {
public:
    explicit TextEncoder(const lavie_text_config& cfg);

    int validate_config() const;
    const std::vector<ParamTable::Param>& params() const { return table_.params(); }
    int set_param(const char* name, const void* data_f16, long long numel);
    // Copies every tensor into one allocation of the handle's own (q | k | v weights and biases fused, biases and norm vectors fp32)
    // and allocates the workspace of the largest call (kTextMaxBatch x max_positions): encode never allocates.
    int finalize(hipStream_t s);
    long long workspace_bytes(int B, int L) const;      // what encode(B, L) uses of it; -1 with a message for a shape it refuses
    int encode(const int* ids_dev, int B, int L, void* out_f16, hipStream_t s);

private:
    int check_shape(const char* who, int B, int L) const;

    lavie_text_config cfg_;
    ClipShape shape_;
    ParamTable table_;
    WeightBlock block_;
    half_t *tok_ = nullptr, *pos_ = nullptr;
    float *lnfg_ = nullptr, *lnfb_ = nullptr;
    std::vector<ClipLayer> layers_;
};

}  // namespace lavie
