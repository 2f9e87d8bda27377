// CLIPTextModel on the engine's operators: the object behind lavie_text_*.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lavie_hip.h"
#include "common.h"

namespace lavie {

constexpr int kTextMaxBatch = 16;

class TextEncoder {
public:
    struct Param {
        std::string name;
        long long numel;
        const half_t* src;      // the caller's tensor, borrowed from set_param until finalize
    };
    explicit TextEncoder(const lavie_text_config& cfg);
    ~TextEncoder();
    TextEncoder(const TextEncoder&) = delete;
    TextEncoder& operator=(const TextEncoder&) = delete;

    int validate_config() const;
    const std::vector<Param>& params() const { return params_; }
    int set_param(const char* name, const void* data_f16, long long numel);
    // Copies every tensor into one allocation of the handle's own (q | k | v weights and biases fused, biases and norm vectors fp32)
    // and allocates the workspace of the largest call (kTextMaxBatch x max_positions): encode never allocates.
    int finalize(hipStream_t s);
    long long workspace_bytes(int B, int L) const;      // what encode(B, L) uses of it; -1 with a message for a shape it refuses
    int encode(const int* ids_dev, int B, int L, void* out_f16, hipStream_t s);

private:
    struct Layer {
        half_t *wqkv, *wo, *w1, *w2;
        float *bqkv, *bo, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
    };
    const half_t* src(const std::string& name) const;
    int check_shape(const char* who, int B, int L) const;

    lavie_text_config cfg_;
    std::vector<Param> params_;
    std::unordered_map<std::string, int> index_;
    bool finalized_ = false;
    char* block_ = nullptr;         // weights, then the workspace
    half_t *tok_ = nullptr, *pos_ = nullptr;
    float *lnfg_ = nullptr, *lnfb_ = nullptr;
    std::vector<Layer> layers_;
    char* ws_ = nullptr;
};

}  // namespace lavie
