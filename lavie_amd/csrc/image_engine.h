// Image conditioning on the engine's operators: the objects behind lavie_vision_* (CLIPVisionTransformer up to
// last_hidden_state) and lavie_mapper_* (the fork's MappingNetwork).  Same lifecycle as TextEncoder (text_engine.h).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lavie_hip.h"
#include "common.h"

namespace lavie {

constexpr int kImageMaxBatch = 16;

// The named fp16 tensors of a handle: listed at construction, borrowed from set_param until finalize
class ParamTable {
public:
    struct Param {
        std::string name;
        long long numel;
        const half_t* src;
    };
    void add(const std::string& name, long long numel);
    void ignore(const std::string& name) { ignored_.push_back(name); }
    const std::vector<Param>& params() const { return params_; }
    // who: the entry point's name for the messages; prefix: accepted in front of every name and added when missing ("" = none)
    int set(const char* who, const char* prefix, const char* name, const void* data, long long numel);
    int all_set(const char* who) const;
    const half_t* src(const std::string& name) const { return params_[index_.at(name)].src; }
    void release();

private:
    std::vector<Param> params_;
    std::vector<std::string> ignored_;
    std::unordered_map<std::string, int> index_;
};

class VisionEncoder {
public:
    explicit VisionEncoder(const lavie_vision_config& cfg);
    ~VisionEncoder();
    VisionEncoder(const VisionEncoder&) = delete;
    VisionEncoder& operator=(const VisionEncoder&) = delete;

    int validate_config() const;
    const std::vector<ParamTable::Param>& params() const { return table_.params(); }
    int set_param(const char* name, const void* data_f16, long long numel);
    int finalize(hipStream_t s);
    long long workspace_bytes(int B) const;      // what encode(B) uses; -1 with a message for a batch it refuses
    int encode(const void* pixel_values, int x_dtype, int B, void* out_f16, hipStream_t s);
    int tokens() const { return cfg_.patch_size > 0 ? 1 + (cfg_.image_size / cfg_.patch_size) * (cfg_.image_size / cfg_.patch_size) : 0; }

private:
    struct Layer {
        half_t *wqkv, *wo, *w1, *w2;
        float *bqkv, *bo, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
    };
    lavie_vision_config cfg_;
    ParamTable table_;
    bool finalized_ = false;
    char* block_ = nullptr;         // weights, then the workspace
    half_t *wpatch_ = nullptr, *cls_ = nullptr, *pos_ = nullptr;
    float *preg_ = nullptr, *preb_ = nullptr;
    std::vector<Layer> layers_;
    char* ws_ = nullptr;
};

class ImageMapper {
public:
    explicit ImageMapper(const lavie_mapper_config& cfg);
    ~ImageMapper();
    ImageMapper(const ImageMapper&) = delete;
    ImageMapper& operator=(const ImageMapper&) = delete;

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
    bool finalized_ = false;
    char* block_ = nullptr;
    half_t *wimg_ = nullptr, *ipos_ = nullptr, *tpos_ = nullptr;
    float* bimg_ = nullptr;
    std::vector<Layer> layers_;
    char* ws_ = nullptr;
};

}  // namespace lavie
