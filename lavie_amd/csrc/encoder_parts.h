// What the weight-holding objects behind lavie_text_*, lavie_vision_* and lavie_mapper_* share: the table of
// named parameters, the carver and owner of the one allocation, and the CLIP pre-LN layer of the text encoder and the vision tower.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lavie_hip.h"
#include "common.h"
#include "pinned_linear.h"

namespace lavie {

#define RUN(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

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

int copy16(half_t* dst, const half_t* src, size_t n, hipStream_t s);

// The one allocation of a handle: its packed weights, then the workspace of its largest call
struct WeightBlock {
    char* base = nullptr;
    char* ws = nullptr;
    bool finalized = false;
    WeightBlock() = default;
    ~WeightBlock() {
        if (base) (void)hipFree(base);
    }
    WeightBlock(const WeightBlock&) = delete;
    WeightBlock& operator=(const WeightBlock&) = delete;
};

// set_param's refusal, and with tail = " already" finalize's
inline int check_open(const WeightBlock& b, const char* who, const char* tail = "") {
    LAVIE_CHECK(!b.finalized, "%s: the handle is finalized%s", who, tail);
    return 0;
}

// carve(base) places every weight from base on and returns the bytes it used; run once with nullptr to count, once to place
template <class Carve>
int allocate(WeightBlock& b, long long ws_bytes, Carve&& carve) {
    if (ws_bytes < 0) return -1;
    const size_t weights = carve((char*)nullptr);
    if (b.base) { (void)hipFree(b.base); b.base = nullptr; }      // a finalize that failed half way
    LAVIE_HIP(hipMalloc((void**)&b.base, weights + (size_t)ws_bytes));
    carve(b.base);
    b.ws = b.base + weights;
    return 0;
}

// ---- the CLIP pre-LN layer (transformers modeling_clip.py: CLIPEncoderLayer), on rows x [B T, C]:
//   h = LN1(x); qkv = h Wqkv^T + b; h = attention(qkv); x = h Wo^T + bo + x; h = LN2(x); m = act(h W1^T + b1); dst = m W2^T + b2 + x
struct ClipShape {
    int hidden, intermediate, layers, heads, act;
    float eps;
};

struct ClipLayer {
    half_t *wqkv, *wo, *w1, *w2;
    float *bqkv, *bo, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
};

struct ClipWorkspace {
    half_t *x, *h, *wide;      // x [M, C] | h [M, C] | wide [M, max(3 C, I)]
};

int check_clip_shape(const char* who, const ClipShape& c);      // who: "text_create", "vision_create"
void list_clip_layer(ParamTable& t, const std::string& prefix, const ClipShape& c);
void carve_clip_layer(Carver& c, ClipLayer& l, const ClipShape& sh);
// q | k | v weights and biases fused in that order, biases and norm vectors to fp32
int pack_clip_layer(const ParamTable& t, const std::string& prefix, const ClipLayer& l, const ClipShape& c, hipStream_t s);
ClipWorkspace carve_clip_workspace(Carver& c, size_t M, const ClipShape& sh);
// causal: launch_causal_attention (the text encoder), else launch_short_attention over all T keys (the vision tower); the last
// residual sum lands in dst, which may be w.x
int run_clip_layer(const ClipLayer& l, const ClipShape& c, const ClipWorkspace& w, int B, int T, bool causal, half_t* dst, hipStream_t s);

}  // namespace lavie
