// What every weight-holding object behind the C ABI shares (the UNet, the text encoder, the vision tower, the mapper, R3D-18; DESIGN.md
// 7.16): the table of named parameters, lent by set_param until finalize, and for the four encoders the carver and owner of the one
// allocation.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

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
        bool required;
    };
    // required = false: listed and checked by set like any other, but finalize reads nothing of it and all_set does not ask for it
    void add(const std::string& name, long long numel, bool required = true);
    void ignore(const std::string& name) { ignored_.push_back(name); }
    const std::vector<Param>& params() const { return params_; }
    // who: the entry point's name for the messages; prefix: accepted in front of every name and added when missing ("" = none)
    int set(const char* who, const char* prefix, const char* name, const void* data, long long numel);
    int all_set(const char* who) const;
    const Param* find(const std::string& name) const;      // nullptr: not listed
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
        used += (count * sizeof(T) + 255) & ~(size_t)255;
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

}  // namespace lavie
