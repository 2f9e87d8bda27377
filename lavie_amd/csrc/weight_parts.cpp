#include "weight_parts.h"

namespace lavie {

void ParamTable::add(const std::string& name, long long numel, bool required) {
    index_[name] = (int)params_.size();
    params_.push_back({name, numel, nullptr, required});
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
    for (const Param& p : params_) LAVIE_CHECK(p.src != nullptr || !p.required, "%s: '%s' was never set", who, p.name.c_str());
    return 0;
}

const ParamTable::Param* ParamTable::find(const std::string& name) const {
    auto it = index_.find(name);
    return it == index_.end() ? nullptr : &params_[it->second];
}

void ParamTable::release() {
    for (Param& p : params_) p.src = nullptr;      // the loan ends when the stream drains
}

int copy16(half_t* dst, const half_t* src, size_t n, hipStream_t s) {
    LAVIE_HIP(hipMemcpyAsync(dst, src, n * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace lavie
