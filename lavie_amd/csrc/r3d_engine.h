// The video ResNet behind lavie_r3d_* (DESIGN.md 7.20): R3D-18 (Tran et al., "A Closer Look at Spatiotemporal Convolutions for Action
// Recognition", 2018) without its classifier, on the kernels of conv3d.hip.  Same lifecycle as the encoders (encoder_parts.h); the
// parameters are fp32, because the BatchNorm fold wants the unrounded statistics.
#pragma once
#include "encoder_parts.h"

namespace lavie {

constexpr int kR3dFeatures = 512;

class R3dEngine {
public:
    R3dEngine();

    const std::vector<ParamTable::Param>& params() const { return table_.params(); }
    int set_param(const char* name, const void* data_f32, long long numel);
    int finalize(hipStream_t s);
    // bytes of the caller's workspace features(N, T, H, W) uses; -1 with a message for a shape it refuses
    long long workspace_bytes(int N, int T, int H, int W) const;
    int features(const void* pixels, int x_dtype, long long stride_n, long long stride_t, long long stride_c, int N, int T, int H, int W,
                 float* out, void* workspace, long long workspace_bytes, hipStream_t s);

private:
    struct Conv {
        std::string name;        // "layer2.0.conv1", "layer2.0.downsample", "stem"
        int cin, cout, ksize, stride;
        half_t* w = nullptr;
        float* b = nullptr;
    };
    struct Block {
        Conv conv1, conv2, down;
        bool has_down;
    };
    void list(const Conv& c, int kt, int kh, int kw);
    ParamTable table_;
    WeightBlock block_;
    Conv stem_;
    std::vector<Block> blocks_;
};

}  // namespace lavie
