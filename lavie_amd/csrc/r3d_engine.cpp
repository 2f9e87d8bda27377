// R3D-18 features: stem (3,7,7) conv - BN - ReLU; layer1 .. layer4, each two basic blocks
//   t = relu(bn1(conv1(x)));  r = x, or bn_d(conv_d(x)) for the (1,1,1) stride-2 downsample of the first block of layers 2 - 4;
//   x = relu(bn2(conv2(t)) + r)
// with (3,3,3) pad-1 convs, stride 2 on conv1 of those first blocks, widths 64, 128, 256, 512; then the mean over all positions.
// Every BatchNorm (inference form, eps 1e-5) is folded into its conv at finalize: scale = gamma / sqrt(var + eps) in double, the
// weight times the scale rounded ONCE to fp16, the shift beta - mean scale kept as the fp32 bias of the conv's epilogue.
// Roundings of a forward: every tensor between two launches is fp16 (one rounding per conv, after bias, residual and ReLU were
// applied in fp32); the downsample is its own launch, so the shortcut of those three blocks is rounded to fp16 before conv2's
// epilogue adds it; the features are fp32.  Every launch works output row by output row in a fixed order: a clip's features have
// the same bits at every batch size and position.
#include "r3d_engine.h"

#include "ops.h"

namespace lavie {

namespace {

constexpr double kBnEps = 1e-5;
const char* const kBnParts[4] = {"weight", "bias", "running_mean", "running_var"};

struct Shapes {
    size_t main_halfs, down_halfs;      // the largest activation tensor and the largest downsample output
};

// walks the extents through the network; 0 or the refusal of the first launch that would refuse
int walk(const char* who, int N, int T, int H, int W, Shapes* out) {
    LAVIE_CHECK(N >= 1 && N <= 65535, "%s: N=%d must be in 1..65535", who, N);
    LAVIE_CHECK(T >= 1 && H >= 1 && W >= 1, "%s: extents T=%d H=%d W=%d must be at least 1", who, T, H, W);
    LAVIE_CHECK((long long)N * T * H * W <= (1ll << 30), "%s: N T H W = %lld pixels per channel exceed 2^30", who, (long long)N * T * H * W);
    int t, h, w;
    RUN(conv3d_stem_out_shape(T, H, W, &t, &h, &w));
    size_t main_halfs = (size_t)N * t * h * w * 64, down_halfs = 0;
    for (int level = 1; level < 4; ++level) {
        RUN(conv3d_out_shape(t, h, w, 3, 2, &t, &h, &w));
        const size_t halfs = (size_t)N * t * h * w * (64 << level);
        if (halfs > main_halfs) main_halfs = halfs;
        if (halfs > down_halfs) down_halfs = halfs;
    }
    out->main_halfs = main_halfs;
    out->down_halfs = down_halfs;
    return 0;
}

}  // namespace

void R3dEngine::list(const Conv& c, int kt, int kh, int kw) {
    table_.add(c.name + ".0.weight", (long long)c.cout * c.cin * kt * kh * kw);
    for (const char* part : kBnParts) table_.add(c.name + ".1." + part, c.cout);
    table_.ignore(c.name + ".1.num_batches_tracked");
}

R3dEngine::R3dEngine() {
    stem_ = Conv{"stem", 3, 64, 0, 0};
    list(stem_, 3, 7, 7);
    int cin = 64;
    for (int level = 0; level < 4; ++level) {
        const int cout = 64 << level;
        for (int b = 0; b < 2; ++b) {
            const std::string p = "layer" + std::to_string(level + 1) + "." + std::to_string(b) + ".";
            Block blk;
            const int stride = (level > 0 && b == 0) ? 2 : 1;
            blk.conv1 = Conv{p + "conv1", cin, cout, 3, stride};
            blk.conv2 = Conv{p + "conv2", cout, cout, 3, 1};
            blk.has_down = stride == 2;
            list(blk.conv1, 3, 3, 3);
            list(blk.conv2, 3, 3, 3);
            if (blk.has_down) {
                blk.down = Conv{p + "downsample", cin, cout, 1, 2};
                list(blk.down, 1, 1, 1);
            }
            blocks_.push_back(blk);
            cin = cout;
        }
    }
    table_.ignore("fc.weight");
    table_.ignore("fc.bias");
}

// accepts the module's own names and the numeric prefixes of nn.Sequential(*children[:-1]): "0." = stem, "1." .. "4." = layer1 .. layer4
int R3dEngine::set_param(const char* name, const void* data_f32, long long numel) {
    RUN(check_open(block_, "r3d_set_param"));
    std::string key = name;
    if (key.size() >= 2 && key[1] == '.' && key[0] >= '0' && key[0] <= '4')
        key = (key[0] == '0' ? std::string("stem") : "layer" + key.substr(0, 1)) + key.substr(1);
    return table_.set("r3d_set_param", "", key.c_str(), data_f32, numel);
}

int R3dEngine::finalize(hipStream_t s) {
    RUN(check_open(block_, "r3d_finalize", " already"));
    RUN(table_.all_set("r3d_finalize"));
    std::vector<Conv*> convs = {&stem_};
    for (Block& b : blocks_) {
        convs.push_back(&b.conv1);
        convs.push_back(&b.conv2);
        if (b.has_down) convs.push_back(&b.down);
    }
    auto taps = [](const Conv& c, int* kt, int* kh, int* kw) {
        if (c.ksize == 0) { *kt = 3; *kh = 7; *kw = 7; }
        else { *kt = *kh = *kw = c.ksize; }
    };
    RUN(allocate(block_, 0, [&](char* base) {
        Carver c{base};
        for (Conv* cv : convs) {
            int kt, kh, kw;
            taps(*cv, &kt, &kh, &kw);
            cv->w = c.take<half_t>((size_t)conv3d_packed_halfs(cv->cout, cv->cin, kt, kh, kw));
            cv->b = c.take<float>((size_t)cv->cout);
        }
        return c.used;
    }));
    for (Conv* cv : convs) {
        int kt, kh, kw;
        taps(*cv, &kt, &kh, &kw);
        auto f32 = [&](const std::string& n) { return reinterpret_cast<const float*>(table_.src(cv->name + n)); };      // the table keeps addresses
        RUN(launch_conv3d_fold_pack(f32(".0.weight"), f32(".1.weight"), f32(".1.bias"), f32(".1.running_mean"), f32(".1.running_var"), kBnEps,
                                    cv->w, cv->b, cv->cout, cv->cin, kt, kh, kw, s));
    }
    table_.release();
    block_.finalized = true;
    return 0;
}

// x | t, each the largest activation tensor, then the downsample output
long long R3dEngine::workspace_bytes(int N, int T, int H, int W) const {
    Shapes sh;
    if (walk("r3d_workspace_bytes", N, T, H, W, &sh)) return -1;
    return (long long)(2 * up256(sh.main_halfs * sizeof(half_t)) + up256(sh.down_halfs * sizeof(half_t)));
}

int R3dEngine::features(const void* pixels, int x_dtype, long long stride_n, long long stride_t, long long stride_c, int N, int T, int H,
                        int W, float* out, void* workspace, long long ws_bytes, hipStream_t s) {
    const char* who = "r3d_features";
    LAVIE_CHECK(block_.finalized, "%s: the handle is not finalized", who);
    LAVIE_CHECK(pixels != nullptr, "%s: pixels is null", who);
    LAVIE_CHECK(out != nullptr, "%s: out_f32 is null", who);
    LAVIE_CHECK(x_dtype == 0 || x_dtype == 1, "%s: x_dtype=%d (0 = fp16, 1 = fp32)", who, x_dtype);
    Shapes sh;
    RUN(walk(who, N, T, H, W, &sh));
    const long long need = (long long)(2 * up256(sh.main_halfs * sizeof(half_t)) + up256(sh.down_halfs * sizeof(half_t)));
    LAVIE_CHECK(workspace != nullptr && ws_bytes >= need, "%s: the workspace holds %lld bytes, this call needs %lld", who,
                workspace ? ws_bytes : 0ll, need);
    Carver c{(char*)workspace};
    half_t* x = c.take<half_t>(sh.main_halfs);
    half_t* t = c.take<half_t>(sh.main_halfs);
    half_t* d = c.take<half_t>(sh.down_halfs);
    int ct, chh, cw;
    RUN(conv3d_stem_out_shape(T, H, W, &ct, &chh, &cw));
    RUN(launch_conv3d_stem(pixels, x_dtype == 1, stride_n, stride_t, stride_c, stem_.w, stem_.b, true, x, N, T, H, W, s));
    for (const Block& b : blocks_) {
        int ot, oh, ow;
        RUN(conv3d_out_shape(ct, chh, cw, 3, b.conv1.stride, &ot, &oh, &ow));
        RUN(launch_conv3d(x, b.conv1.w, b.conv1.b, nullptr, true, t, N, ct, chh, cw, b.conv1.cin, b.conv1.cout, 3, b.conv1.stride, s));
        const half_t* res = x;
        if (b.has_down) {
            RUN(launch_conv3d(x, b.down.w, b.down.b, nullptr, false, d, N, ct, chh, cw, b.down.cin, b.down.cout, 1, 2, s));
            res = d;
        }
        // the block's output replaces x: an element's residual is read by the lane that then writes it
        RUN(launch_conv3d(t, b.conv2.w, b.conv2.b, res, true, x, N, ot, oh, ow, b.conv2.cin, b.conv2.cout, 3, 1, s));
        ct = ot; chh = oh; cw = ow;
    }
    return launch_mean_rows(x, out, N, ct * chh * cw, kR3dFeatures, s);
}

}  // namespace lavie
