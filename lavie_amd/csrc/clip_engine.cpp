// Host side of the CLIP image processor: the output geometry of transformers' shortest-edge resize and centre crop,
// the refusals, Pillow's resampling coefficients in double -> int32, the 768-entry normalisation table, and a cache of the uploaded
// tables keyed by (device, H, W, size, crop, mean, std).  The kernels are in clip_preprocess.hip.
//
// One axis, `in` source samples to `out` (ImagingResample's precompute_coeffs and normalize_coeffs_8bpc, bicubic, a = -0.5):
//   scale = in / out; fs = max(scale, 1); support = 2 fs; ksize = 2 ceil(support) + 1
//   output xx: center = (xx + 0.5) scale; xmin = max(int(center - support + 0.5), 0); xmax = min(int(center + support + 0.5), in)
//   w_x = bicubic((x + xmin - center + 0.5) / fs) for x in [0, xmax - xmin); summed in index order; each divided by the sum
//   k_x = int(w_x 2^22 + 0.5) for w_x >= 0, int(w_x 2^22 - 0.5) below; int() truncates
// Everything is double arithmetic written operation by operation; contraction into fused multiply-adds is switched off so that the
// integers are those of the NumPy model (tests/clip_reference.py) on every host.
#include <math.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "ops.h"

#pragma clang fp contract(off)

namespace lavie {

namespace {

double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's bilinear (triangle) filter, support 1.0: the video processor's resize
double bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

struct Filter {
    double (*fn)(double);
    double support;
};
const Filter kBicubic = {bicubic, 2.0}, kBilinear = {bilinear, 1.0};

int axis_ksize(int in, int out, const Filter& f = kBicubic) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(f.support * fs) * 2 + 1;
}

// outputs [first, first + n) of the axis: xmin[n], cnt[n], coeff[n, ksize] (zero behind the taps)
void axis_table(int in, int out, int first, int n, int* xmin_out, int* cnt_out, int* coeff_out, const Filter& f = kBicubic) {
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = f.support * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<double> w((size_t)ksize);
    for (int i = 0; i < n; ++i) {
        const int xx = first + i;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int cnt = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            w[x] = f.fn((x + xmin - center + 0.5) / fs);
            ww += w[x];
        }
        int* k = coeff_out + (size_t)i * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < cnt) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << 22)) : (int)(0.5 + v * (double)(1 << 22));
        }
        xmin_out[i] = xmin;
        cnt_out[i] = cnt;
    }
}

struct Geometry {
    int out_h, out_w;        // the resized image
    int y0, x0;              // first kept row / column of it
    int ks_h, ks_v;          // taps per output of the horizontal (over W) and the vertical (over H) pass
    int row0, rows;          // source rows the kept output rows read
};

// transformers' get_resize_output_image_size (shortest edge, default_to_square = False) and center_crop; every refusal by name
int geometry(const char* who, int H, int W, int size, int crop, Geometry* g) {
    LAVIE_CHECK(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: H=%d W=%d must be in 1..65535", who, H, W);
    const int shorter = H < W ? H : W, longer = H < W ? W : H;
    LAVIE_CHECK(shorter >= 8, "%s: short edge %d is below 8", who, shorter);
    LAVIE_CHECK(size >= 1 && size <= 16384, "%s: size=%d must be in 1..16384", who, size);
    LAVIE_CHECK(crop >= 1, "%s: crop=%d must be at least 1", who, crop);
    const int new_long = (int)((double)((long long)size * longer) / (double)shorter);
    if (W <= H) { g->out_w = size; g->out_h = new_long; }      // transformers: the short edge is W when W <= H
    else { g->out_h = size; g->out_w = new_long; }
    const double sh = (double)H / g->out_h, sw = (double)W / g->out_w;
    LAVIE_CHECK(sh <= 32.0 && sw <= 32.0, "%s: scale %.3f is above 32 (H=%d W=%d to size=%d)", who, sh > sw ? sh : sw, H, W, size);
    const int edge = g->out_h < g->out_w ? g->out_h : g->out_w;
    LAVIE_CHECK(crop <= edge, "%s: crop=%d is greater than the resized edge %d (the stock processor pads there: not built)", who, crop, edge);
    g->y0 = (g->out_h - crop) / 2;
    g->x0 = (g->out_w - crop) / 2;
    g->ks_h = axis_ksize(W, g->out_w);
    g->ks_v = axis_ksize(H, g->out_h);
    // first tap of the first kept row, end of the last kept row's taps (both monotone in the output index)
    const double support = 2.0 * (sh < 1.0 ? 1.0 : sh);
    int lo = (int)((g->y0 + 0.5) * sh - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)((g->y0 + crop - 1 + 0.5) * sh + support + 0.5);
    if (hi > H) hi = H;
    g->row0 = lo;
    g->rows = hi - lo;
    return 0;
}

struct PlanKey {
    int device, H, W, size, crop, mode;      // mode 0: the CLIP processor (resize, then crop); 1: the video processor (crop, then resize)
    float ms[6];
    bool operator<(const PlanKey& o) const { return memcmp(this, &o, sizeof(PlanKey)) < 0; }
};

// The uploaded tables of one key.  Held by shared_ptr: the cache owns one reference and every call in progress another, so an entry
// dropped from the cache lives until the last call that looked it up has enqueued its launches; the destructor then drains the
// tables' device before it frees them.
struct Plan {
    Geometry g;
    int device = 0;
    int* dev = nullptr;          // one allocation: hx | hc | hk | vy | vc | vk | lut
    const int *hx = nullptr, *hc = nullptr, *hk = nullptr, *vy = nullptr, *vc = nullptr, *vk = nullptr;
    const float* lut = nullptr;
    Plan() = default;
    Plan(const Plan&) = delete;
    Plan& operator=(const Plan&) = delete;
    ~Plan() {
        if (!dev) return;
        int cur = 0;
        const bool swap = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
        (void)hipDeviceSynchronize();          // a launch that reads the tables may still be in flight
        (void)hipFree(dev);
        if (swap) (void)hipSetDevice(cur);
    }
};

std::mutex g_mutex;
// never destroyed: the tables stay valid (and reachable) until the process ends, whatever order the runtime is torn down in
std::map<PlanKey, std::shared_ptr<const Plan>>& g_plans = *new std::map<PlanKey, std::shared_ptr<const Plan>>();
constexpr size_t kMaxPlans = 64;

// g: the geometry of (H, W, size, crop), already validated by the caller.  nout = outputs per axis (the tables' length);
// fill(hx, hc, hk, vy, vc, vk) writes the two axes' tables in source coordinates.
template <class Fill>
int get_plan(const char* who, int mode, const Geometry& g, int nout, int H, int W, int size, int crop, const float* mean, const float* std_,
             Fill&& fill, std::shared_ptr<const Plan>* out) {
    PlanKey key;
    memset(&key, 0, sizeof(key));
    LAVIE_HIP(hipGetDevice(&key.device));
    key.H = H; key.W = W; key.size = size; key.crop = crop; key.mode = mode;
    for (int c = 0; c < 3; ++c) { key.ms[c] = mean[c]; key.ms[3 + c] = std_[c]; }
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_plans.find(key);
    if (it != g_plans.end()) {
        *out = it->second;
        return 0;
    }
    const size_t n_h = (size_t)nout * g.ks_h, n_v = (size_t)nout * g.ks_v;
    std::vector<int> host(4 * (size_t)nout + n_h + n_v + 768);
    int* hx = host.data();
    int* hc = hx + nout;
    int* hk = hc + nout;
    int* vy = hk + n_h;
    int* vc = vy + nout;
    int* vk = vc + nout;
    float lut[768];
    fill(hx, hc, hk, vy, vc, vk);
    for (int i = 0; i < nout; ++i) {
        LAVIE_CHECK(hx[i] >= 0 && hc[i] >= 1 && hx[i] + hc[i] <= W && hc[i] <= g.ks_h, "%s: internal: column taps [%d, +%d) leave [0, %d)", who,
                    hx[i], hc[i], W);
        LAVIE_CHECK(vy[i] >= g.row0 && vc[i] >= 1 && vy[i] + vc[i] <= g.row0 + g.rows && vc[i] <= g.ks_v,
                    "%s: internal: row taps [%d, +%d) leave [%d, +%d)", who, vy[i], vc[i], g.row0, g.rows);
        vy[i] -= g.row0;
    }
    for (int c = 0; c < 3; ++c)
        for (int u = 0; u < 256; ++u) {               // (u / 255 - mean) / std in fp32 with true divisions: the stock bits
            const float scaled = (float)u / 255.0f;
            const float centred = scaled - mean[c];
            lut[c * 256 + u] = centred / std_[c];
        }
    memcpy(vk + n_v, lut, sizeof lut);
    if (g_plans.size() >= kMaxPlans) g_plans.clear();  // the dropped entries free themselves once no call holds them (~Plan)
    auto p = std::make_shared<Plan>();
    p->g = g;
    p->device = key.device;
    LAVIE_HIP(hipMalloc((void**)&p->dev, host.size() * sizeof(int)));
    if (hipError_t e = hipMemcpy(p->dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice)) {
        set_error("%s: uploading the tables failed: %s", who, hipGetErrorString(e));
        return -2;
    }
    p->hx = p->dev; p->hc = p->hx + nout; p->hk = p->hc + nout; p->vy = p->hk + n_h; p->vc = p->vy + nout; p->vk = p->vc + nout;
    p->lut = reinterpret_cast<const float*>(p->vk + n_v);
    g_plans.emplace(key, p);
    *out = p;
    return 0;
}

// Python's round() of diff / 2 (half to even), as torchvision's CenterCrop computes its offsets
int centre_offset(int diff) { return (diff & 1) ? ((diff >> 1) + ((diff >> 1) & 1)) : diff >> 1; }

// the video processor: rows [y0, y0 + crop) x columns [x0, x0 + crop) of the frame, resized to size x size by the bilinear filter
int video_geometry(const char* who, int H, int W, int crop, int size, Geometry* g) {
    LAVIE_CHECK(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: H=%d W=%d must be in 1..65535", who, H, W);
    LAVIE_CHECK(size >= 1 && size <= 16384, "%s: size=%d must be in 1..16384", who, size);
    LAVIE_CHECK(crop >= 1, "%s: crop=%d must be at least 1", who, crop);
    LAVIE_CHECK(crop <= H && crop <= W, "%s: crop=%d is greater than the frame %d x %d (the stock transform pads there: not built)", who, crop,
                H, W);
    LAVIE_CHECK((double)crop / size <= 32.0, "%s: scale %.3f is above 32 (crop=%d to size=%d)", who, (double)crop / size, crop, size);
    g->out_h = g->out_w = size;
    g->y0 = centre_offset(H - crop);
    g->x0 = centre_offset(W - crop);
    g->ks_h = g->ks_v = axis_ksize(crop, size, kBilinear);
    g->row0 = g->y0;              // the horizontal pass runs over every row of the crop
    g->rows = crop;
    return 0;
}
size_t mid_bytes(int B, const Geometry& g, int crop) { return ((size_t)B * g.rows * crop * 3 + 255) / 256 * 256; }

}  // namespace

int clip_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out) {
    const char* who = "clip_resample_table_host";
    LAVIE_CHECK(in >= 1 && in <= 65535 && out >= 1 && out <= 65535, "%s: in=%d out=%d must be in 1..65535", who, in, out);
    LAVIE_CHECK((double)in / (double)out <= 32.0, "%s: scale %.3f is above 32", who, (double)in / (double)out);
    const int ksize = axis_ksize(in, out);
    if (xmin_out == nullptr && count_out == nullptr && coeff_out == nullptr) return ksize;       // the size query
    LAVIE_CHECK(xmin_out && count_out && coeff_out, "%s: xmin_out, count_out and coeff_out are all given or all null", who);
    axis_table(in, out, 0, out, xmin_out, count_out, coeff_out);
    return ksize;
}

long long clip_preprocess_workspace_bytes(int B, int H, int W, int size, int crop) {
    const char* who = "clip_preprocess_workspace_bytes";
    Geometry g;
    if (B < 1 || B > 65535) {
        set_error("%s: B=%d must be in 1..65535", who, B);
        return -1;
    }
    if (geometry(who, H, W, size, crop, &g)) return -1;
    return (long long)mid_bytes(B, g, crop);
}

int clip_preprocess(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype, int size,
                    int crop, const float* mean, const float* std_, void* workspace, long long workspace_bytes, hipStream_t stream) {
    const char* who = "clip_preprocess";
    LAVIE_CHECK(in_u8 && out, "%s: null tensor", who);
    LAVIE_CHECK(B >= 1 && B <= 65535, "%s: B=%d must be in 1..65535", who, B);
    LAVIE_CHECK(out_dtype == 0 || out_dtype == 1, "%s: out_dtype=%d (0 = fp16, 1 = fp32)", who, out_dtype);
    LAVIE_CHECK(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: H=%d W=%d must be in 1..65535", who, H, W);
    LAVIE_CHECK(row_pitch >= 3ll * W, "%s: row_pitch=%lld is below 3 W = %d", who, row_pitch, 3 * W);
    LAVIE_CHECK(B == 1 || image_pitch >= (long long)(H - 1) * row_pitch + 3ll * W,
                "%s: image_pitch=%lld is below the %lld bytes of one image", who, image_pitch, (long long)(H - 1) * row_pitch + 3ll * W);
    for (int c = 0; c < 3; ++c)
        LAVIE_CHECK(isfinite(mean[c]) && isfinite(std_[c]) && std_[c] != 0.f, "%s: mean[%d]=%g std[%d]=%g must be finite, std not 0", who, c,
                    mean[c], c, std_[c]);
    LAVIE_CHECK(((uintptr_t)out & (out_dtype == 1 ? 3 : 1)) == 0, "%s: out is not aligned to its element size", who);
    Geometry g;
    if (int rc = geometry(who, H, W, size, crop, &g)) return rc;
    const long long need = (long long)mid_bytes(B, g, crop);
    LAVIE_CHECK(workspace != nullptr && workspace_bytes >= need, "%s: the workspace holds %lld bytes, this call needs %lld", who,
                workspace ? workspace_bytes : 0ll, need);
    std::shared_ptr<const Plan> p;                     // every refusal is behind us: only now is the device touched
    auto fill = [&](int* hx, int* hc, int* hk, int* vy, int* vc, int* vk) {
        axis_table(W, g.out_w, g.x0, crop, hx, hc, hk);
        axis_table(H, g.out_h, g.y0, crop, vy, vc, vk);
    };
    if (int rc = get_plan(who, 0, g, crop, H, W, size, crop, mean, std_, fill, &p)) return rc;
    uint8_t* mid = (uint8_t*)workspace;
    if (int rc = launch_clip_resample_h((const uint8_t*)in_u8, row_pitch, B == 1 ? 0 : image_pitch, mid, B, p->g.row0, p->g.rows, crop, p->hx, p->hc,
                                        p->hk, p->g.ks_h, stream))
        return rc;
    return launch_clip_resample_v(mid, out, out_dtype == 1, B, p->g.rows, crop, p->vy, p->vc, p->vk, p->g.ks_v, p->lut, stream);
}

// ---- the video processor: torchvision's CenterCrop(crop) then Resize(size) on a PIL image, per frame
int video_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out) {
    const char* who = "video_resample_table_host";
    LAVIE_CHECK(in >= 1 && in <= 65535 && out >= 1 && out <= 65535, "%s: in=%d out=%d must be in 1..65535", who, in, out);
    LAVIE_CHECK((double)in / (double)out <= 32.0, "%s: scale %.3f is above 32", who, (double)in / (double)out);
    const int ksize = axis_ksize(in, out, kBilinear);
    if (xmin_out == nullptr && count_out == nullptr && coeff_out == nullptr) return ksize;       // the size query
    LAVIE_CHECK(xmin_out && count_out && coeff_out, "%s: xmin_out, count_out and coeff_out are all given or all null", who);
    axis_table(in, out, 0, out, xmin_out, count_out, coeff_out, kBilinear);
    return ksize;
}

long long video_preprocess_workspace_bytes(int B, int H, int W, int crop, int size) {
    const char* who = "video_preprocess_workspace_bytes";
    Geometry g;
    if (B < 1 || B > 65535) {
        set_error("%s: B=%d must be in 1..65535", who, B);
        return -1;
    }
    if (video_geometry(who, H, W, crop, size, &g)) return -1;
    return (long long)mid_bytes(B, g, size);
}

int video_preprocess(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype, int crop,
                     int size, const float* mean, const float* std_, void* workspace, long long workspace_bytes, hipStream_t stream) {
    const char* who = "video_preprocess";
    LAVIE_CHECK(in_u8 && out, "%s: null tensor", who);
    LAVIE_CHECK(mean && std_, "%s: null mean or std", who);
    LAVIE_CHECK(B >= 1 && B <= 65535, "%s: B=%d must be in 1..65535", who, B);
    LAVIE_CHECK(out_dtype == 0 || out_dtype == 1, "%s: out_dtype=%d (0 = fp16, 1 = fp32)", who, out_dtype);
    LAVIE_CHECK(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: H=%d W=%d must be in 1..65535", who, H, W);
    LAVIE_CHECK(row_pitch >= 3ll * W, "%s: row_pitch=%lld is below 3 W = %d", who, row_pitch, 3 * W);
    LAVIE_CHECK(B == 1 || image_pitch >= (long long)(H - 1) * row_pitch + 3ll * W,
                "%s: image_pitch=%lld is below the %lld bytes of one image", who, image_pitch, (long long)(H - 1) * row_pitch + 3ll * W);
    for (int c = 0; c < 3; ++c)
        LAVIE_CHECK(isfinite(mean[c]) && isfinite(std_[c]) && std_[c] != 0.f, "%s: mean[%d]=%g std[%d]=%g must be finite, std not 0", who, c,
                    mean[c], c, std_[c]);
    LAVIE_CHECK(((uintptr_t)out & (out_dtype == 1 ? 3 : 1)) == 0, "%s: out is not aligned to its element size", who);
    Geometry g;
    if (int rc = video_geometry(who, H, W, crop, size, &g)) return rc;
    const long long need = (long long)mid_bytes(B, g, size);
    LAVIE_CHECK(workspace != nullptr && workspace_bytes >= need, "%s: the workspace holds %lld bytes, this call needs %lld", who,
                workspace ? workspace_bytes : 0ll, need);
    std::shared_ptr<const Plan> p;
    auto fill = [&](int* hx, int* hc, int* hk, int* vy, int* vc, int* vk) {      // the cropped square's tables, moved to frame coordinates
        axis_table(crop, size, 0, size, hx, hc, hk, kBilinear);
        axis_table(crop, size, 0, size, vy, vc, vk, kBilinear);
        for (int i = 0; i < size; ++i) { hx[i] += g.x0; vy[i] += g.y0; }
    };
    if (int rc = get_plan(who, 1, g, size, H, W, size, crop, mean, std_, fill, &p)) return rc;
    uint8_t* mid = (uint8_t*)workspace;
    if (int rc = launch_clip_resample_h((const uint8_t*)in_u8, row_pitch, B == 1 ? 0 : image_pitch, mid, B, p->g.row0, p->g.rows, size, p->hx,
                                        p->hc, p->hk, p->g.ks_h, stream))
        return rc;
    return launch_clip_resample_v(mid, out, out_dtype == 1, B, p->g.rows, size, p->vy, p->vc, p->vk, p->g.ks_v, p->lut, stream);
}

}  // namespace lavie
