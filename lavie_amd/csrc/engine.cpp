// UNet3DConditionModel.forward on a HIP stream: weight packing, workspace planning, kernel sequencing.
// Mirrors the wiring of /root/reference/base/models/unet.py:454-506 and unet_blocks.py
// (226-232, 320-362, 417-441, 524-574, 625-648) on channels-last activations; see DESIGN.md.
#include "engine.h"
#include "profile.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace lavie {

// ------------------------------------------------------------------ error text
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

static unsigned long g_debug_epoch = 0;
static int g_fused_mask = 0x137;        // bit 0: fused feed-forward, 1: fused temporal sub-block, 2: fused text cross-attention, 4: parity form of the upsample convs, 5: GroupNorm statistics from the producers' epilogues (A/B switches); 6: debug verification of those statistics against the statistics pass (off); 8: GroupNorm -> proj_in -> norm1 -> q|k|v as one row-resident kernel
void set_fused_mask(int m) { g_fused_mask = m; }
int fused_mask() { return g_fused_mask; }
void bump_debug_epoch() { ++g_debug_epoch; }
static bool debug_check_shared() {
    const char* e = getenv("LAVIE_DEBUG_CHECK_SHARED");
    return e && e[0] == '1';
}
unsigned long debug_epoch() { return g_debug_epoch; }

int ensure_dynamic_lds(const void* kernel, int bytes) {
    static std::vector<std::pair<const void*, int>> seen;      // a handful of entries; one host thread per process drives the GPU
    for (const auto& e : seen)
        if (e.first == kernel && e.second >= bytes) return 0;
    LAVIE_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    seen.emplace_back(kernel, bytes);
    return 0;
}

// ------------------------------------------------------------------ arena
DeviceArena::~DeviceArena() { free_all(); }

void DeviceArena::free_all() {
    for (void* p : chunks_) (void)hipFree(p);
    chunks_.clear();
    cur_ = nullptr;
    cap_ = off_ = peak_ = total_ = 0;
}

int DeviceArena::init_fixed(size_t bytes) {
    free_all();
    fixed_ = true;
    void* p = nullptr;
    LAVIE_HIP(hipMalloc(&p, bytes));
    chunks_.push_back(p);
    cur_ = (char*)p;
    cap_ = bytes;
    total_ = bytes;
    return 0;
}

void* DeviceArena::alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (virtual_) {
        off_ += bytes;
        if (off_ > peak_) peak_ = off_;
        return (void*)(uintptr_t)256;   // never dereferenced
    }
    if (off_ + bytes > cap_) {
        if (fixed_) return nullptr;
        const size_t sz = bytes > kChunk ? bytes : kChunk;
        void* p = nullptr;
        if (hipMalloc(&p, sz) != hipSuccess) return nullptr;
        chunks_.push_back(p);
        cur_ = (char*)p;
        cap_ = sz;
        off_ = 0;
        total_ += sz;
    }
    void* r = cur_ + off_;
    off_ += bytes;
    if (off_ > peak_) peak_ = off_;
    return r;
}

// ------------------------------------------------------------------ model structure
UNet::UNet(const lavie_unet_config& cfg) : cfg_(cfg) { build_param_list(); }
UNet::~UNet() {
    drop_graph();
    if (cap_stream_) (void)hipStreamDestroy(cap_stream_);
    if (kv_block_) (void)hipFree(kv_block_);
    if (xbl_block_) (void)hipFree(xbl_block_);
    if (lc_block_) (void)hipFree(lc_block_);
    for (auto& kv : lora_) {
        for (LoraSlot& s : kv.second.slot) lora_free(s);
        if (kv.second.base) (void)hipFree(kv.second.base);
    }
}

int UNet::validate_config() {
    const lavie_unet_config& c = cfg_;
    LAVIE_CHECK(c.num_levels >= 1 && c.num_levels <= LAVIE_MAX_LEVELS, "config: num_levels=%d", c.num_levels);
    LAVIE_CHECK(c.in_channels >= 1 && c.in_channels <= 16 && c.out_channels >= 1 && c.out_channels <= 8,
                "config: in/out channels %d/%d unsupported", c.in_channels, c.out_channels);
    LAVIE_CHECK(c.heads >= 1 && c.layers_per_block >= 1 && c.norm_groups >= 1, "config: heads/layers/groups");
    LAVIE_CHECK(c.cross_attention_dim % 64 == 0, "config: cross_attention_dim %d must be a multiple of 64", c.cross_attention_dim);
    for (int l = 0; l < c.num_levels; ++l) {
        const int w = c.block_out_channels[l];
        LAVIE_CHECK(w % 64 == 0 && w % c.norm_groups == 0, "config: width %d must be a multiple of 64 and of norm_groups", w);
        if (c.attn_levels[l]) {
            const int min_dh = c.temporal_plain ? 8 : c.rotary_dim;
            LAVIE_CHECK(w % c.heads == 0 && (w / c.heads) % 8 == 0 && w / c.heads >= min_dh && w / c.heads <= 160,
                        "config: width %d gives head dim %d (need multiple of 8, %d..160)", w, w / c.heads, min_dh);
        }
    }
    LAVIE_CHECK(c.rotary_dim == 32 || c.rotary_dim == 16 || c.rotary_dim == 8, "config: rotary_dim %d", c.rotary_dim);
    LAVIE_CHECK(c.in_channels % 2 == 0, "config: in_channels %d must be even (conv_in packs channel pairs)", c.in_channels);
    return 0;
}

void UNet::build_param_list() {
    const lavie_unet_config& c = cfg_;
    auto add = [&](const std::string& name, long long numel) { table_.add(name, numel); };
    auto affine = [&](const std::string& p, int ch) { add(p + ".weight", ch); add(p + ".bias", ch); };
    auto conv = [&](const std::string& p, long long cin, long long cout, int k) { add(p + ".weight", cout * cin * k * k); add(p + ".bias", cout); };
    auto lin = [&](const std::string& p, long long cin, long long cout, bool bias) { add(p + ".weight", cout * cin); if (bias) add(p + ".bias", cout); };
    const int temb = c.block_out_channels[0] * 4;
    int temb_total = 0;
    auto resnet = [&](const std::string& p, int cin, int cout) {
        affine(p + ".norm1", cin);
        conv(p + ".conv1", cin, cout, 3);
        lin(p + ".time_emb_proj", temb, cout, true);
        affine(p + ".norm2", cout);
        conv(p + ".conv2", cout, cout, 3);
        if (cin != cout) conv(p + ".conv_shortcut", cin, cout, 1);
        ResnetW r;
        r.prefix = p; r.cin = cin; r.cout = cout; r.shortcut = cin != cout; r.temb_off = temb_total;
        temb_total += cout;
        resnets_.push_back(r);
    };
    auto attention = [&](const std::string& p, int ch, int kv) {
        lin(p + ".to_q", ch, ch, false); lin(p + ".to_k", kv, ch, false); lin(p + ".to_v", kv, ch, false);
        lin(p + ".to_out.0", ch, ch, true);
    };
    auto conv_t = [&](const std::string& p, long long cin, long long cout, int taps) { add(p + ".weight", cout * cin * taps); add(p + ".bias", cout); };
    auto transformer = [&](const std::string& p, int ch, int level) {
        const bool vsr = c.vsr_blocks != 0;
        const bool cross1 = vsr && level >= 0 && c.only_cross_attention[level] != 0;
        const std::string tname = vsr ? "temporal" : "temp";          // attn_temporal / norm_temporal in the VSR model
        if (vsr) {                                                     // resblock_temporal: ResnetBlock3DCNN (3,1,1), no temb
            affine(p + ".resblock_temporal.norm1", ch);
            conv_t(p + ".resblock_temporal.conv1", ch, ch, 3);
            affine(p + ".resblock_temporal.norm2", ch);
            conv_t(p + ".resblock_temporal.conv2", ch, ch, 3);
        }
        affine(p + ".norm", ch);
        if (vsr) lin(p + ".proj_in", ch, ch, true); else conv(p + ".proj_in", ch, ch, 1);
        const std::string b = p + ".transformer_blocks.0";
        attention(b + ".attn1", ch, cross1 ? c.cross_attention_dim : ch);
        affine(b + ".norm1", ch);
        attention(b + ".attn2", ch, c.cross_attention_dim);
        affine(b + ".norm2", ch);
        attention(b + ".attn_" + tname, ch, ch);
        if (!c.temporal_plain) {
            add(b + ".attn_" + tname + ".time_rel_pos_bias.relative_attention_bias.weight", (long long)c.rel_buckets * c.heads);
            // listed so that the loader sends it, never read: angles are always derived in fp32 from rotary_dim (SURVEY.md §8c
            // decision; an fp16 copy of freqs would be lossy)
            table_.add(b + ".attn_" + tname + ".rotary_emb.freqs", c.rotary_dim / 2, /*required=*/false);
        }
        affine(b + ".norm_" + tname, ch);
        lin(b + ".ff.net.0.proj", ch, 8 * ch, true);
        lin(b + ".ff.net.2", 4 * ch, ch, true);
        affine(b + ".norm3", ch);
        if (vsr) lin(p + ".proj_out", ch, ch, true); else conv(p + ".proj_out", ch, ch, 1);
        TransformerW t;
        t.prefix = p; t.C = ch;
        t.tres.present = vsr;
        t.attn1_cross = cross1;
        transformers_.push_back(t);
    };
    auto temporal_module = [&](const std::string& p, int ch) {
        TemporalModuleW m;
        m.prefix = p; m.C = ch;
        const std::string t = p + ".resblocks_3d_t", sp = p + ".resblocks_3d_s";
        affine(t + ".norm1", ch);
        conv_t(t + ".conv1", ch, ch, 5);
        lin(t + ".time_emb_proj", temb, ch, true);
        affine(t + ".norm2", ch);
        conv_t(t + ".conv2", ch, ch, 3);
        m.t_temb_off = temb_total;
        temb_total += ch;
        affine(sp + ".norm1", ch);
        conv(sp + ".conv1", ch, ch, 3);
        lin(sp + ".time_emb_proj", temb, ch, true);
        affine(sp + ".norm2", ch);
        conv(sp + ".conv2", ch, ch, 3);
        m.s.prefix = sp; m.s.cin = ch; m.s.cout = ch; m.s.shortcut = false; m.s.temb_off = temb_total; m.s.eps = 1e-6f;
        temb_total += ch;
        conv(p + ".shift_conv", ch, ch, 1);
        tmods_.push_back(m);
    };
    const bool tmod = c.vsr_temporal_modules != 0;
    const int* widths = c.block_out_channels;
    const int L = c.num_levels;
    if (c.num_class_embeds > 0) add("class_embedding.weight", (long long)c.num_class_embeds * temb);
    if (c.vsr_blocks && !c.temporal_plain) table_.add("temporal_rotary_emb.freqs", c.rotary_dim / 2, /*required=*/false);   // as rotary_emb.freqs
    conv("conv_in", c.in_channels, widths[0], 3);
    lin("time_embedding.linear_1", widths[0], temb, true);
    lin("time_embedding.linear_2", temb, temb, true);
    std::vector<int> skips{widths[0]};
    int cur = widths[0];
    for (int l = 0; l < L; ++l) {
        for (int j = 0; j < c.layers_per_block; ++j) {
            const std::string p = "down_blocks." + std::to_string(l);
            resnet(p + ".resnets." + std::to_string(j), cur, widths[l]);
            cur = widths[l];
            if (c.attn_levels[l]) transformer(p + ".attentions." + std::to_string(j), cur, l);
            skips.push_back(cur);
        }
        if (l + 1 < L) {
            conv("down_blocks." + std::to_string(l) + ".downsamplers.0.conv", cur, cur, 3);
            skips.push_back(cur);
        }
        if (tmod) temporal_module("down_temporal_blocks." + std::to_string(l), cur);
    }
    resnet("mid_block.resnets.0", cur, cur);
    transformer("mid_block.attentions.0", cur, -1);      // the mid block always self-attends (vsr/models/unet.py:248-270)
    resnet("mid_block.resnets.1", cur, cur);
    if (tmod) temporal_module("mid_temporal_block", cur);
    for (int i = 0; i < L; ++i) {
        const int l = L - 1 - i;
        const std::string p = "up_blocks." + std::to_string(i);
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            const int sk = skips.back();
            skips.pop_back();
            resnet(p + ".resnets." + std::to_string(j), cur + sk, widths[l]);
            cur = widths[l];
            if (c.attn_levels[l]) transformer(p + ".attentions." + std::to_string(j), cur, l);
        }
        if (i + 1 < L) conv(p + ".upsamplers.0.conv", cur, cur, 3);
        if (tmod) temporal_module("up_temporal_blocks." + std::to_string(i), cur);
    }
    affine("conv_norm_out", widths[0]);
    conv("conv_out", widths[0], c.out_channels, 3);
    tproj_.N = temb_total;
    tproj_.K = temb;
}

// ------------------------------------------------------------------ weight packing
// finalize has checked that every required tensor is set, so table_.src() of a key cannot fail below: a key that is listed under a
// condition is looked up under the same condition
#define WALLOC(var, type, count)                                                                  \
    do {                                                                                          \
        (var) = (type*)weights_.alloc((size_t)(count) * sizeof(type));                            \
        LAVIE_CHECK((var) != nullptr, "finalize: out of device memory (%zu B; hip: %s)", (size_t)(count) * sizeof(type), hipGetErrorString(hipGetLastError())); \
    } while (0)

int UNet::pack_f32(const std::string& key, size_t n, float** out, hipStream_t s) {
    WALLOC(*out, float, n);
    return launch_f16_to_f32(table_.src(key), *out, (int64_t)n, s);
}

int UNet::pack_copy(const std::string& key, size_t n, half_t** out, hipStream_t s) {
    WALLOC(*out, half_t, n);
    return copy16(*out, table_.src(key), n, s);
}

int UNet::pack_norm(const std::string& prefix, int C, NormW* out, hipStream_t s) {
    out->C = C;
    RUN(pack_f32(prefix + ".weight", C, &out->g, s));
    return pack_f32(prefix + ".bias", C, &out->b, s);
}

int UNet::pack_linear(const std::string& prefix, int N, int K, bool bias, LinW* out, hipStream_t s) {
    out->N = N;
    out->K = K;
    out->b = nullptr;
    RUN(pack_copy(prefix + ".weight", (size_t)N * K, &out->w, s));
    return bias ? pack_f32(prefix + ".bias", N, &out->b, s) : 0;
}

int UNet::pack_resnet(ResnetW* r, hipStream_t s) {
    const std::string& p = r->prefix;
    RUN(pack_norm(p + ".norm1", r->cin, &r->n1, s));
    RUN(pack_norm(p + ".norm2", r->cout, &r->n2, s));
    WALLOC(r->w1, half_t, (size_t)r->cout * 9 * r->cin);
    RUN(launch_pack_conv3x3(table_.src(p + ".conv1.weight"), r->w1, r->cout, r->cin, 9 * r->cin, 0, true, s));
    RUN(pack_f32(p + ".conv1.bias", r->cout, &r->b1, s));
    r->ldw2 = 9 * r->cout + (r->shortcut ? r->cin : 0);
    WALLOC(r->w2, half_t, (size_t)r->cout * r->ldw2);
    RUN(launch_pack_conv3x3(table_.src(p + ".conv2.weight"), r->w2, r->cout, r->cout, r->ldw2, 0, true, s));
    if (r->shortcut) {
        WALLOC(r->b2, float, r->cout);
        RUN(launch_copy_rows(table_.src(p + ".conv_shortcut.weight"), r->cin, r->w2, r->ldw2, r->cout, r->cin, 9 * r->cout, s));
        RUN(launch_add_f16_to_f32(table_.src(p + ".conv2.bias"), table_.src(p + ".conv_shortcut.bias"), r->b2, r->cout, s));
    } else {
        RUN(pack_f32(p + ".conv2.bias", r->cout, &r->b2, s));
    }
    // fused time_emb_proj rows
    RUN(copy16(tproj_.w + (size_t)r->temb_off * tproj_.K, table_.src(p + ".time_emb_proj.weight"), (size_t)r->cout * tproj_.K, s));
    return launch_f16_to_f32(table_.src(p + ".time_emb_proj.bias"), tproj_.b + r->temb_off, r->cout, s);
}

int UNet::pack_transformer(TransformerW* t, hipStream_t s) {
    const std::string& p = t->prefix;
    const std::string b = p + ".transformer_blocks.0";
    const int C = t->C, X = cfg_.cross_attention_dim;
    RUN(pack_norm(p + ".norm", C, &t->gn, s));
    RUN(pack_linear(p + ".proj_in", C, C, true, &t->pin, s));      // [C, C, 1, 1] == [C, C]
    RUN(pack_linear(p + ".proj_out", C, C, true, &t->pout, s));
    RUN(pack_norm(b + ".norm1", C, &t->ln1, s));
    RUN(pack_norm(b + ".norm2", C, &t->ln2, s));
    const std::string tname = cfg_.vsr_blocks ? "temporal" : "temp";
    RUN(pack_norm(b + ".norm_" + tname, C, &t->lnt, s));
    if (t->tres.present) RUN(pack_temporal_res(p + ".resblock_temporal", C, 3, &t->tres, s));
    RUN(pack_norm(b + ".norm3", C, &t->ln3, s));
    auto fuse = [&](const std::string& a, const char* const* names, int count, int K, half_t** out) -> int {
        WALLOC(*out, half_t, (size_t)count * C * K);
        for (int i = 0; i < count; ++i)
            RUN(copy16(*out + (size_t)i * C * K, table_.src(a + "." + names[i] + ".weight"), (size_t)C * K, s));
        return 0;
    };
    static const char* const qkv[] = {"to_q", "to_k", "to_v"};
    static const char* const kv[] = {"to_k", "to_v"};
    static const char* const qonly[] = {"to_q"};
    t->qkv1.N = t->attn1_cross ? C : 3 * C; t->q2.N = C; t->qkvt.N = 3 * C; t->ff1.N = 8 * C;
    if (t->attn1_cross) {
        RUN(fuse(b + ".attn1", qonly, 1, C, &t->qkv1.w));
        RUN(fuse(b + ".attn1", kv, 2, X, &t->wkv1));
    } else {
        RUN(fuse(b + ".attn1", qkv, 3, C, &t->qkv1.w));
    }
    RUN(pack_linear(b + ".attn1.to_out.0", C, C, true, &t->o1, s));
    RUN(fuse(b + ".attn2", qonly, 1, C, &t->q2.w));
    RUN(fuse(b + ".attn2", kv, 2, X, &t->wkv2));
    RUN(pack_linear(b + ".attn2.to_out.0", C, C, true, &t->o2, s));
    RUN(fuse(b + ".attn_" + tname, qkv, 3, C, &t->qkvt.w));
    RUN(pack_linear(b + ".attn_" + tname + ".to_out.0", C, C, true, &t->ot, s));
    if (!cfg_.temporal_plain)
        RUN(pack_copy(b + ".attn_" + tname + ".time_rel_pos_bias.relative_attention_bias.weight", (size_t)cfg_.rel_buckets * cfg_.heads,
                      &t->relemb, s));
    const half_t* ff1_w = table_.src(b + ".ff.net.0.proj.weight");
    const half_t* ff1_b = table_.src(b + ".ff.net.0.proj.bias");
    WALLOC(t->ff1.w, half_t, (size_t)8 * C * C);
    WALLOC(t->ff1.b, float, 8 * C);
    RUN(launch_pack_geglu_rows(ff1_w, t->ff1.w, 8 * C, C, s));
    RUN(launch_pack_geglu_bias(ff1_b, t->ff1.b, 8 * C, s));
    RUN(pack_linear(b + ".ff.net.2", C, 4 * C, true, &t->ff2, s));
    // derived images and LayerNorm folds of the attention projections: allocated here, filled by derive_transformer() from the
    // packed copies above, which lora_apply() rewrites in place and fills again through the same function
    if (!cfg_.temporal_plain && !cfg_.vsr_blocks && temporal_block_supported(C, cfg_.heads, 16, cfg_.rotary_dim))
        WALLOC(t->tb_img, half_t, temporal_block_image_bytes(C) / sizeof(half_t));     // fused temporal sub-block (clips of 16 frames)
    if (!t->attn1_cross && !cfg_.vsr_blocks && cross_block_variant(C, cfg_.heads, 1, 16) == CROSS_SHORT)
        WALLOC(t->xb_tmpl[CROSS_SHORT], half_t, cross_block_image_bytes(CROSS_SHORT) / sizeof(half_t));       // fused text cross-attention sub-block
    if (!t->attn1_cross && !cfg_.vsr_blocks && proj_qkv_supported(C))                  // fused GroupNorm -> proj_in -> norm1 -> q|k|v
        WALLOC(t->pq_img, half_t, proj_qkv_image_bytes(C) / sizeof(half_t));
    if (geglu_mlp_supported(C)) {      // fused norm3 -> feed-forward -> residual kernel: weight image in MFMA-fragment order
        WALLOC(t->ff_img, half_t, geglu_mlp_image_bytes(C) / sizeof(half_t));
        WALLOC(t->ff_b1img, float, geglu_mlp_bias_floats(C));
        RUN(pack_geglu_mlp(ff1_w, ff1_b, table_.src(b + ".ff.net.2.weight"), C, t->ff_img, t->ff_b1img, s));
    }

    // LayerNorm-folded projections (norm1 -> attn1 qkv, norm2 -> attn2 q, norm_temp -> attn_temp qkv, norm3 -> GEGLU)
    auto fold_alloc = [&](LnProj* p) -> int {
        WALLOC(p->fw, half_t, (size_t)p->N * C);
        WALLOC(p->fs, float, p->N);
        WALLOC(p->fb, float, p->N);
        return 0;
    };
    for (LnProj* p : {&t->qkv1, &t->q2, &t->qkvt}) RUN(fold_alloc(p));      // filled by derive_transformer()
    RUN(derive_transformer(*t, s));
    {
        // GEGLU: fold in the checkpoint's row order, then apply the value/gate interleave to W', s and b'
        LnProj tmp = t->ff1;
        RUN(fold_alloc(&tmp));
        RUN(launch_ln_fold(ff1_w, t->ln3.g, t->ln3.b, ff1_b, tmp.fw, tmp.fs, tmp.fb, 8 * C, C, s));
        RUN(fold_alloc(&t->ff1));
        RUN(launch_pack_geglu_rows(tmp.fw, t->ff1.fw, 8 * C, C, s));
        RUN(launch_pack_geglu_vec(tmp.fs, t->ff1.fs, 8 * C, s));
        RUN(launch_pack_geglu_vec(tmp.fb, t->ff1.fb, 8 * C, s));
    }
    return 0;
}

// Everything of a transformer block that is computed from its attention projections, written into the allocations of
// pack_transformer() from the packed copies (qkv1, wkv1, o1, q2, o2, qkvt, ot, and proj_in for the GroupNorm -> q|k|v
// image): finalize() and lora_apply() share it, so an in-place re-derivation is the fresh build's sequence of kernels.
int UNet::derive_transformer(const TransformerW& t, hipStream_t s) {
    const int C = t.C;
    const size_t CC = (size_t)C * C;
    if (t.tb_img) RUN(pack_temporal_block(t.qkvt.w, t.qkvt.w + CC, t.qkvt.w + 2 * CC, t.ot.w, C, t.tb_img, s));
    for (int v = 0; v < kCrossVariants; ++v)
        if (t.xb_tmpl[v]) RUN(pack_cross_block((CrossVariant)v, t.o1.w, t.q2.w, t.o2.w, C, t.xb_tmpl[v], s));
    if (t.pq_img) RUN(pack_proj_qkv(t.pin.w, t.qkv1.w, C, t.pq_img, s));
    for (const LnProj* p : {&t.qkv1, &t.q2, &t.qkvt})
        RUN(launch_ln_fold(p->w, (t.*p->ln).g, (t.*p->ln).b, nullptr, p->fw, p->fs, p->fb, p->N, C, s));
    return 0;
}

int UNet::pack_temporal_res(const std::string& prefix, int C, int taps1, TemporalResW* out, hipStream_t s) {
    out->present = true;
    out->taps1 = taps1;
    RUN(pack_norm(prefix + ".norm1", C, &out->n1, s));
    RUN(pack_norm(prefix + ".norm2", C, &out->n2, s));
    WALLOC(out->w1, half_t, (size_t)C * taps1 * C);
    WALLOC(out->w2, half_t, (size_t)C * 3 * C);
    RUN(launch_pack_conv_taps(table_.src(prefix + ".conv1.weight"), out->w1, C, C, taps1, taps1 * C, 0, true, s));
    RUN(launch_pack_conv_taps(table_.src(prefix + ".conv2.weight"), out->w2, C, C, 3, 3 * C, 0, true, s));
    RUN(pack_f32(prefix + ".conv1.bias", C, &out->b1, s));
    return pack_f32(prefix + ".conv2.bias", C, &out->b2, s);
}

int UNet::pack_sampler(const std::string& prefix, int C, SamplerW* out, hipStream_t s, bool up) {
    const half_t* w = table_.src(prefix + ".weight");
    out->C = C;
    WALLOC(out->w, half_t, (size_t)C * 9 * C);
    RUN(launch_pack_conv3x3(w, out->w, C, C, 9 * C, 0, true, s));
    RUN(pack_f32(prefix + ".bias", C, &out->b, s));
    if (up && C % 160 == 0) {          // conv(nearest_x2(x)) as four 2x2 convs on x: weights of coinciding taps summed once, here
        WALLOC(out->wpar, half_t, (size_t)4 * C * 4 * C);
        RUN(launch_pack_conv3x3_parity(w, out->wpar, C, C, s));
    }
    return 0;
}

int UNet::finalize(hipStream_t s) {
    RUN(validate_config());
    LAVIE_CHECK(!finalized_, "finalize: already finalized");
    RUN(table_.all_set("finalize"));      // a missing tensor is refused here, before anything is allocated or enqueued
    if (const int rc = pack_model(s)) {
        // out of memory or a HIP error half way: give the arena back, so that a retry starts from nothing.  hipFree waits for the
        // copies and pack kernels already enqueued into it
        weights_.free_all();
        downs_.clear();
        ups_.clear();
        return rc;
    }
    lora_dirty_.assign(transformers_.size(), 0);
    table_.release();                     // the caller's tensors are read by what is enqueued on s: theirs again once s has drained
    finalized_ = true;
    return 0;
}

int UNet::pack_model(hipStream_t s) {
    const lavie_unet_config& c = cfg_;
    const int C0 = c.block_out_channels[0];
    WALLOC(zero_page_, half_t, 256);
    LAVIE_HIP(hipMemsetAsync(zero_page_, 0, 512, s));
    // conv_in / conv_out / conv_norm_out
    WALLOC(conv_in_w_, half_t, (size_t)9 * c.in_channels * C0);
    RUN(launch_pack_conv_in(table_.src("conv_in.weight"), conv_in_w_, C0, c.in_channels, s));
    RUN(pack_f32("conv_in.bias", C0, &conv_in_b_, s));
    WALLOC(conv_out_w_, half_t, (size_t)c.out_channels * 9 * C0);
    RUN(launch_pack_conv3x3(table_.src("conv_out.weight"), conv_out_w_, c.out_channels, C0, 9 * C0, 0, false, s));
    RUN(pack_f32("conv_out.bias", c.out_channels, &conv_out_b_, s));
    RUN(pack_norm("conv_norm_out", C0, &norm_out_, s));
    RUN(pack_linear("time_embedding.linear_1", C0 * 4, C0, true, &time1_, s));
    RUN(pack_linear("time_embedding.linear_2", C0 * 4, C0 * 4, true, &time2_, s));
    WALLOC(tproj_.w, half_t, (size_t)tproj_.N * tproj_.K);
    WALLOC(tproj_.b, float, tproj_.N);
    for (ResnetW& r : resnets_) RUN(pack_resnet(&r, s));
    for (TransformerW& t : transformers_) RUN(pack_transformer(&t, s));
    for (TemporalModuleW& m : tmods_) {
        const std::string t = m.prefix + ".resblocks_3d_t";
        RUN(pack_temporal_res(t, m.C, 5, &m.t, s));
        RUN(copy16(tproj_.w + (size_t)m.t_temb_off * tproj_.K, table_.src(t + ".time_emb_proj.weight"), (size_t)m.C * tproj_.K, s));
        RUN(launch_f16_to_f32(table_.src(t + ".time_emb_proj.bias"), tproj_.b + m.t_temb_off, m.C, s));
        RUN(pack_resnet(&m.s, s));
        RUN(pack_linear(m.prefix + ".shift_conv", m.C, m.C, true, &m.shift, s));
    }
    if (c.num_class_embeds > 0) RUN(pack_copy("class_embedding.weight", (size_t)c.num_class_embeds * C0 * 4, &class_emb_, s));
    const int L = c.num_levels;
    downs_.resize(L > 1 ? L - 1 : 0);
    ups_.resize(L > 1 ? L - 1 : 0);
    for (int l = 0; l + 1 < L; ++l)
        RUN(pack_sampler("down_blocks." + std::to_string(l) + ".downsamplers.0.conv", c.block_out_channels[l], &downs_[l], s));
    for (int i = 0; i + 1 < L; ++i)
        RUN(pack_sampler("up_blocks." + std::to_string(i) + ".upsamplers.0.conv", c.block_out_channels[L - 1 - i], &ups_[i], s, /*up=*/true));
    return 0;
}

int UNet::ensure_tables(int F, hipStream_t s) {
    if (tables_.count(F)) return 0;     // built before: switching clip length costs nothing and allocates nothing
    FrameTables ft;
    const int rp = cfg_.rotary_dim / 2;
    std::vector<float> hc((size_t)F * rp), hs((size_t)F * rp);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < rp; ++k) {
            const float freq = (float)pow(10000.0, -2.0 * k / cfg_.rotary_dim);
            const float ang = (float)f * freq;
            hc[(size_t)f * rp + k] = (float)cos((double)ang);
            hs[(size_t)f * rp + k] = (float)sin((double)ang);
        }
    std::vector<int> hb((size_t)F * F);
    relpos_bucket_table(F, cfg_.rel_buckets, cfg_.rel_max_distance, hb.data());
    int* buckets_dev = nullptr;
    WALLOC(ft.rot_cos, float, (size_t)F * rp);
    WALLOC(ft.rot_sin, float, (size_t)F * rp);
    WALLOC(buckets_dev, int, (size_t)F * F);
    // pageable host memory: these copies complete before returning (once per distinct F in the handle's lifetime)
    LAVIE_HIP(hipMemcpy(ft.rot_cos, hc.data(), hc.size() * sizeof(float), hipMemcpyHostToDevice));
    LAVIE_HIP(hipMemcpy(ft.rot_sin, hs.data(), hs.size() * sizeof(float), hipMemcpyHostToDevice));
    LAVIE_HIP(hipMemcpy(buckets_dev, hb.data(), hb.size() * sizeof(int), hipMemcpyHostToDevice));
    ft.relbias.assign(transformers_.size(), nullptr);
    if (cfg_.temporal_plain) {
        // plain softmax(scale q k^T) v over frames (interpolation/models/attention.py:268-289): one shared all-zero bias
        // table (s + 0.0f == s exactly) and rot_dim = 0 in the kernel parameters
        float* zero = nullptr;
        WALLOC(zero, float, (size_t)cfg_.heads * F * F);
        LAVIE_HIP(hipMemsetAsync(zero, 0, (size_t)cfg_.heads * F * F * sizeof(float), s));
        for (size_t i = 0; i < transformers_.size(); ++i) ft.relbias[i] = zero;
    } else {
        for (size_t i = 0; i < transformers_.size(); ++i) {
            WALLOC(ft.relbias[i], float, (size_t)cfg_.heads * F * F);
            RUN(launch_fill_relpos_bias(transformers_[i].relemb, buckets_dev, ft.relbias[i], cfg_.heads, F, s));
        }
    }
    LAVIE_HIP(hipStreamSynchronize(s));
    tables_.emplace(F, std::move(ft));
    return 0;
}

// ------------------------------------------------------------------ forward
// The switches that decide which kernels a call runs, as one value: read once where the call enters (call_ctx()) or enumerated by
// prepare() for its dry runs; nothing below reads the switches themselves
struct Route {
    int mask;               // fused_mask(): bits 0, 1, 2, 8 the row-resident kernels, 4 the parity upsample convs, 5 producer-side GroupNorm statistics
    bool shared;            // set_cfg_shared_input: the layers in front of the first text cross-attention run on half the batch
    bool ln_fold;           // set_ln_fold: LayerNorm folded into the producer / consumer GEMM epilogues
    int pag = 0;            // set_pag: trailing batch entries whose attn1 is the identity on values in the selected blocks (0 = off)
};

struct FwdCtx {
    hipStream_t s;
    DeviceArena* ws;
    bool dry;               // plan only: allocate, launch nothing
    Route route;
    int B, F, H, W, ctx_len;       // H x W: the latent size the call enters with (level 0)
    const FrameTables* tables;     // of this F; nullptr: none built (a call that runs no temporal attention, a dry run)
    bool text_cached, text_bound;  // text K / V: cached (cache_context) for this very ctx tensor and shape / bound into the fused kernel's images
    float* gn_ws = nullptr;        // GroupNorm scratch, gn_workspace_floats(B*F, groups) floats
    const int* labels = nullptr;   // VSR noise level per video (host), num_class_embeds > 0
    int lc_mode = LAVIE_LAYER_CACHE_OFF;      // layer cache: what this call does with it, and the depth of its cuts (0 with OFF)
    int lc_depth = 0;
};

FwdCtx UNet::call_ctx(hipStream_t s, DeviceArena* ws, int B, int F, int H, int W, const half_t* ctx, int ctx_len, int pag,
                      const Route* planned) const {
    const bool dry = planned != nullptr;
    const auto ft = tables_.find(F);
    const bool cached = !dry && kv_ctx_ != nullptr && kv_ctx_ == ctx && kv_B_ == B && kv_len_ == ctx_len;
    return FwdCtx{s, ws, dry, dry ? *planned : Route{fused_mask(), cfg_shared_input_, ln_fold_, pag}, B, F, H, W, ctx_len,
                  ft == tables_.end() ? nullptr : &ft->second, cached, cached && xb_bound_};
}

#define LAUNCH(expr)              \
    do {                          \
        if (!c.dry) RUN(expr);    \
    } while (0)

// Development aid (LAVIE_DEBUG_TRACE_HALVES=1): after the named step, wait for the stream and report whether the two batch halves of
// the rows are bit-equal (meaningful for a forward fed identical halves) — localises an irreproducible kernel
static bool trace_halves_on() {
    static const bool on = [] { const char* e = getenv("LAVIE_DEBUG_TRACE_HALVES"); return e && e[0] == '1'; }();
    return on;
}
static int trace_halves(const FwdCtx& c, const char* what, const void* p, size_t rows, size_t row_bytes, int line, int elt) {
    if (c.dry || !trace_halves_on() || rows % 2 != 0) return 0;
    LAVIE_HIP(hipStreamSynchronize(c.s));
    std::vector<unsigned char> h(rows * row_bytes);
    LAVIE_HIP(hipMemcpy(h.data(), p, h.size(), hipMemcpyDeviceToHost));
    const size_t half = rows / 2 * row_bytes;
    size_t bad = 0, first = 0, last = 0, bad_rows = 0, cmin = row_bytes, cmax = 0;
    for (size_t r = 0; r < rows / 2; ++r) {
        bool rb = false;
        for (size_t j = 0; j < row_bytes; ++j) {
            const size_t i = r * row_bytes + j;
            if (h[i] != h[half + i]) {
                if (!bad) first = i;
                last = i; ++bad; rb = true;
                if (j < cmin) cmin = j;
                if (j > cmax) cmax = j;
            }
        }
        bad_rows += rb;
    }
    fprintf(stderr, "[halves] line %d %-28s rows %zu x %zu B: %s", line, what, rows, row_bytes, bad ? "DIFFER" : "equal");
    if (bad) fprintf(stderr, " (%zu bytes in %zu rows, rows %zu .. %zu, col bytes %zu .. %zu)", bad, bad_rows, first / row_bytes, last / row_bytes, cmin, cmax);
    fprintf(stderr, "\n");
    if (bad && elt == 2) {          // the first few differing fp16 pairs
        int shown = 0;
        for (size_t i = 0; i + 1 < half && shown < 8; i += 2) {
            if (h[i] == h[half + i] && h[i + 1] == h[half + i + 1]) continue;
            _Float16 a, b;
            memcpy(&a, &h[i], 2); memcpy(&b, &h[half + i], 2);
            fprintf(stderr, "          row %zu col %zu: %.6g vs %.6g (bits %02x%02x %02x%02x)\n", i / row_bytes, (i % row_bytes) / 2, (double)a, (double)b,
                    h[i + 1], h[i], h[half + i + 1], h[half + i]);
            ++shown;
        }
    }
    return 0;
}
#define TRACE(what, ptr, rows, cols) RUN(trace_halves(c, what, ptr, (size_t)(rows), (size_t)(cols) * sizeof(*(ptr)), __LINE__, (int)sizeof(*(ptr))))

#define WS(var, type, count)                                                                                     \
    type* var = (type*)c.ws->alloc((size_t)(count) * sizeof(type));                                              \
    LAVIE_CHECK(var != nullptr, "workspace exhausted: call lavie_unet_prepare for this shape (needed %zu more B)", \
                (size_t)(count) * sizeof(type))

// LayerNorm row statistics of a block's residual stream, between the GEMM whose epilogue emits them and the LayerNorm-folded GEMMs
// that consume them.  The producer leaves per-wave-tile partials; the first consumer finalizes them on demand, once (round 4).
struct RowStats {
    float* partials;       // [M, slots, 2] (sum, sum^2): slots = one per wave tile of the producer's plan
    float* stats;          // [M, 2] (mean, rstd) of the rows
    int slots = 0, row_len = 0, rows = 0;      // of the latest producer
    bool pending = false;  // `partials` are newer than `stats`
};

// GroupNorm statistics from the producing kernel (igemm.h colstat_out, round 4): the buffer of an Act (engine.h) for a [M, C] tensor
static size_t colstat_floats(size_t M, int C) { return (M / COLSTAT_REDUCE_ROWS + 8) * (size_t)C * 2; }
// A new [rows, C] tensor and its statistics buffer, from the workspace
static int ws_act(FwdCtx& c, size_t rows, int C, Act* a) {
    WS(p, half_t, rows * C);
    WS(cs, float, colstat_floats(rows, C));
    *a = Act{p, C, GnColStat(), cs};
    return 0;
}
// One implicit GEMM on the forward's stream: plan it, take the split-K slab from the workspace, launch unless this is the dry run.
// The dry run passes placeholder addresses and so gets the plan of the real call.  *plan_out (optional) receives the plan.
// THE place that resets the statistics the output tensor carried (out; nullptr: no tensor a GroupNorm reads) and, where it has a
// buffer, has the epilogue fill it and describes the new ones in out->cs.
static int run_igemm(FwdCtx& c, IgemmParams& p, bool gather, int epilogue, Act* out, IgemmPlan* plan_out = nullptr) {
    const size_t mark = c.ws->mark();
    IgemmPlan plan;
    const int rc = igemm_run(p, gather, epilogue, c.s, [&](size_t bytes, float** slab) {
        *slab = (float*)c.ws->alloc(bytes);
        LAVIE_CHECK(c.dry || *slab != nullptr, "workspace exhausted (split-K slab)");
        return 0;
    }, out && (c.route.mask & 32) ? out->csbuf : nullptr, c.dry, &plan);
    c.ws->release(mark);
    if (out) out->cs = p.colstat_out ? gn_colstat_describe(p, plan, out->csbuf) : GnColStat();
    if (plan_out) *plan_out = plan;
    return rc;
}

// C[M, w.N] = A[M, w.K] w^T + bias (+ R); the GEGLU epilogue writes [M, w.N / 2].  What the epilogue leaves besides, both stated
// by every caller: rs = LayerNorm statistics of the output rows (with fold_s, the row sums of LayerNorm-folded weights, the GEMM
// consumes the statistics of its input rows instead); gn = the tensor C is the contents of, for its GroupNorm statistics
static int linear(FwdCtx& c, const half_t* A, const LinW& w, const half_t* R, half_t* C, int M, RowStats* rs, Act* gn,
                  int epilogue = EPI_LINEAR, const float* fold_s = nullptr) {
    const int N = w.N, K = w.K, ldc = epilogue == EPI_GEGLU ? N / 2 : N;
    IgemmParams p;
    RUN(igemm_setup_linear(&p, A, K, w.w, K, w.b, C, ldc, M, N, K));
    p.R = R;
    const bool emit = rs && !fold_s;
    p.rowstat_out = emit ? rs->partials : nullptr;
    if (fold_s) {
        p.ln_s = fold_s;
        if (rs->pending) {           // the producer left its partials: finalize now, once
            LAUNCH(launch_rowstat_finalize(rs->partials, rs->slots, rs->rows, rs->row_len, 1e-5f, rs->stats, c.s));
            rs->pending = false;
        }
        p.ln_stats = rs->stats;
    }
    // column statistics describe a plain dense output only: behind any other epilogue the tensor is left with none
    const bool dense = epilogue == EPI_LINEAR && ldc == N;
    if (gn && !dense) gn->cs = GnColStat();
    IgemmPlan plan;
    RUN(run_igemm(c, p, false, epilogue, dense ? gn : nullptr, &plan));
    if (emit) {
        rs->slots = N / plan.rowstat_cols;      // one slot per wave tile of the kernel that ran
        rs->row_len = N; rs->rows = M; rs->pending = true;
    }
    return 0;
}

// 3x3 conv (pad 1) of x [.., C], plus the optional centre-tap shortcut sources sc1 | sc2 (nullptr: none) as further K segments.
static int conv3x3(FwdCtx& c, const half_t* x, int C, const Act* sc1, const Act* sc2, const half_t* W, int ldw, const float* bias,
                   const float* bias2, int ldb2, int rows_per_batch, const half_t* R, Act* y, int NI, int Hi, int Wi, int stride,
                   int ups, const half_t* zero) {
    const half_t* sc[2] = {sc1 ? sc1->p : nullptr, sc2 ? sc2->p : nullptr};
    const int scC[2] = {sc1 ? sc1->C : 0, sc2 ? sc2->C : 0};      // (a source of no channels is no segment)
    IgemmParams p;
    RUN(igemm_setup_conv3x3(&p, &x, &C, 1, sc, scC, 2, W, ldw, y->p, NI, Hi, Wi, y->C, stride, ups, zero));
    p.bias = bias; p.bias2 = bias2; p.ldb2 = ldb2; p.rows_per_batch = rows_per_batch; p.R = R;
    return run_igemm(c, p, true, EPI_LINEAR, y);
}

// (taps,1,1) temporal conv over the frame axis of token rows [(b f d), C] (IgemmParams temporal mode; 128-row kernel).
static int tconv(FwdCtx& c, const half_t* x, int C, const half_t* W, const float* bias, const float* bias2, int ldb2,
                 const half_t* R, Act* y, int D, int taps, const half_t* zero) {
    IgemmParams p;
    RUN(igemm_setup_temporal_conv(&p, x, C, W, bias, y->p, c.B, c.F, D, y->C, taps, zero));
    p.bias2 = bias2; p.ldb2 = ldb2; p.rows_per_batch = c.F * D; p.R = R;
    return run_igemm(c, p, true, EPI_LINEAR, y);      // (round 4) the GroupNorm behind a temporal conv folds its epilogue's sums too
}

// ResnetBlock3DCNN (vsr/models/resnet.py:283-315): y = x + conv2(silu(gn(conv1(silu(gn(x))) + temb))); GroupNorm statistics
// span the whole video (5-D input), eps 1e-6; bias2 = the block's rows of the fused time-embedding projection or nullptr
// (attention.py:350: temb_channels=None).  y may be x itself (in place): norm1 has taken x's statistics, and in stream order read
// their buffer, long before conv2's epilogue replaces them.
int UNet::run_temporal_res(FwdCtx& c, const TemporalResW& r, const Act& x, Act* y, int D, const float* bias2, int ldb2) {
    const int C = x.C;
    const size_t M = (size_t)c.B * c.F * D;
    const int P = c.F * D;
    const size_t mark = c.ws->mark();
    WS(nrm, half_t, M * C);
    Act h1;
    RUN(ws_act(c, M, C, &h1));
    LAUNCH(launch_group_norm(x.p, C, nullptr, 0, c.B, P, cfg_.norm_groups, r.n1.g, r.n1.b, 1e-6f, true, c.gn_ws, nrm, c.s, &x.cs));
    TRACE("tres.norm1", nrm, M, C);
    RUN(tconv(c, nrm, C, r.w1, r.b1, bias2, ldb2, nullptr, &h1, D, r.taps1, zero_page_));
    TRACE("tres.conv1", h1.p, M, C);
    LAUNCH(launch_group_norm(h1.p, C, nullptr, 0, c.B, P, cfg_.norm_groups, r.n2.g, r.n2.b, 1e-6f, true, c.gn_ws, nrm, c.s, &h1.cs));
    TRACE("tres.norm2", nrm, M, C);
    RUN(tconv(c, nrm, C, r.w2, r.b2, nullptr, 0, x.p, y, D, 3, zero_page_));
    TRACE("tres.conv2", y->p, M, C);
    c.ws->release(mark);
    return 0;
}

// TemporalModule3D.forward (vsr/models/temporal_module.py:153-178): y = x + shift_conv(resblocks_3d_s(resblocks_3d_t(x))).
// y must not alias x when x is still referenced as a skip tensor.
int UNet::run_temporal_module(FwdCtx& c, const TemporalModuleW& m, const Act& x, Act* y, const float* tproj, int ld_tproj, int H, int W) {
    const int C = m.C, D = H * W;
    const size_t M = (size_t)c.B * c.F * D;
    const size_t mark = c.ws->mark();
    WS(h1p, half_t, M * C);
    WS(h2p, half_t, M * C);
    WS(h1cs, float, colstat_floats(M, C));
    Act h1{h1p, C, GnColStat(), h1cs}, h2{h2p, C};      // (h2's one consumer is no GroupNorm)
    RUN(run_temporal_res(c, m.t, x, &h1, D, tproj + m.t_temb_off, ld_tproj));
    RUN(run_resnet(c, m.s, h1, nullptr, tproj + m.s.temb_off, ld_tproj, &h2, H, W));
    RUN(linear(c, h2.p, m.shift, x.p, y->p, (int)M, nullptr, y));
    TRACE("tmodule.shift", y->p, M, C);
    c.ws->release(mark);
    return 0;
}

int UNet::run_resnet(FwdCtx& c, const ResnetW& r, const Act& x1, const Act* x2, const float* tproj, int ld_tproj, Act* y, int H, int W) {
    const int C1 = x1.C, C2 = x2 ? x2->C : 0;
    LAVIE_CHECK(C1 + C2 == r.cin, "resnet %s: got %d+%d input channels, expected %d", r.prefix.c_str(), C1, C2, r.cin);
    const int G = cfg_.norm_groups;
    const int NI = c.B * c.F;
    const int P = c.F * H * W;            // rows sharing GroupNorm statistics: the whole video (resnet.py:180)
    const size_t M = (size_t)NI * H * W;
    const size_t mark = c.ws->mark();
    WS(nrm, half_t, M * r.cin);
    WS(h1p, half_t, M * r.cout);
    WS(n2, half_t, M * r.cout);
    WS(h1cs, float, colstat_floats(M, r.cout));      // GroupNorm statistics of h1, written by conv1's epilogue
    Act h1{h1p, r.cout, GnColStat(), h1cs};
    const float eps = r.eps > 0.f ? r.eps : cfg_.norm_eps;
    // norm1: statistics from the producers of x1 / x2 where they left them, else the statistics pass
    LAUNCH(launch_group_norm(x1.p, C1, x2 ? x2->p : nullptr, C2, c.B, P, G, r.n1.g, r.n1.b, eps, true, c.gn_ws, nrm, c.s, &x1.cs,
                             x2 ? &x2->cs : nullptr));
    TRACE("resnet.norm1", nrm, M, r.cin);
    RUN(conv3x3(c, nrm, r.cin, nullptr, nullptr, r.w1, 9 * r.cin, r.b1, tproj, ld_tproj, P, nullptr, &h1, NI, H, W, 1, 0, zero_page_));
    TRACE("resnet.conv1", h1.p, M, r.cout);
    LAUNCH(launch_group_norm(h1.p, r.cout, nullptr, 0, c.B, P, G, r.n2.g, r.n2.b, eps, true, c.gn_ws, n2, c.s, &h1.cs));
    TRACE("resnet.norm2", n2, M, r.cout);
    // The 1x1 conv_shortcut rides in conv2 as extra centre-tap K segments — which keeps conv2 off the halo-patch kernel (it
    // takes 9-tap segments only).  Running the shortcut as its own GEMM in front of a halo-patch conv2 was measured slower
    // (round 3, profiles/r03_ab_split_shortcut.txt: forward 21.33 -> 21.41 ms) and is not built.
    RUN(conv3x3(c, n2, r.cout, r.shortcut ? &x1 : nullptr, r.shortcut ? x2 : nullptr, r.w2, r.ldw2, r.b2, nullptr, 0, 1,
                r.shortcut ? nullptr : x1.p, y, NI, H, W, 1, 0, zero_page_));
    TRACE("resnet.conv2", y->p, M, r.cout);
    c.ws->release(mark);
    return 0;
}

// The route of one transformer block: which kernel runs each sub-block and which producers of the residual stream `tx` emit
// LayerNorm row statistics.  Host arithmetic only; run_transformer() sequences launches from it and decides nothing itself.
struct BlockRoute {
    bool ff_first;          // interpolation block order: feed-forward -> temporal (base: temporal -> feed-forward)
    bool fused_head;        // GroupNorm -> proj_in -> norm1 -> q|k|v as one row-resident kernel (rowfuse_pin.hip)
    CrossVariant text;      // attn1.to_out .. attn2.to_out + residual: GEMMs (CROSS_NONE), or one kernel, of this variant
    bool fused_t, fused_ff; // the temporal / feed-forward sub-block as one row-resident kernel (rowfuse.hip)
    bool fold_t, fold_ff;   // else: its first GEMM is LayerNorm-folded (false: an explicit LayerNorm in front of it)
    bool emit_pin, emit_o1, emit_o2, emit_ot, emit_ff2;        // proj_in, attn1 / attn2 / temporal to_out, ff2: row statistics from the epilogue
};
// text_bound: the text K / V of this block are cached and bound into its fused-kernel image for this very context
static BlockRoute block_route(const lavie_unet_config& cfg, const TransformerW& t, const Route& r, int F, int D, int ctx_len, bool text_bound) {
    const int heads = cfg.heads;
    const bool fold = r.ln_fold;
    BlockRoute b;
    b.ff_first = cfg.ff_before_temporal != 0;
    b.fused_head = t.pq_img != nullptr && !t.tres.present && !t.attn1_cross && (r.mask & 256) && D % 16 == 0;
    // The row-resident kernels take their LayerNorm statistics from the rows they hold.  The feed-forward kernel fits both block orders:
    // in the interpolation order it also writes the finished (mean, rstd) rows that the folded temporal q|k|v projection behind it reads
    b.fused_ff = t.ff_img != nullptr && (r.mask & 1) && (!b.ff_first || fold);
    b.fused_t = t.tb_img != nullptr && !b.ff_first && F == 16 && (r.mask & 2);
    // The fused text kernel emits no row statistics, so the sub-block behind it must be one that needs none
    const bool fused_x = t.xb_tmpl[CROSS_SHORT] != nullptr && text_bound && (b.ff_first ? b.fused_ff : b.fused_t) && !t.attn1_cross && (r.mask & 4);
    b.text = fused_x ? cross_block_variant(t.C, heads, ctx_len, F * D) : CROSS_NONE;
    // A GEMM behind a LayerNorm is folded when its producer can emit the statistics: the fused temporal kernel cannot
    b.fold_t = fold && !b.fused_t;
    b.fold_ff = fold && !b.fused_ff && !b.fused_t;
    // THE emission rule: a producer emits row statistics exactly when the next consumer of the residual stream is a LayerNorm-folded
    // GEMM.  The consumers, in order: attn1 q(kv), attn2 q, then temporal q|k|v and ff1 in the block's order, then proj_out (no LayerNorm)
    const bool gemms = b.text == CROSS_NONE;
    b.emit_pin = !b.fused_head && fold;
    b.emit_o1 = gemms && fold;
    b.emit_o2 = gemms && (b.ff_first ? b.fold_ff : b.fold_t);
    b.emit_ot = !b.fused_t && !b.ff_first && b.fold_ff;
    b.emit_ff2 = !b.fused_ff && b.ff_first && b.fold_t;
    return b;
}

int UNet::run_transformer(FwdCtx& c, const TransformerW& t, Act& x, const half_t* ctx, int H, int W, bool shared_prefix) {
    const int C = t.C, G = cfg_.norm_groups, heads = cfg_.heads, dh = C / heads;
    const int NI = c.B * c.F, D = H * W;
    const int T = NI * D;
    const int X = cfg_.cross_attention_dim;
    const float scale = 1.0f / sqrtf((float)dh);
    const size_t mark = c.ws->mark();
    WS(tx, half_t, (size_t)T * C);
    WS(ln, half_t, (size_t)T * C);
    WS(att, half_t, (size_t)T * C);
    WS(wide, half_t, (size_t)T * 4 * C);          // qkv [T,3C] / GEGLU output [T,4C] / q2 [T,C]
    WS(kv2, half_t, (size_t)c.B * c.ctx_len * 2 * C);
    const size_t ti = &t - transformers_.data();
    const BlockRoute br = block_route(cfg_, t, c.route, c.F, D, c.ctx_len, c.text_bound && xb_img_[ti] != nullptr);
    const bool fold = c.route.ln_fold;

    // VSR: ResnetBlock3DCNN (3,1,1) on the block input, before the residual is taken (vsr/models/attention.py:395-400)
    if (t.tres.present) {
        // in place; conv2's epilogue leaves the new statistics where the old ones were (the per-frame GroupNorm below takes them only
        // if its frames are whole blocks: the temporal tiles of the halo-patch kernel span a video, GnColStat::span)
        RUN(run_temporal_res(c, t.tres, x, &x, D, nullptr, 0));
    }
    // shared_prefix (set_cfg_shared_input; base block only): both halves of the batch are identical up to the text
    // cross-attention, so GroupNorm, proj_in, the qkv projection and the self-attention run on the first half (NIp frames,
    // Tp rows) and `tx` / `att` are copied to the second
    const int NIp = shared_prefix ? NI / 2 : NI, Tp = shared_prefix ? T / 2 : T;
    LAVIE_CHECK(!shared_prefix || (!t.tres.present && !t.attn1_cross && c.B % 2 == 0), "transformer: shared prefix on an unsupported block");
    // perturbed-attention guidance (set_pag, which vouches for the plain self-attention branch): the last pagF frames take no softmax
    const int pagF = c.route.pag > 0 && ti < pag_sel_.size() && pag_sel_[ti] ? c.route.pag * c.F : 0;
    LAVIE_CHECK(pagF == 0 || (!shared_prefix && !t.attn1_cross && !cfg_.sparse_causal_attn1 && pagF < NI),
                "transformer: perturbed attention on an unsupported block or batch (B=%d, perturbed=%d)", c.B, c.route.pag);
    WS(gn_ab, float, (size_t)NI * C * 2);        // (planned whether or not the fused head runs: the plan must not depend on it)
    // LayerNorm folding: the GEMM that produces the residual stream `tx` also emits per-row (sum, sum^2) partials of
    // its fp16 output, and the projection that consumes LN(tx) runs on raw `tx` with gamma folded into its weights,
    // finishing rstd * (acc - mean * s) + b' in its epilogue — no LayerNorm kernel, no normalised copy in HBM.
    RowStats rs{nullptr, nullptr};
    if (fold) {
        WS(rsp, float, (size_t)T * (C / 32) * 2);
        WS(rsm, float, (size_t)T * 2);
        rs.partials = rsp;
        rs.stats = rsm;
    }
    auto emit = [&](bool on) { return on ? &rs : nullptr; };
    // THE projection behind a LayerNorm, `rows` rows of tx -> wide.  Folded: one GEMM on the raw rows that takes their statistics;
    // otherwise the LayerNorm into `ln`, then the plain GEMM
    auto ln_proj = [&](const LnProj& p, bool folded, int rows, int epilogue = EPI_LINEAR) -> int {
        if (folded) return linear(c, tx, LinW{p.fw, p.fb, p.N, C}, nullptr, wide, rows, &rs, nullptr, epilogue, p.fs);
        LAUNCH(launch_layernorm(tx, (t.*p.ln).g, (t.*p.ln).b, ln, rows, C, 1e-5f, c.s));
        return linear(c, ln, LinW{p.w, p.b, p.N, C}, nullptr, wide, rows, nullptr, nullptr, epilogue);
    };
    // Text attention through GEMMs (attn2; attn1 of the VSR only_cross_attention levels): q of every token, K | V once per video,
    // from the cache or computed here
    auto text_attention = [&](const LnProj& q, half_t* wkv, const std::vector<half_t*>& cache) -> int {
        RUN(ln_proj(q, fold, T));
        const half_t* kvc = kv2;
        if (c.text_cached) kvc = cache[ti];
        else RUN(linear(c, ctx, LinW{wkv, nullptr, 2 * C, X}, nullptr, kv2, c.B * c.ctx_len, nullptr, nullptr));
        if (!c.dry) {
            AttnParams a;
            a.q = wide; a.ldq = C; a.k = kvc; a.ldk = 2 * C; a.v = kvc + C; a.ldv = 2 * C;
            a.o = att; a.ldo = C; a.NBq = NI; a.Lq = D; a.Lk = c.ctx_len; a.heads = heads; a.dh = dh; a.kv_batch_div = c.F; a.scale = scale;
            RUN(launch_attention(a, c.s));
        }
        return 0;
    };
    if (br.fused_head) {
        // Round 4: the norm's statistics become per-(frame, channel) scale / shift pairs and nothing between x and (tx, qkv) touches memory
        LAUNCH(launch_group_norm(x.p, C, nullptr, 0, NIp, D, G, t.gn.g, t.gn.b, 1e-6f, false, c.gn_ws, nullptr, c.s, &x.cs, nullptr, gn_ab));
        LAUNCH(launch_proj_qkv(x.p, gn_ab, D, t.pq_img, t.pin.b, t.ln1.g, t.ln1.b, 1e-5f, tx, wide, Tp, C, c.s));
    } else {
        // per-frame GroupNorm (eps 1e-6) + 1x1 proj_in (attention.py:369-373)
        LAUNCH(launch_group_norm(x.p, C, nullptr, 0, NIp, D, G, t.gn.g, t.gn.b, 1e-6f, false, c.gn_ws, ln, c.s, &x.cs));
        RUN(linear(c, ln, t.pin, nullptr, tx, Tp, emit(br.emit_pin), nullptr));
    }
    if (!shared_prefix) TRACE("block.proj_in", tx, T, C);

    if (t.attn1_cross) {
        // VSR only_cross_attention levels: attn1 attends to the text context (vsr/models/attention.py:558-561)
        RUN(text_attention(t.qkv1, t.wkv1, kv1_cache_));
    } else {
        // spatial self-attention (attention.py:513-522)
        if (!br.fused_head) RUN(ln_proj(t.qkv1, fold, Tp));      // (the fused head left q | k | v in `wide`)
        if (!c.dry) {
            AttnParams a;
            a.q = wide; a.ldq = 3 * C; a.k = wide + C; a.ldk = 3 * C; a.v = wide + 2 * C; a.ldv = 3 * C;
            a.o = att; a.ldo = C; a.NBq = NIp - pagF; a.Lq = D; a.Lk = D; a.heads = heads; a.dh = dh; a.kv_batch_div = 1; a.scale = scale;
            if (cfg_.sparse_causal_attn1) {      // keys/values = first frame || previous frame (interpolation attention.py:630-639)
                a.Lk = 2 * D;
                a.sc_frames = c.F;
            }
            RUN(launch_attention(a, c.s));
            // the perturbed entries: attention = the identity on values, so their rows of `att` are the V columns of q | k | v
            if (pagF) {
                const size_t r0 = (size_t)(NI - pagF) * D;
                RUN(launch_copy_rows(wide + r0 * 3 * C + 2 * C, 3 * C, att + r0 * C, C, pagF * D, C, 0, c.s));
            }
        }
    }
    if (!shared_prefix) TRACE("block.attn1 q(kv)", wide, T, t.attn1_cross ? C : 3 * C);
    if (!shared_prefix) TRACE("block.attn1", att, T, C);
    if (shared_prefix && !c.dry) {       // the second half of the batch: the same residual stream and attention output so far
        LAVIE_HIP(hipMemcpyAsync(tx + (size_t)Tp * C, tx, (size_t)Tp * C * sizeof(half_t), hipMemcpyDeviceToDevice, c.s));
        LAVIE_HIP(hipMemcpyAsync(att + (size_t)Tp * C, att, (size_t)Tp * C * sizeof(half_t), hipMemcpyDeviceToDevice, c.s));
    }
    // attn1.to_out -> + residual -> norm2 -> attn2 -> to_out -> + residual: one kernel on this context's K / V image ...
    if (br.text != CROSS_NONE) {
        LAUNCH(launch_cross_block(br.text, att, tx, tx, T, c.F * D, C, heads, xb_img_[ti], t.o1.b, t.ln2.g, t.ln2.b, t.o2.b, c.ctx_len, scale, 1e-5f, c.s));
    } else {       // ... or GEMMs
        RUN(linear(c, att, t.o1, tx, tx, T, emit(br.emit_o1), nullptr));
        TRACE("block.attn1.to_out", tx, T, C);

        // text cross-attention (attention.py:524-534); K/V once per video instead of once per frame (364)
        RUN(text_attention(t.q2, t.wkv2, kv2_cache_));
        TRACE("block.attn2", att, T, C);
        RUN(linear(c, att, t.o2, tx, tx, T, emit(br.emit_o2), nullptr));
    }
    TRACE("block.after text", tx, T, C);

    auto temporal = [&]() -> int {
        // temporal self-attention over frames, tokens stay in (b f) d order (attention.py:548-555)
        if (br.fused_t) {      // norm_temp -> q|k|v -> rotary / bias / softmax / PV -> to_out -> + residual in ONE kernel, in place
            LAUNCH(launch_temporal_block(tx, tx, c.B, c.F, D, C, heads, t.tb_img, t.lnt.g, t.lnt.b, t.ot.b, c.tables->relbias[ti],
                                         c.tables->rot_cos, c.tables->rot_sin, cfg_.rotary_dim, scale, 1e-5f, c.s));
            return 0;
        }
        RUN(ln_proj(t.qkvt, br.fold_t, T));
        if (br.fold_t) TRACE("temporal.row statistics", rs.stats, T, 2);
        TRACE("temporal.qkv before", wide, T, 3 * C);
        if (!c.dry) {
            TemporalParams tp;
            tp.qkv = wide; tp.ld = 3 * C; tp.o = att; tp.ldo = C; tp.B = c.B; tp.F = c.F; tp.D = D; tp.heads = heads; tp.dh = dh;
            tp.bias = c.tables->relbias[ti]; tp.rot_cos = c.tables->rot_cos; tp.rot_sin = c.tables->rot_sin; tp.rot_dim = cfg_.temporal_plain ? 0 : cfg_.rotary_dim; tp.scale = scale;
            RUN(launch_temporal_attention(tp, c.s));
        }
        TRACE("temporal.qkv", wide, T, 3 * C);
        TRACE("temporal.attention", att, T, C);
        RUN(linear(c, att, t.ot, tx, tx, T, emit(br.emit_ot), nullptr));
        return 0;
    };
    auto feed_forward = [&]() -> int {
        // GEGLU feed-forward (attention.py:558)
        if (br.fused_ff) {     // norm3 -> ff1 -> GEGLU -> ff2 -> + residual in ONE kernel, in place on the residual stream
            // interpolation order: norm_temp consumes this output; the kernel writes its (mean, rstd) rows where ff2's epilogue +
            // rowstat_finalize would have put them: finished rows, nothing pending
            LAUNCH(launch_geglu_mlp(tx, tx, T, C, t.ff_img, t.ff_b1img, t.ln3.g, t.ln3.b, t.ff2.b, 1e-5f, c.s, br.ff_first ? rs.stats : nullptr));
            if (br.ff_first) rs.pending = false;
            return 0;
        }
        RUN(ln_proj(t.ff1, br.fold_ff, T, EPI_GEGLU));
        // (K = 4C: the planner may pick another kernel than for the K = C producers, hence a slot count per producer)
        RUN(linear(c, wide, t.ff2, tx, tx, T, emit(br.emit_ff2), nullptr));
        return 0;
    };
    // base block order: temporal -> feed-forward (attention.py:548-560); interpolation block: feed-forward -> temporal
    // (interpolation/models/attention.py:592-604)
    if (br.ff_first) {
        RUN(feed_forward());
        TRACE("block.feed-forward", tx, T, C);
        RUN(temporal());
        TRACE("block.temporal", tx, T, C);
    } else {
        RUN(temporal());
        TRACE("block.temporal", tx, T, C);
        RUN(feed_forward());
        TRACE("block.feed-forward", tx, T, C);
    }

    // 1x1 proj_out + residual, in place on the block input (attention.py:394-401)
    // (its epilogue leaves the GroupNorm statistics of the block's output for the next resnet / skip consumer: x.cs is rewritten)
    RUN(linear(c, tx, t.pout, x.p, x.p, T, nullptr, &x));
    TRACE("block.proj_out", x.p, T, C);
    c.ws->release(mark);
    return 0;
}

int UNet::run_conv(FwdCtx& c, const Act& x, const SamplerW& w, Act* y, int Hi, int Wi, int stride, int ups) {
    const int C = x.C;
    if (ups && stride == 1 && w.wpar && (c.route.mask & 16)) {
        // Upsample3D (resnet.py:44-79): the 3x3 conv of the nearest-x2 image as four 2x2 convs on the source image, one per
        // output parity, on the halo-patch kernel (igemm_patch.hip MODE 3): 4 C instead of 9 C multiply-adds per output element
        IgemmParams p;
        if (igemm_setup_parity_upsample(&p, x.p, C, w.wpar, w.b, y->p, c.B * c.F, Hi, Wi, zero_page_)) return run_igemm(c, p, true, EPI_LINEAR, y);
    }
    return conv3x3(c, x.p, C, nullptr, nullptr, w.w, 9 * C, w.b, nullptr, 0, 1, nullptr, y, c.B * c.F, Hi, Wi, stride, ups, zero_page_);
}

int UNet::run(FwdCtx& c, const half_t* sample, const float* timesteps, const half_t* ctx, half_t* out) {
    const lavie_unet_config& cfg = cfg_;
    const int L = cfg.num_levels;
    const int NI = c.B * c.F;
    const int C0 = cfg.block_out_channels[0];
    const int temb = C0 * 4;
    const int G = cfg.norm_groups;

    // GroupNorm scratch (partials + mean/rstd), shared by every GroupNorm of the pass: stream order keeps it safe
    {
        WS(gnws, float, gn_workspace_floats(NI, G));
        c.gn_ws = gnws;
    }

    // time embedding (unet.py:428-434) and all 22 resnet projections in one GEMV (resnet.py:186)
    WS(tsin, float, (size_t)c.B * C0);
    WS(e1, float, (size_t)c.B * temb);
    WS(emb, float, (size_t)c.B * temb);
    WS(tproj, float, (size_t)c.B * tproj_.N);
    LAUNCH(launch_timestep_sinusoid(timesteps, tsin, c.B, C0, c.s));
    LAUNCH(launch_gemv(tsin, time1_.w, time1_.b, e1, c.B, temb, C0, 0, 1, c.s));
    // `emb` only ever reaches the resnets through SiLU (resnet.py:186): apply it once here instead of once per
    // output feature inside the stacked projection
    if (cfg.num_class_embeds > 0) {
        // emb = time_embedding + class_embedding[noise level] (vsr/models/unet.py:494-505), then the consumers' SiLU
        LAUNCH(launch_gemv(e1, time2_.w, time2_.b, emb, c.B, temb, temb, 0, 0, c.s));
        if (!c.dry) {
            LAVIE_CHECK(c.labels != nullptr, "forward: this model has a class embedding: call lavie_unet_forward_labels");
            for (int b = 0; b < c.B; ++b)
                LAVIE_CHECK(c.labels[b] >= 0 && c.labels[b] < cfg.num_class_embeds, "forward: class label %d out of range", c.labels[b]);
            RUN(launch_add_class_emb_silu(emb, class_emb_, c.labels, c.B, temb, c.s));
        }
    } else {
        LAUNCH(launch_gemv(e1, time2_.w, time2_.b, emb, c.B, temb, temb, 0, 1, c.s));
    }
    LAUNCH(launch_gemv(emb, tproj_.w, tproj_.b, tproj, c.B, tproj_.N, temb, 0, 0, c.s));

    std::vector<int> Hs(L), Ws(L);
    for (int l = 0; l < L; ++l) {
        Hs[l] = l == 0 ? c.H : (Hs[l - 1] - 1) / 2 + 1;
        Ws[l] = l == 0 ? c.W : (Ws[l - 1] - 1) / 2 + 1;
    }
    auto rows = [&](int l) { return (size_t)NI * Hs[l] * Ws[l]; };

    Act x;      // the running activation; the skips keep theirs
    std::vector<Act> skips;
    size_t ri = 0, ti = 0, mi = 0;
    const bool tmod = cfg.vsr_temporal_modules != 0;

    // Layer cache (set_layer_cache): cut A lies behind layer lcd - 1 of down level 0, cut B in front of layer layers_per_block - lcd
    // of the last up block.  A refresh call is the full walk whose producer of the running activation at B writes it into the cache
    // block instead of the workspace (`to_cache`: the next new tensor); a reuse call walks the same list of steps, but between the
    // cuts (`deep`) a step only advances its counter and the skip stack holds placeholders, and at B the cached tensor becomes x.
    const int lpb = cfg.layers_per_block;
    const int lcd = c.lc_mode != LAVIE_LAYER_CACHE_OFF ? c.lc_depth : 0;
    const bool refresh = c.lc_mode == LAVIE_LAYER_CACHE_REFRESH, reuse = c.lc_mode == LAVIE_LAYER_CACHE_REUSE;
    bool deep = false, to_cache = false;
    Act filled;                 // refresh: the tensor at B as its producer left it
    auto new_act = [&](size_t nrows, int C, Act* a) -> int {
        if (!to_cache) return ws_act(c, nrows, C, a);
        to_cache = false;
        // (a dry run has no block: placeholder addresses, as the virtual arena hands out)
        half_t* p = c.dry ? (half_t*)(uintptr_t)256 : (half_t*)lc_block_;
        const size_t act_bytes = (nrows * C * sizeof(half_t) + 255) & ~(size_t)255;
        LAVIE_CHECK(c.dry || (lc_block_ && act_bytes + colstat_floats(nrows, C) * sizeof(float) <= lc_bytes_),
                    "forward: the layer cache holds %zu B, this shape needs more: call lavie_unet_prepare for it", lc_bytes_);
        *a = Act{p, C, GnColStat(), (float*)((char*)p + (c.dry ? 0 : act_bytes))};
        return 0;
    };

    // Classifier-free guidance runs the UNet on the latents twice with different text: up to the first text cross-attention
    // (conv_in, the first resnet, and GroupNorm / proj_in / self-attention of the first transformer block) the two halves of the
    // batch are the same computation.  With set_cfg_shared_input the caller vouches for sample[b] == sample[b + B/2]; those
    // layers then run on the first half and their outputs are copied (base UNet only: the first down block must have attention).
    const bool shared_ok = c.B % 2 == 0 && cfg.attn_levels[0] && cfg.layers_per_block >= 1 && !tmod && !cfg.vsr_blocks &&
                           cfg.num_class_embeds == 0 && !cfg.sparse_causal_attn1 && !transformers_[0].attn1_cross && !transformers_[0].tres.present;
    // a caller that left the switch on for a batch or model it cannot apply to gets an error, not a silently different amount of work
    LAVIE_CHECK(!c.route.shared || shared_ok || c.dry || c.route.pag > 0, "forward: set_cfg_shared_input(1) needs an even batch (B=%d) and the base UNet "
                "(attention in the first down block, no VSR / interpolation variants)", c.B);
    // (while perturbed-attention guidance is on the switch is ignored, include/lavie_hip.h: the batch is [.. | prompt | perturbed])
    const bool shared = c.route.shared && shared_ok && c.route.pag == 0;
    if (shared && !c.dry && debug_check_shared()) {
        // LAVIE_DEBUG_CHECK_SHARED=1: verify the caller's promise (sample[b] == sample[b + B/2], equal timesteps) before trusting it
        const size_t half_bytes = (size_t)(c.B / 2) * cfg.in_channels * c.F * c.H * c.W * sizeof(half_t);
        std::vector<char> h0(half_bytes), h1(half_bytes);
        std::vector<float> ts(c.B);
        LAVIE_HIP(hipStreamSynchronize(c.s));
        LAVIE_HIP(hipMemcpy(h0.data(), sample, half_bytes, hipMemcpyDeviceToHost));
        LAVIE_HIP(hipMemcpy(h1.data(), (const char*)sample + half_bytes, half_bytes, hipMemcpyDeviceToHost));
        LAVIE_HIP(hipMemcpy(ts.data(), timesteps, c.B * sizeof(float), hipMemcpyDeviceToHost));
        LAVIE_CHECK(memcmp(h0.data(), h1.data(), half_bytes) == 0, "forward: set_cfg_shared_input(1) but the two halves of the sample differ");
        for (int b = 0; b < c.B / 2; ++b)
            LAVIE_CHECK(ts[b] == ts[b + c.B / 2], "forward: set_cfg_shared_input(1) but timesteps %g / %g differ", ts[b], ts[b + c.B / 2]);
    }
    FwdCtx ch = c;                       // the same stream / workspace / scratch, half the batch
    if (shared) ch.B = c.B / 2;
    auto dup_half = [&](half_t* p, size_t rows_full, int ch_count) -> int {
        if (shared && !c.dry)
            LAVIE_HIP(hipMemcpyAsync(p + rows_full / 2 * ch_count, p, rows_full / 2 * ch_count * sizeof(half_t), hipMemcpyDeviceToDevice, c.s));
        return 0;
    };
    // The steps of the walk below: each takes a new tensor and its statistics buffer from the workspace, runs on x, and advances x
    auto resnet = [&](FwdCtx& cc, int l, const Act* skip) -> int {
        const ResnetW& r = resnets_[ri++];
        if (deep) return 0;
        Act y;
        RUN(new_act(rows(l), r.cout, &y));
        RUN(run_resnet(cc, r, x, skip, tproj + r.temb_off, tproj_.N, &y, Hs[l], Ws[l]));
        x = y;
        return 0;
    };
    auto transformer = [&](int l, bool shared_prefix) {      // in place on x
        const TransformerW& t = transformers_[ti++];
        return deep ? 0 : run_transformer(c, t, x, ctx, Hs[l], Ws[l], shared_prefix);
    };
    auto resample = [&](const SamplerW& w, int l, int l_out) -> int {      // down: stride 2; up: nearest x2 in front of the conv
        if (deep) return 0;
        Act y;
        RUN(new_act(rows(l_out), x.C, &y));
        RUN(run_conv(c, x, w, &y, Hs[l], Ws[l], l_out > l ? 2 : 1, l_out < l ? 1 : 0));
        x = y;
        return 0;
    };
    auto temporal_module = [&](int l) -> int {      // VSR; into a NEW buffer: x itself may stay alive as a skip
        const TemporalModuleW& m = tmods_[mi++];
        if (deep) return 0;
        Act y;
        RUN(new_act(rows(l), x.C, &y));
        RUN(run_temporal_module(c, m, x, &y, tproj, tproj_.N, Hs[l], Ws[l]));
        x = y;
        return 0;
    };

    WS(x0, half_t, rows(0) * C0);
    LAUNCH(launch_conv_in(sample, conv_in_w_, conv_in_b_, x0, ch.B, cfg.in_channels, c.F, Hs[0], Ws[0], C0, c.s));
    RUN(dup_half(x0, rows(0), C0));
    x = Act{x0, C0};           // conv_in leaves no statistics: its two consumers run the statistics pass
    skips.push_back(x);

    for (int l = 0; l < L; ++l) {
        for (int j = 0; j < cfg.layers_per_block; ++j) {
            // the shared prefix: the first resnet runs on the first half of the batch and its output is copied to the second; x.cs then
            // describes the first half, which is all its one consumer, the half-batch GroupNorm of the first transformer block, reads
            const bool first = shared && l == 0 && j == 0;
            RUN(resnet(first ? ch : c, l, nullptr));
            if (first) RUN(dup_half(x.p, rows(l), x.C));
            if (cfg.attn_levels[l]) RUN(transformer(l, first));
            else if (first) x.cs = GnColStat();
            skips.push_back(x);
            if (reuse && l == 0 && j + 1 == lcd) deep = true;      // cut A
        }
        if (l + 1 < L) {
            RUN(resample(downs_[l], l, l + 1));
            skips.push_back(x);
        }
        if (tmod) RUN(temporal_module(l + 1 < L ? l + 1 : l));      // after the downsampler (vsr/models/unet.py:523-533)
    }
    RUN(resnet(c, L - 1, nullptr));
    RUN(transformer(L - 1, false));
    RUN(resnet(c, L - 1, nullptr));
    if (tmod) RUN(temporal_module(L - 1));
    for (int i = 0; i < L; ++i) {
        const int l = L - 1 - i;
        for (int j = 0; j < cfg.layers_per_block + 1; ++j) {
            if (lcd > 0 && i == L - 1 && j == lpb - lcd) {          // cut B
                if (refresh) filled = x;
                if (reuse) {
                    x = c.dry ? Act{(half_t*)(uintptr_t)256, lc_channels(lcd)} : lc_act_;
                    deep = false;
                }
            }
            // refresh: the resnet in front of B (and the transformer behind it, in place) produces the cached tensor
            if (refresh && i == L - 1 && j + 1 == lpb - lcd) to_cache = true;
            Act sk = skips.back();
            skips.pop_back();
            if (i < 2 && !deep) {
                // FreeU (diffusers apply_freeu), in place: both tensors have this resnet as their one consumer left.  Its mode-sum
                // partials are taken from the workspace whether FreeU is on or off (so prepare()'s plan covers a setting made after
                // it) and given back at once: the resnet's buffers lie over them, behind the launches in stream order.  A tensor
                // FreeU changes no longer has its producer's GroupNorm statistics: norm1 runs the statistics pass, as behind conv_in
                const size_t fmark = c.ws->mark();
                WS(freeu_ws, float, freeu_workspace_floats(sk.C, NI, Hs[l], Ws[l]));
                if (freeu_b_[i] != 1.f || freeu_s_[i] != 1.f) {
                    LAUNCH(launch_freeu(x.p, x.C, sk.p, sk.C, NI, Hs[l], Ws[l], freeu_b_[i], freeu_s_[i], x.p, sk.p, freeu_ws, c.s));
                    if (freeu_b_[i] != 1.f) x.cs = GnColStat();
                    if (freeu_s_[i] != 1.f) sk.cs = GnColStat();
                }
                c.ws->release(fmark);
            }
            RUN(resnet(c, l, &sk));
            if (cfg.attn_levels[l]) RUN(transformer(l, false));
        }
        // refresh at the full depth: B lies in front of the last up block, its tensor comes from the upsampler into level 0 or, in the
        // VSR model, from the temporal module behind it
        const bool into_b = refresh && lcd == lpb && i == L - 2;
        if (into_b && !tmod) to_cache = true;
        if (i + 1 < L) RUN(resample(ups_[i], l, l - 1));
        if (into_b && tmod) to_cache = true;
        if (tmod) RUN(temporal_module(i + 1 < L ? l - 1 : l));      // after the upsampler (vsr/models/unet.py:575-590)
    }
    // conv_norm_out + SiLU + conv_out (unet.py:504-506), back to the caller's NCFHW layout
    {
        WS(nrm, half_t, rows(0) * C0);
        const int P = c.F * Hs[0] * Ws[0];
        LAUNCH(launch_group_norm(x.p, C0, nullptr, 0, c.B, P, G, norm_out_.g, norm_out_.b, cfg.norm_eps, true, c.gn_ws, nrm, c.s, &x.cs));
        LAUNCH(launch_conv_out(nrm, conv_out_w_, conv_out_b_, out, c.B, C0, c.F, Hs[0], Ws[0], cfg.out_channels, c.s));
    }
    if (refresh && !c.dry) lc_act_ = filled;
    return 0;
}

static int check_shape(const lavie_unet_config& cfg, int B, int F, int H, int W, int ctx_len) {
    LAVIE_CHECK(B >= 1 && B <= 8 && F >= 1 && F <= 64 && H >= 1 && W >= 1 && ctx_len >= 1,
                "shape: B=%d (1..8) F=%d (1..64) H=%d W=%d ctx_len=%d unsupported", B, F, H, W, ctx_len);
    const int div = 1 << (cfg.num_levels - 1);
    LAVIE_CHECK(H % div == 0 && W % div == 0, "shape: H=%d W=%d must be multiples of %d (unet.py:393-401 upsample-size "
                "forwarding is not implemented)", H, W, div);
    return 0;
}

int UNet::prepare(int B, int F, int H, int W, int ctx_len) {
    LAVIE_CHECK(finalized_, "prepare: call lavie_unet_finalize first");
    RUN(check_shape(cfg_, B, F, H, W, ctx_len));
    // The forward may run under other switches than the ones current now (the guided loop turns the shared CFG prefix on AFTER
    // prepare(); lavie_debug_fused_mask and the text cache change which GEMMs run, and a half-batch launch may plan another
    // split-K slab): the plan is the maximum over every combination of them, so none of those switches can outgrow the workspace.
    // Each combination is a Route value handed to a dry run: no switch is touched.
    size_t peak = 0;
    const int mask = fused_mask();
    // masks: the current one; without the row-resident kernels (bits 0 - 2, 8: their GEMMs and row-statistics buffers appear); and both
    // again with every workspace-consuming option on (bit 4: the parity form's slabs, 5: statistics buffers)
    const int masks[4] = {mask, mask & ~0x107, mask | 0x30, (mask | 0x30) & ~0x107};
    for (int variant = 0; variant < 8; ++variant) {
        if ((variant & 1) && B % 2 != 0) continue;
        DeviceArena plan;
        plan.init_virtual();
        // (Route::pag = 0: perturbed-attention guidance runs every GEMM on all rows and takes nothing from the workspace that the plain
        // branch does not, so the plan holds for a setting made before or after; with it the shared-input variants would go unplanned)
        const Route route{masks[variant >> 1], (variant & 1) != 0, ln_fold_, 0};
        FwdCtx c = call_ctx(nullptr, &plan, B, F, H, W, nullptr, ctx_len, 0, &route);
        RUN(run(c, nullptr, nullptr, nullptr, nullptr));
        if (plan.peak() > peak) peak = plan.peak();
        // The shallow walk of a layer-cache reuse call, at every depth the model admits (so a depth set after prepare() is covered): its
        // allocations are a subsequence of the full walk's, so its peak cannot exceed the one above; it is planned all the same and the
        // relation is checked, so a step added to one walk only does not go unnoticed.  (A refresh call takes one tensor less.)
        for (int depth = 1; cfg_.num_levels >= 3 && depth <= cfg_.layers_per_block; ++depth) {
            DeviceArena shallow;
            shallow.init_virtual();
            FwdCtx cs = call_ctx(nullptr, &shallow, B, F, H, W, nullptr, ctx_len, 0, &route);
            cs.lc_mode = LAVIE_LAYER_CACHE_REUSE;
            cs.lc_depth = depth;
            RUN(run(cs, nullptr, nullptr, nullptr, nullptr));
            LAVIE_CHECK(shallow.peak() <= plan.peak(), "prepare: the shallow walk at depth %d plans %zu B, more than the full walk's %zu B",
                        depth, shallow.peak(), plan.peak());
        }
    }
    if (B != lc_shape_[0] || F != lc_shape_[1] || H != lc_shape_[2] || W != lc_shape_[3]) lc_key_[0] = 0;      // another shape: a held cache is invalid
    lc_shape_[0] = B; lc_shape_[1] = F; lc_shape_[2] = H; lc_shape_[3] = W;
    RUN(ensure_layer_cache());
    const size_t need = peak + (1 << 20);
    if (need > ws_.total_bytes()) {
        drop_graph();                               // the captured addresses die with the old workspace
        ++graph_gen_;
        RUN(ws_.init_fixed(need));
    }
    return 0;
}

int UNet::ensure_layer_cache() {
    size_t need = 0;
    if (lc_depth_ > 0 && lc_shape_[0] > 0) {
        const size_t rows0 = (size_t)lc_shape_[0] * lc_shape_[1] * lc_shape_[2] * lc_shape_[3];
        const int C = lc_channels(lc_depth_);
        need = ((rows0 * C * sizeof(half_t) + 255) & ~(size_t)255) + colstat_floats(rows0, C) * sizeof(float);
    }
    if (need == lc_bytes_) return 0;
    lc_key_[0] = 0;
    lc_act_ = Act();
    if (lc_block_) {
        LAVIE_HIP(hipDeviceSynchronize());          // a forward in flight may still read it
        (void)hipFree(lc_block_);
        lc_block_ = nullptr;
        lc_bytes_ = 0;
    }
    if (need > 0) {
        LAVIE_HIP(hipMalloc(&lc_block_, need));
        lc_bytes_ = need;
    }
    return 0;
}

int UNet::set_layer_cache(int depth) {
    LAVIE_CHECK(depth >= 0 && depth <= cfg_.layers_per_block, "set_layer_cache: depth=%d must be 0 (off) or 1..%d (layers_per_block)", depth,
                cfg_.layers_per_block);
    LAVIE_CHECK(depth == 0 || cfg_.num_levels >= 3, "set_layer_cache: the model has %d levels, the layer cache needs 3 or more (FreeU's two "
                "deepest up blocks must stay below level 0)", cfg_.num_levels);
    lc_key_[0] = 0;
    lc_depth_ = depth;
    return ensure_layer_cache();
}

int UNet::set_freeu(float s1, float s2, float b1, float b2) {
    const float v[4] = {s1, s2, b1, b2};
    for (float f : v)
        LAVIE_CHECK(__builtin_isfinite(f) && f > 0.f, "set_freeu: s1=%g s2=%g b1=%g b2=%g must all be finite and > 0", (double)s1, (double)s2,
                    (double)b1, (double)b2);
    freeu_s_[0] = s1; freeu_s_[1] = s2; freeu_b_[0] = b1; freeu_b_[1] = b2;
    ++graph_gen_;                                   // a captured forward holds the old setting's launches
    return 0;
}

int UNet::set_pag(const char* const* layers, int n_layers, int perturbed) {
    LAVIE_CHECK(n_layers >= 0 && (n_layers == 0 || layers != nullptr), "set_pag: n_layers=%d with layers_host %s", n_layers,
                layers ? "given" : "null");
    LAVIE_CHECK(perturbed >= 0, "set_pag: perturbed=%d must be >= 0", perturbed);
    std::vector<char> sel(transformers_.size(), 0);
    for (int i = 0; i < n_layers; ++i) {
        LAVIE_CHECK(layers[i] != nullptr && layers[i][0] != 0, "set_pag: layers_host[%d] is null or empty", i);
        const std::string e = layers[i];
        int hits = 0;
        for (size_t ti = 0; ti < transformers_.size(); ++ti) {
            const TransformerW& t = transformers_[ti];
            if (t.prefix.compare(0, e.size(), e) != 0 || (t.prefix.size() > e.size() && t.prefix[e.size()] != '.')) continue;
            LAVIE_CHECK(!t.attn1_cross && !cfg_.sparse_causal_attn1,
                        "set_pag: layers_host[%d]='%s' selects %s, whose attn1 is not the plain spatial self-attention (%s)", i, layers[i],
                        t.prefix.c_str(), t.attn1_cross ? "only_cross_attention level" : "sparse-causal attention");
            sel[ti] = 1;
            ++hits;
        }
        LAVIE_CHECK(hits > 0, "set_pag: layers_host[%d]='%s' selects no transformer (prefixes are spelled as in the state dict: "
                    "mid_block, down_blocks.2, up_blocks.1.attentions.0, ...)", i, layers[i]);
    }
    LAVIE_CHECK(finalized_, "set_pag: call lavie_unet_finalize first");
    const bool on = n_layers > 0 && perturbed > 0;
    if (on) pag_sel_ = sel; else pag_sel_.clear();
    pag_perturbed_ = on ? perturbed : 0;
    ++graph_gen_;                                   // a captured forward holds the old setting's launches
    return 0;
}

int UNet::pag_route(const char* who, int B) const {
    if (pag_perturbed_ == 0) return 0;
    if (B <= pag_perturbed_) {
        set_error("%s: B=%d but perturbed=%d batch entries take the perturbed attention (lavie_unet_set_pag): B must be larger", who, B,
                  pag_perturbed_);
        return -1;
    }
    return pag_perturbed_;
}

void UNet::drop_graph() {
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    graph_exec_ = nullptr;
    graph_ = nullptr;
    graph_key_ = GraphKey();
}

int UNet::forward_graph(const half_t* sample, const float* timesteps, const half_t* ctx, half_t* out, int B, int F, int H, int W,
                        int ctx_len, hipStream_t stream) {
    bool profiling = false;
    for (int cls = 0; cls < KC_COUNT; ++cls) profiling = profiling || profile_enabled(cls);
    GraphKey key;
    key.sample = sample; key.t = timesteps; key.ctx = ctx; key.out = out; key.kv_ctx = kv_ctx_;
    key.B = B; key.F = F; key.H = H; key.W = W; key.L = ctx_len; key.gen = graph_gen_; key.debug_epoch = debug_epoch(); key.stream = stream;
    if (profiling) return forward(sample, timesteps, ctx, out, B, F, H, W, ctx_len, stream, nullptr);
    if (graph_exec_ && key == graph_key_) {
        LAVIE_HIP(hipGraphLaunch(graph_exec_, stream));
        return 0;
    }
    if (!(key == graph_seen_)) {                    // first sight of this tuple: eager (one-time setup must not be captured)
        graph_seen_ = key;
        return forward(sample, timesteps, ctx, out, B, F, H, W, ctx_len, stream, nullptr);
    }
    drop_graph();
    // captured on a private stream (the caller's may be the legacy default stream, which cannot be captured); the graph
    // itself is launched on the caller's stream
    if (!cap_stream_) LAVIE_HIP(hipStreamCreateWithFlags(&cap_stream_, hipStreamNonBlocking));
    LAVIE_HIP(hipStreamBeginCapture(cap_stream_, hipStreamCaptureModeThreadLocal));
    const int rc = forward(sample, timesteps, ctx, out, B, F, H, W, ctx_len, cap_stream_, nullptr);
    hipGraph_t g = nullptr;
    const hipError_t end = hipStreamEndCapture(cap_stream_, &g);
    if (rc != 0 || end != hipSuccess || g == nullptr) {
        if (g) (void)hipGraphDestroy(g);
        graph_seen_ = GraphKey();
        if (rc != 0) return rc;
        LAVIE_CHECK(false, "forward_graph: stream capture failed (%s)", hipGetErrorString(end));
    }
    graph_ = g;
    LAVIE_HIP(hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0));
    graph_key_ = key;
    LAVIE_HIP(hipGraphLaunch(graph_exec_, stream));
    return 0;
}

int UNet::forward(const half_t* sample, const float* timesteps, const half_t* ctx, half_t* out, int B, int F, int H, int W,
                  int ctx_len, hipStream_t stream, const int* class_labels_host, int layer_cache) {
    LAVIE_CHECK(finalized_, "forward: call lavie_unet_finalize first");
    LAVIE_CHECK(sample && timesteps && ctx && out, "forward: null tensor");
    RUN(check_shape(cfg_, B, F, H, W, ctx_len));
    LAVIE_CHECK(ws_.total_bytes() > 0, "forward: call lavie_unet_prepare first");
    const int key[6] = {B, F, H, W, ctx_len, lc_depth_};
    if (layer_cache != LAVIE_LAYER_CACHE_OFF) {
        const char* what = layer_cache == LAVIE_LAYER_CACHE_REUSE ? "reuse" : "refresh";
        LAVIE_CHECK(layer_cache == LAVIE_LAYER_CACHE_REFRESH || layer_cache == LAVIE_LAYER_CACHE_REUSE,
                    "forward_cached: mode=%d must be 0 (off), 1 (refresh) or 2 (reuse)", layer_cache);
        LAVIE_CHECK(lc_depth_ > 0, "forward_cached: %s needs a layer cache: call lavie_unet_set_layer_cache with a depth >= 1", what);
        // the cache's contents and its record belong to the order of execution, which a captured call has none of yet
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        LAVIE_HIP(hipStreamIsCapturing(stream, &cap));
        LAVIE_CHECK(cap == hipStreamCaptureStatusNone, "forward_cached: %s on a capturing stream is not supported", what);
        if (layer_cache == LAVIE_LAYER_CACHE_REUSE) {
            LAVIE_CHECK(lc_key_[0] != 0, "forward_cached: reuse without a valid layer cache: run a refresh forward (mode 1) first");
            LAVIE_CHECK(memcmp(key, lc_key_, sizeof(key)) == 0,
                        "forward_cached: reuse with B=%d F=%d H=%d W=%d ctx_len=%d depth=%d, but the cache was filled with B=%d F=%d H=%d W=%d "
                        "ctx_len=%d depth=%d", B, F, H, W, ctx_len, lc_depth_, lc_key_[0], lc_key_[1], lc_key_[2], lc_key_[3], lc_key_[4], lc_key_[5]);
        } else {
            lc_key_[0] = 0;                         // invalid until the walk has been enqueued whole
        }
    }
    RUN(ensure_tables(F, stream));
    ws_.release(0);
    const int pag = pag_route("forward", B);
    if (pag < 0) return -1;
    FwdCtx c = call_ctx(stream, &ws_, B, F, H, W, ctx, ctx_len, pag);
    c.labels = class_labels_host;
    c.lc_mode = layer_cache;
    c.lc_depth = layer_cache != LAVIE_LAYER_CACHE_OFF ? lc_depth_ : 0;
    RUN(run(c, sample, timesteps, ctx, out));
    if (layer_cache == LAVIE_LAYER_CACHE_REFRESH) memcpy(lc_key_, key, sizeof(key));
    return 0;
}

int UNet::cache_context(const half_t* ctx, int B, int ctx_len, hipStream_t stream) {
    LAVIE_CHECK(finalized_, "cache_context: call lavie_unet_finalize first");
    kv_ctx_ = nullptr;                              // invalid until every buffer is written
    ++graph_gen_;
    if (ctx == nullptr) return 0;
    LAVIE_CHECK(B >= 1 && B <= 8 && ctx_len >= 1, "cache_context: B=%d ctx_len=%d unsupported", B, ctx_len);
    LAVIE_CHECK(ws_.total_bytes() > 0, "cache_context: call lavie_unet_prepare first (split-K slabs come from the workspace)");
    const size_t rows = (size_t)B * ctx_len;
    const int X = cfg_.cross_attention_dim;
    const int C0 = cfg_.block_out_channels[0];
    const CrossVariant xv = cross_block_variant(C0, cfg_.heads, ctx_len, 16);
    if (xv == CROSS_LONG) RUN(ensure_long_templates(stream));
    const size_t img_bytes = cross_block_image_bytes(xv);      // (no variant: as the short one)
    if (rows > kv_cache_rows_ || B > kv_cache_B_ || kv2_cache_.size() != transformers_.size() || img_bytes > xb_img_bytes_) {
        // the cache lives in a block of its own: a longer context frees the old block instead of stranding it in the
        // grow-only weights arena.  Earlier forwards that read the old block are ordered before the free by the sync.
        size_t total = 0;
        auto span = [&](size_t i) { return (rows * 2 * transformers_[i].C * sizeof(half_t) + 255) & ~(size_t)255; };
        // a long context lays the images out for the long layout; a short one after it keeps (and uses the front of) the larger ones
        const size_t xb_bytes = img_bytes > xb_img_bytes_ ? img_bytes : xb_img_bytes_;
        auto img_span = [&](size_t i) { return transformers_[i].xb_tmpl[CROSS_SHORT] ? (size_t)B * xb_bytes : 0; };
        for (size_t i = 0; i < transformers_.size(); ++i) total += span(i) * (transformers_[i].attn1_cross ? 2 : 1) + img_span(i);
        if (kv_block_) {
            LAVIE_HIP(hipStreamSynchronize(stream));
            LAVIE_HIP(hipFree(kv_block_));
            kv_block_ = nullptr;
            kv_cache_rows_ = 0;
            kv_cache_B_ = 0;
            xb_img_bytes_ = 0;
        }
        LAVIE_HIP(hipMalloc(&kv_block_, total));
        kv2_cache_.assign(transformers_.size(), nullptr);
        kv1_cache_.assign(transformers_.size(), nullptr);
        xb_img_.assign(transformers_.size(), nullptr);
        char* cur = (char*)kv_block_;
        for (size_t i = 0; i < transformers_.size(); ++i) {
            kv2_cache_[i] = (half_t*)cur; cur += span(i);
            if (transformers_[i].attn1_cross) { kv1_cache_[i] = (half_t*)cur; cur += span(i); }
            if (img_span(i)) { xb_img_[i] = (half_t*)cur; cur += img_span(i); }
        }
        kv_cache_rows_ = rows;
        kv_cache_B_ = B;
        xb_img_bytes_ = xb_bytes;
    }
    ws_.release(0);
    FwdCtx c = call_ctx(stream, &ws_, B, 1, 0, 0, ctx, ctx_len, /*pag (attn1 only)=*/0);
    for (size_t i = 0; i < transformers_.size(); ++i) {
        const TransformerW& t = transformers_[i];
        RUN(linear(c, ctx, LinW{t.wkv2, nullptr, 2 * t.C, X}, nullptr, kv2_cache_[i], (int)rows, nullptr, nullptr));
        if (t.attn1_cross) RUN(linear(c, ctx, LinW{t.wkv1, nullptr, 2 * t.C, X}, nullptr, kv1_cache_[i], (int)rows, nullptr, nullptr));
    }
    // the fused cross-attention kernel streams K / V with its weights: one image per video, written here once per context
    xb_bound_ = false;
    if (xv != CROSS_NONE) {
        for (size_t i = 0; i < transformers_.size(); ++i)
            if (xb_img_[i]) RUN(bind_cross_block(xv, transformers_[i].xb_tmpl[xv], kv2_cache_[i], B, ctx_len, transformers_[i].C, xb_img_[i], stream));
        xb_bound_ = true;
    }
    kv_ctx_ = ctx;
    kv_B_ = B;
    kv_len_ = ctx_len;
    return 0;
}

// Long templates (the 81..160-key variant of the fused text cross-attention) are built on the first long context, not at finalize:
// a text-only model never pays for them (one 840 KiB template per level-0 transformer: 4.1 MiB at the production config, 5 blocks).
// Once built, derive_transformer() re-derives them with the short ones, so an adapter change keeps them current.
int UNet::ensure_long_templates(hipStream_t stream) {
    if (xbl_block_) return 0;
    size_t n = 0;
    for (const TransformerW& t : transformers_) n += t.xb_tmpl[CROSS_SHORT] ? 1 : 0;
    if (n == 0) return 0;
    const size_t bytes = cross_block_image_bytes(CROSS_LONG);
    LAVIE_HIP(hipMalloc(&xbl_block_, n * bytes));
    char* cur = (char*)xbl_block_;
    for (TransformerW& t : transformers_) {
        if (!t.xb_tmpl[CROSS_SHORT]) continue;
        t.xb_tmpl[CROSS_LONG] = (half_t*)cur;
        cur += bytes;
        RUN(pack_cross_block(CROSS_LONG, t.o1.w, t.q2.w, t.o2.w, t.C, t.xb_tmpl[CROSS_LONG], stream));
    }
    return 0;
}

// ------------------------------------------------------------------ low-rank adapters
// `name` is `<transformer>.transformer_blocks.0.<attn1 | attn2 | attn_temp(oral)>.<to_q | to_k | to_v | to_out.0>.weight`: attn = 0 / 1 / 2,
// proj = 0 .. 3.  Host only: the C ABI refuses a bad name before any HIP call.
int UNet::lora_target(const char* name, int* ti, int* attn, int* proj) const {
    LAVIE_CHECK(table_.find(name) != nullptr, "lora: unknown state-dict key '%s'", name);
    const std::string tname = cfg_.vsr_blocks ? "attn_temporal" : "attn_temp";
    const char* const attns[3] = {"attn1", "attn2", tname.c_str()};
    static const char* const projs[4] = {"to_q", "to_k", "to_v", "to_out.0"};
    const std::string n = name;
    for (size_t i = 0; i < transformers_.size(); ++i) {
        const std::string p = transformers_[i].prefix + ".transformer_blocks.0.";
        if (n.compare(0, p.size(), p) != 0) continue;
        for (int a = 0; a < 3; ++a)
            for (int j = 0; j < 4; ++j)
                if (n.compare(p.size(), std::string::npos, std::string(attns[a]) + "." + projs[j] + ".weight") == 0) {
                    *ti = (int)i; *attn = a; *proj = j;
                    return 0;
                }
    }
    LAVIE_CHECK(false, "lora: '%s' is not a LoRA target (only the to_q / to_k / to_v / to_out.0 weights of attn1 / attn2 / %s)",
                name, tname.c_str());
}

void UNet::lora_free(LoraSlot& s) {
    if (s.A) (void)hipFree(s.A);
    if (s.B) (void)hipFree(s.B);
    s.A = s.B = nullptr;
    s.r = 0;
}

int UNet::lora_set(const char* name, const half_t* base, const float* A, const float* B, int r, float scale, hipStream_t stream) {
    return lora_set_slot(0, name, base, A, B, r, scale, stream);
}

int UNet::lora_set_slot(int slot, const char* name, const half_t* base, const float* A, const float* B, int r, float scale,
                        hipStream_t stream) {
    LAVIE_CHECK(slot >= 0 && slot < kLoraMaxTerms, "lora_set: slot %d outside 0..%d", slot, kLoraMaxTerms - 1);
    LAVIE_CHECK(name && base && A && B, "lora_set: null argument");
    LAVIE_CHECK(r >= 1 && r <= kLoraMaxRank, "lora_set: rank %d outside 1..%d", r, kLoraMaxRank);
    LAVIE_CHECK(__builtin_isfinite(scale), "lora_set: scale %g is not finite", (double)scale);
    int ti = 0, attn = 0, proj = 0;
    RUN(lora_target(name, &ti, &attn, &proj));
    LAVIE_CHECK(finalized_, "lora_set: call lavie_unet_finalize first");
    auto found = lora_.find(name);
    if (found == lora_.end()) {
        const TransformerW& t = transformers_[ti];
        LoraEntry e;
        e.ti = ti;
        e.N = t.C;                                  // every target is [C][K]: K = C, or the text width behind to_k / to_v
        e.K = (int)(table_.find(name)->numel / e.N);
        const size_t nk = (size_t)e.N * e.K;
        if (proj == 3) e.dst = attn == 0 ? t.o1.w : attn == 1 ? t.o2.w : t.ot.w;
        else if (attn == 0 && t.attn1_cross) e.dst = proj == 0 ? t.qkv1.w : t.wkv1 + (proj - 1) * nk;
        else if (attn == 0) e.dst = t.qkv1.w + proj * nk;
        else if (attn == 1) e.dst = proj == 0 ? t.q2.w : t.wkv2 + (proj - 1) * nk;
        else e.dst = t.qkvt.w + proj * nk;
        LAVIE_HIP(hipMalloc((void**)&e.base, nk * sizeof(half_t)));
        found = lora_.emplace(name, e).first;
    }
    LoraEntry& e = found->second;
    LoraSlot& s = e.slot[slot];
    lora_dirty_[ti] = 1;        // from here on the entry may change; should an allocation below fail, the next apply still visits
                                // the block and drops an entry that was left without a slot
    if (s.r != r) {
        if (s.A || s.B) {       // an earlier apply may still read them
            LAVIE_HIP(hipStreamSynchronize(stream));
            lora_free(s);
        }
        LAVIE_HIP(hipMalloc((void**)&s.A, (size_t)r * e.K * sizeof(float)));
        LAVIE_HIP(hipMalloc((void**)&s.B, (size_t)e.N * r * sizeof(float)));
    }
    // the base of a target is the same tensor whichever slot registers it: copying it again is idempotent
    LAVIE_HIP(hipMemcpyAsync(e.base, base, (size_t)e.N * e.K * sizeof(half_t), hipMemcpyDeviceToDevice, stream));
    LAVIE_HIP(hipMemcpyAsync(s.A, A, (size_t)r * e.K * sizeof(float), hipMemcpyDeviceToDevice, stream));
    LAVIE_HIP(hipMemcpyAsync(s.B, B, (size_t)e.N * r * sizeof(float), hipMemcpyDeviceToDevice, stream));
    s.r = r;
    s.scale = scale;
    return 0;
}

int UNet::lora_clear(const char* name, hipStream_t stream) { return lora_clear_slot(0, name, stream); }

int UNet::lora_clear_slot(int slot, const char* name, hipStream_t stream) {
    LAVIE_CHECK(slot >= 0 && slot < kLoraMaxTerms, "lora_clear: slot %d outside 0..%d", slot, kLoraMaxTerms - 1);
    int ti = 0, attn = 0, proj = 0;
    if (name) RUN(lora_target(name, &ti, &attn, &proj));
    LAVIE_CHECK(finalized_, "lora_clear: call lavie_unet_finalize first");
    bool synced = false;
    for (auto& kv : lora_) {
        LoraEntry& e = kv.second;
        if ((name && kv.first != name) || e.slot[slot].r == 0) continue;
        if (!synced) { LAVIE_HIP(hipStreamSynchronize(stream)); synced = true; }
        lora_free(e.slot[slot]);    // the base copy stays: with no slot left, until the next apply has written it back
        lora_dirty_[e.ti] = 1;
    }
    return 0;
}

int UNet::lora_set_scale(float scale) {
    LAVIE_CHECK(__builtin_isfinite(scale), "lora_set_scale: scale %g is not finite", (double)scale);
    LAVIE_CHECK(finalized_, "lora_set_scale: call lavie_unet_finalize first");
    if (scale == lora_scale_) return 0;
    lora_scale_ = scale;
    for (const auto& kv : lora_) lora_dirty_[kv.second.ti] = 1;
    return 0;
}

int UNet::lora_set_slot_weight(int slot, float weight) {
    LAVIE_CHECK(slot >= 0 && slot < kLoraMaxTerms, "lora_set_slot_weight: slot %d outside 0..%d", slot, kLoraMaxTerms - 1);
    LAVIE_CHECK(__builtin_isfinite(weight), "lora_set_slot_weight: weight %g is not finite", (double)weight);
    LAVIE_CHECK(finalized_, "lora_set_slot_weight: call lavie_unet_finalize first");
    if (weight == lora_weight_[slot]) return 0;
    lora_weight_[slot] = weight;
    for (const auto& kv : lora_)
        if (kv.second.slot[slot].r) lora_dirty_[kv.second.ti] = 1;
    return 0;
}

int UNet::lora_apply(hipStream_t stream) {
    LAVIE_CHECK(finalized_, "lora_apply: call lavie_unet_finalize first");
    bool any = false;
    for (char d : lora_dirty_) any = any || d;
    if (!any) return 0;
    bool drop = false;
    for (auto& kv : lora_) {
        const LoraEntry& e = kv.second;
        if (!lora_dirty_[e.ti]) continue;
        // the terms of this target: its slots in ascending order, factor (global * weight) * scale in fp32; a zero factor is no term
        LoraTerm terms[kLoraMaxTerms];
        int n = 0;
        for (int i = 0; i < kLoraMaxTerms; ++i) {
            const LoraSlot& s = e.slot[i];
            if (s.r == 0) continue;
            const float gw = lora_scale_ * lora_weight_[i];
            const float eff = gw * s.scale;
            if (eff != 0.f) terms[n++] = LoraTerm{s.A, s.B, s.r, eff};
        }
        if (n == 1) RUN(launch_lora_merge(e.base, terms[0].A, terms[0].B, e.dst, e.N, e.K, terms[0].r, terms[0].scale, stream));
        else if (n > 1) RUN(launch_lora_merge_multi(e.base, terms, n, e.dst, e.N, e.K, stream));
        else LAVIE_HIP(hipMemcpyAsync(e.dst, e.base, (size_t)e.N * e.K * sizeof(half_t), hipMemcpyDeviceToDevice, stream));
        drop = drop || e.empty();
    }
    for (size_t i = 0; i < transformers_.size(); ++i)
        if (lora_dirty_[i]) RUN(derive_transformer(transformers_[i], stream));
    if (drop) {                 // cleared entries: their base is back in place
        LAVIE_HIP(hipStreamSynchronize(stream));
        for (auto it = lora_.begin(); it != lora_.end();) {
            if (it->second.empty()) {
                for (LoraSlot& s : it->second.slot) lora_free(s);      // a buffer a failed registration left behind
                (void)hipFree(it->second.base);
                it = lora_.erase(it);
            }
            else ++it;
        }
    }
    lora_dirty_.assign(transformers_.size(), 0);
    ++graph_gen_;
    // a cached context holds text K / V (and the fused kernel's per-video images) computed from the old attn2 weights: recompute
    // them into the same buffers from the tensor the cache_context contract keeps alive and unmodified
    if (kv_ctx_) RUN(cache_context(kv_ctx_, kv_B_, kv_len_, stream));
    return 0;
}

int UNet::resnet_forward(const char* prefix, const half_t* x1, int C1, const half_t* x2, int C2, const float* temb, half_t* y,
                         int B, int F, int H, int W, hipStream_t stream) {
    LAVIE_CHECK(finalized_, "resnet_forward: call lavie_unet_finalize first");
    const ResnetW* r = nullptr;
    for (const ResnetW& cand : resnets_) if (cand.prefix == prefix) r = &cand;
    LAVIE_CHECK(r != nullptr, "resnet_forward: no ResnetBlock3D with prefix '%s'", prefix);
    // standalone call: private workspace sized on the fly (test seam, not the hot path)
    DeviceArena local;
    const size_t M = (size_t)B * F * H * W;
    RUN(local.init_fixed((M * (r->cin + 2 * r->cout)) * sizeof(half_t) + (size_t)B * r->cout * 4 + colstat_floats(M, r->cout) * sizeof(float) + (4 << 20)));
    FwdCtx c = call_ctx(stream, &local, B, F, H, W, nullptr, 0, /*pag (attn1 only)=*/0);
    c.gn_ws = (float*)local.alloc(gn_workspace_floats(B * F, cfg_.norm_groups) * sizeof(float));
    float* tproj = (float*)local.alloc((size_t)B * r->cout * sizeof(float));
    RUN(launch_gemv(temb, tproj_.w + (size_t)r->temb_off * tproj_.K, tproj_.b + r->temb_off, tproj, B, r->cout, tproj_.K, 1, 0, stream));
    const Act a1{const_cast<half_t*>(x1), C1}, a2{const_cast<half_t*>(x2), C2};      // (no producer statistics in, none asked for out)
    Act ay{y, r->cout};
    RUN(run_resnet(c, *r, a1, C2 ? &a2 : nullptr, tproj, r->cout, &ay, H, W));
    LAVIE_HIP(hipStreamSynchronize(stream));     // the private workspace dies with this frame
    return 0;
}

int UNet::transformer_forward(const char* prefix, half_t* x, const half_t* ctx, int B, int F, int H, int W, int ctx_len,
                              hipStream_t stream) {
    LAVIE_CHECK(finalized_, "transformer_forward: call lavie_unet_finalize first");
    const TransformerW* t = nullptr;
    for (const TransformerW& cand : transformers_) if (cand.prefix == prefix) t = &cand;
    LAVIE_CHECK(t != nullptr, "transformer_forward: no Transformer3DModel with prefix '%s'", prefix);
    LAVIE_CHECK(F >= 1 && F <= 64, "transformer_forward: F=%d unsupported", F);
    const int pag = pag_route("transformer_forward", B);
    if (pag < 0) return -1;
    RUN(ensure_tables(F, stream));
    DeviceArena local;
    const size_t T = (size_t)B * F * H * W;
    RUN(local.init_fixed(T * t->C * 7 * sizeof(half_t) + (size_t)B * ctx_len * 2 * t->C * sizeof(half_t) + (4 << 20)));
    FwdCtx c = call_ctx(stream, &local, B, F, H, W, ctx, ctx_len, pag);
    c.gn_ws = (float*)local.alloc(gn_workspace_floats(B * F, cfg_.norm_groups) * sizeof(float));
    Act ax{x, t->C};
    RUN(run_transformer(c, *t, ax, ctx, H, W));
    LAVIE_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace lavie
