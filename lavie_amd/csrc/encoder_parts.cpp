#include "encoder_parts.h"

#include <math.h>

#include "ops.h"

namespace lavie {

int check_clip_shape(const char* who, const ClipShape& c) {
    LAVIE_CHECK(c.hidden >= kPinBn && c.hidden % kPinBn == 0 && c.hidden <= 2048, "%s: hidden=%d must be a multiple of %d up to 2048", who,
                c.hidden, kPinBn);
    LAVIE_CHECK(c.intermediate >= kPinBn && c.intermediate % kPinBn == 0 && c.intermediate <= 16384,
                "%s: intermediate=%d must be a multiple of %d up to 16384", who, c.intermediate, kPinBn);
    LAVIE_CHECK(c.layers >= 1 && c.layers <= 64, "%s: layers=%d must be 1..64", who, c.layers);
    LAVIE_CHECK(c.heads >= 1 && c.hidden % c.heads == 0 && (c.hidden / c.heads == 32 || c.hidden / c.heads == 64),
                "%s: heads=%d gives a head dim of hidden / heads that is not 32 or 64 (hidden=%d)", who, c.heads, c.hidden);
    LAVIE_CHECK(c.act == LAVIE_TEXT_ACT_QUICK_GELU || c.act == LAVIE_TEXT_ACT_GELU, "%s: act=%d is neither quick_gelu (0) nor gelu (1)", who,
                c.act);
    LAVIE_CHECK(isfinite(c.eps) && c.eps > 0.f, "%s: eps must be finite and > 0", who);
    return 0;
}

void list_clip_layer(ParamTable& t, const std::string& p, const ClipShape& c) {
    const long long C = c.hidden, I = c.intermediate;
    for (const char* proj : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
        t.add(p + "self_attn." + proj + ".weight", C * C);
        t.add(p + "self_attn." + proj + ".bias", C);
    }
    t.add(p + "layer_norm1.weight", C);
    t.add(p + "layer_norm1.bias", C);
    t.add(p + "mlp.fc1.weight", I * C);
    t.add(p + "mlp.fc1.bias", I);
    t.add(p + "mlp.fc2.weight", C * I);
    t.add(p + "mlp.fc2.bias", C);
    t.add(p + "layer_norm2.weight", C);
    t.add(p + "layer_norm2.bias", C);
}

void carve_clip_layer(Carver& c, ClipLayer& l, const ClipShape& sh) {
    const size_t C = sh.hidden, I = sh.intermediate;
    l.wqkv = c.take<half_t>(3 * C * C);
    l.wo = c.take<half_t>(C * C);
    l.w1 = c.take<half_t>(I * C);
    l.w2 = c.take<half_t>(C * I);
    l.bqkv = c.take<float>(3 * C);
    l.bo = c.take<float>(C);
    l.b1 = c.take<float>(I);
    l.b2 = c.take<float>(C);
    l.ln1g = c.take<float>(C);
    l.ln1b = c.take<float>(C);
    l.ln2g = c.take<float>(C);
    l.ln2b = c.take<float>(C);
}

int pack_clip_layer(const ParamTable& t, const std::string& p, const ClipLayer& l, const ClipShape& c, hipStream_t s) {
    const size_t C = c.hidden, I = c.intermediate;
    auto to16 = [&](half_t* dst, const std::string& n, size_t count) { return copy16(dst, t.src(p + n), count, s); };
    auto to32 = [&](float* dst, const std::string& n, size_t count) { return launch_f16_to_f32(t.src(p + n), dst, (int64_t)count, s); };
    const char* qkv[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
        RUN(to16(l.wqkv + j * C * C, std::string("self_attn.") + qkv[j] + ".weight", C * C));
        RUN(to32(l.bqkv + j * C, std::string("self_attn.") + qkv[j] + ".bias", C));
    }
    RUN(to16(l.wo, "self_attn.out_proj.weight", C * C));
    RUN(to32(l.bo, "self_attn.out_proj.bias", C));
    RUN(to16(l.w1, "mlp.fc1.weight", I * C));
    RUN(to32(l.b1, "mlp.fc1.bias", I));
    RUN(to16(l.w2, "mlp.fc2.weight", C * I));
    RUN(to32(l.b2, "mlp.fc2.bias", C));
    RUN(to32(l.ln1g, "layer_norm1.weight", C));
    RUN(to32(l.ln1b, "layer_norm1.bias", C));
    RUN(to32(l.ln2g, "layer_norm2.weight", C));
    RUN(to32(l.ln2b, "layer_norm2.bias", C));
    return 0;
}

ClipWorkspace carve_clip_workspace(Carver& c, size_t M, const ClipShape& sh) {
    const size_t C = sh.hidden, I = sh.intermediate;
    ClipWorkspace w;
    w.x = c.take<half_t>(M * C);
    w.h = c.take<half_t>(M * C);
    w.wide = c.take<half_t>(M * (3 * C > I ? 3 * C : I));
    return w;
}

int run_clip_layer(const ClipLayer& l, const ClipShape& c, const ClipWorkspace& w, int B, int T, bool causal, half_t* dst, hipStream_t s) {
    const int M = B * T, C = c.hidden, I = c.intermediate, dh = C / c.heads;
    const float scale = 1.0f / sqrtf((float)dh);
    half_t *x = w.x, *h = w.h, *wide = w.wide;
    RUN(launch_layernorm(x, l.ln1g, l.ln1b, h, M, C, c.eps, s));
    RUN(pinned_linear(h, l.wqkv, l.bqkv, nullptr, wide, M, 3 * C, C, s));
    if (causal)
        RUN(launch_causal_attention(wide, 3 * C, h, C, B, T, c.heads, dh, scale, s));
    else
        RUN(launch_short_attention(wide, 3 * C, wide + C, 3 * C, wide + 2 * C, 3 * C, h, C, B, T, T, c.heads, dh, scale, false, s));
    RUN(pinned_linear(h, l.wo, l.bo, x, x, M, C, C, s));
    RUN(launch_layernorm(x, l.ln2g, l.ln2b, h, M, C, c.eps, s));
    RUN(pinned_linear(h, l.w1, l.b1, nullptr, wide, M, I, C, s));
    RUN(launch_act(wide, (int64_t)M * I, c.act, s));
    return pinned_linear(wide, l.w2, l.b2, x, dst, M, C, I, s);
}

}  // namespace lavie
