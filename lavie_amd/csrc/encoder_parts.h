// What the weight-holding objects behind lavie_text_*, lavie_vision_* and lavie_mapper_* share beyond weight_parts.h (DESIGN.md 7.16,
// 7.17): the CLIP pre-LN layer of the text encoder and the vision tower.
#pragma once
#include "../../include/lavie_hip.h"
#include "pinned_linear.h"
#include "weight_parts.h"

namespace lavie {

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
