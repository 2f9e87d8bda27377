// `make asan` driver: walks the C ABI of the host-only sanitizer build (hip_stub.cpp) the way the Python facade does:
// create -> parameter inventory -> set_param -> finalize (weight packing, arena carving) -> prepare (workspace dry run over every
// switch combination) -> cache_context -> forward (sequencing + every launcher's host side) -> error paths -> destroy, for the
// base, interpolation and VSR variants of the engine at reduced widths.  Exit code 0 and a silent sanitizer = pass.
// `hostcheck trace FILE` instead writes the launch trace of the cases in run_traces() to FILE (tests/golden/make_golden_trace.py).
// `hostcheck optrace IN OUT` replays the operator calls listed in IN (run_optrace()) and writes their launches to OUT;
// `hostcheck kernels OUT` lists every registered kernel name (tests/opcases.py: gemm_reach()).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../../include/lavie_hip.h"

extern "C" long lavie_hostcheck_launches();
extern "C" long lavie_hostcheck_last_grid_x();
extern "C" void lavie_hostcheck_trace_to(FILE* f);
extern "C" void lavie_hostcheck_trace_copies(int on);
extern "C" void lavie_hostcheck_kernel_names_to(FILE* f);

#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "hostcheck: %s failed at line %d: %s\n", #cond, __LINE__, lavie_last_error()); \
            exit(2);                                                                           \
        }                                                                                      \
    } while (0)

static lavie_unet_config base_config() {
    lavie_unet_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = (int)sizeof(c);
    c.in_channels = 4; c.out_channels = 4; c.num_levels = 2;
    c.block_out_channels[0] = 320; c.block_out_channels[1] = 640;
    c.attn_levels[0] = 1; c.attn_levels[1] = 0;
    c.layers_per_block = 2; c.heads = 8; c.cross_attention_dim = 128; c.norm_groups = 32; c.norm_eps = 1e-5f;
    c.rotary_dim = 32; c.rel_buckets = 32; c.rel_max_distance = 32;
    return c;
}

static void run_model(const lavie_unet_config& cfg, int B, int F, int H, int W, bool labels, bool check_switches = false) {
    lavie_unet_t h = nullptr;
    REQUIRE(lavie_unet_create(&cfg, &h) == 0);
    const int n = lavie_unet_num_params(h);
    REQUIRE(n > 0);
    std::vector<void*> bufs;
    for (int i = 0; i < n; ++i) {
        const char* name = nullptr;
        long long numel = 0;
        REQUIRE(lavie_unet_param_info(h, i, &name, &numel) == 0 && name && numel > 0);
        void* p = calloc((size_t)numel, 2);          // exact size: an over-long packing copy trips ASan
        bufs.push_back(p);
        REQUIRE(lavie_unet_set_param(h, name, p, numel) == 0);
        if (i == 0) {                                // argument checks of set_param
            REQUIRE(lavie_unet_set_param(h, name, p, numel + 1) != 0);
            REQUIRE(lavie_unet_set_param(h, "no.such.key", p, numel) != 0);
            REQUIRE(lavie_unet_set_param(h, name, nullptr, numel) != 0);
        }
    }
    REQUIRE(lavie_unet_param_info(h, n, nullptr, nullptr) != 0);
    REQUIRE(lavie_unet_prepare(h, B, F, H, W, 77) != 0);              // before finalize: refused
    REQUIRE(lavie_unet_finalize(h, nullptr) == 0);
    REQUIRE(lavie_unet_finalize(h, nullptr) != 0);                    // twice: refused
    REQUIRE(lavie_unet_prepare(h, B, F, H + 1, W, 77) != 0);          // not a multiple of 2^(levels-1)
    REQUIRE(lavie_unet_prepare(h, B, F, H, W, 77) == 0);
    REQUIRE(lavie_unet_workspace_bytes(h) > 0 && lavie_unet_weight_bytes(h) > 0);
    const size_t in_elems = (size_t)B * cfg.in_channels * F * H * W, out_elems = (size_t)B * cfg.out_channels * F * H * W;
    void* x = calloc(in_elems, 2);
    void* y = calloc(out_elems, 2);
    void* ctx = calloc((size_t)B * 77 * cfg.cross_attention_dim, 2);
    float* t = (float*)calloc(B, sizeof(float));
    std::vector<int> lab(B, 3);
    const long before = lavie_hostcheck_launches();
    if (labels) {
        REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) != 0);        // class-embedded model needs labels
        REQUIRE(lavie_unet_forward_labels(h, x, t, ctx, lab.data(), y, B, F, H, W, 77, nullptr) == 0);
    } else {
        REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) == 0);
        REQUIRE(lavie_unet_cache_context(h, ctx, B, 77, nullptr) == 0);
        REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) == 0);
        if (B % 2 == 0 && !cfg.sparse_causal_attn1 && !cfg.vsr_blocks) {
            REQUIRE(lavie_unet_set_cfg_shared_input(h, 1) == 0);
            REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) == 0);
            REQUIRE(lavie_unet_set_cfg_shared_input(h, 0) == 0);
        } else {
            REQUIRE(lavie_unet_set_cfg_shared_input(h, 1) == 0);
            REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) != 0);    // the switch cannot apply: an error, not a guess
            REQUIRE(lavie_unet_set_cfg_shared_input(h, 0) == 0);
        }
        REQUIRE(lavie_unet_cache_context(h, nullptr, 0, 0, nullptr) == 0);
        // a 154-token context (77 text + 77 mapped image tokens): long templates built on first use, long images bound, the
        // long fused text cross-attention where level 0 has it; then back to 77 tokens on the same buffers
        void* ctx2 = calloc((size_t)B * 154 * cfg.cross_attention_dim, 2);
        REQUIRE(lavie_unet_prepare(h, B, F, H, W, 154) == 0);
        REQUIRE(lavie_unet_cache_context(h, ctx2, B, 154, nullptr) == 0);
        REQUIRE(lavie_unet_forward(h, x, t, ctx2, y, B, F, H, W, 154, nullptr) == 0);
        REQUIRE(lavie_unet_cache_context(h, ctx, B, 77, nullptr) == 0);
        REQUIRE(lavie_unet_prepare(h, B, F, H, W, 77) == 0);
        REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) == 0);
        REQUIRE(lavie_unet_cache_context(h, nullptr, 0, 0, nullptr) == 0);
        free(ctx2);
    }
    REQUIRE(lavie_hostcheck_launches() > before + 50);
    {   // FreeU: decoder-only launches in front of the resnets of up blocks 0 and 1, inside the workspace prepare() planned; a refused
        // value leaves the setting in force; (1, 1, 1, 1) is the plain forward again
        auto launches = [&]() {
            const long b = lavie_hostcheck_launches();
            REQUIRE((labels ? lavie_unet_forward_labels(h, x, t, ctx, lab.data(), y, B, F, H, W, 77, nullptr)
                            : lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr)) == 0);
            return lavie_hostcheck_launches() - b;
        };
        const long long ws_bytes = lavie_unet_workspace_bytes(h);
        const long off = launches();
        REQUIRE(lavie_unet_set_freeu(h, 0.9f, 0.2f, 1.5f, 1.6f) == 0);
        const long on = launches();
        REQUIRE(on > off);
        REQUIRE(lavie_unet_set_freeu(h, 0.f, 0.2f, 1.5f, 1.6f) != 0 && lavie_unet_set_freeu(h, 0.9f, -1.f, 1.5f, 1.6f) != 0 &&
                lavie_unet_set_freeu(h, 0.9f, 0.2f, NAN, 1.6f) != 0 && lavie_unet_set_freeu(h, 0.9f, 0.2f, 1.5f, INFINITY) != 0 &&
                lavie_unet_set_freeu(nullptr, 1.f, 1.f, 1.f, 1.f) != 0);
        REQUIRE(launches() == on);
        REQUIRE(lavie_unet_set_freeu(h, 1.f, 1.f, 1.5f, 1.f) == 0);     // b1 alone: stage 0's apply launches, no sums, stage 1 nothing
        const long b1_only = launches();
        REQUIRE(b1_only > off && b1_only < on);
        REQUIRE(lavie_unet_set_freeu(h, 1.f, 1.f, 1.f, 1.f) == 0);
        REQUIRE(launches() == off);
        REQUIRE(lavie_unet_workspace_bytes(h) == ws_bytes);
    }
    {   // perturbed-attention guidance: one strided row copy more per selected transformer, inside the workspace prepare() planned; a
        // refused call names its argument and leaves the setting in force; off is the plain forward again
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        auto forward = [&]() {
            return labels ? lavie_unet_forward_labels(h, x, t, ctx, lab.data(), y, B, F, H, W, 77, nullptr)
                          : lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr);
        };
        auto launches = [&]() {
            const long b = lavie_hostcheck_launches();
            REQUIRE(forward() == 0);
            return lavie_hostcheck_launches() - b;
        };
        const char* mid[1] = {"mid_block"};
        const char* two[2] = {"mid_block", "down_blocks.0.attentions.1"};
        const char* almost[1] = {"mid_bloc"};               // a prefix of the name, but not up to a '.'
        const char* level0[1] = {"down_blocks.0"};
        const char* empty[1] = {""};
        const long long ws_bytes = lavie_unet_workspace_bytes(h);
        const long off = launches();
        REQUIRE(refused(lavie_unet_set_pag(nullptr, mid, 1, 1), "null handle"));
        REQUIRE(refused(lavie_unet_set_pag(h, mid, 1, -1), "perturbed=-1"));
        REQUIRE(refused(lavie_unet_set_pag(h, almost, 1, 1), "selects no transformer"));
        REQUIRE(refused(lavie_unet_set_pag(h, empty, 1, 1), "layers_host[0]"));
        REQUIRE(refused(lavie_unet_set_pag(h, nullptr, 1, 1), "layers_host"));
        REQUIRE(refused(lavie_unet_set_pag(h, mid, -1, 1), "n_layers=-1"));
        REQUIRE(launches() == off);
        if (cfg.sparse_causal_attn1) {
            REQUIRE(refused(lavie_unet_set_pag(h, mid, 1, 1), "plain spatial self-attention"));
            REQUIRE(launches() == off);
        } else {
            if (cfg.vsr_blocks && cfg.only_cross_attention[0])       // attn1 of that level attends to the text
                REQUIRE(refused(lavie_unet_set_pag(h, level0, 1, 1), "plain spatial self-attention"));
            REQUIRE(lavie_unet_set_pag(h, mid, 1, 1) == 0);
            if (B > 1) {
                REQUIRE(launches() == off + 1);
                REQUIRE(refused(lavie_unet_set_pag(h, almost, 1, 1), "selects no transformer") && launches() == off + 1);
                REQUIRE(lavie_unet_set_cfg_shared_input(h, 1) == 0);          // ignored while PAG is on
                REQUIRE(launches() == off + 1);
                REQUIRE(lavie_unet_set_cfg_shared_input(h, 0) == 0);
                if (!cfg.vsr_blocks) {
                    REQUIRE(lavie_unet_set_pag(h, two, 2, 1) == 0);
                    REQUIRE(launches() == off + 2);
                }
                REQUIRE(lavie_unet_set_pag(h, mid, 1, B) == 0);
            }
            REQUIRE(refused(forward(), "perturbed="));                        // B <= perturbed
            REQUIRE(lavie_unet_set_pag(h, mid, 1, 0) == 0);                   // perturbed == 0: off
            REQUIRE(launches() == off);
            REQUIRE(lavie_unet_set_pag(h, mid, 1, 1) == 0 && lavie_unet_set_pag(h, nullptr, 0, 0) == 0);
            REQUIRE(launches() == off);
        }
        REQUIRE(lavie_unet_workspace_bytes(h) == ws_bytes);
    }
    if (check_switches) {   // a rejected switch value leaves the one in force: the launch count of a forward tells them apart
        auto launches = [&]() {
            const long b = lavie_hostcheck_launches();
            REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) == 0);
            return lavie_hostcheck_launches() - b;
        };
        const long def = launches();
        REQUIRE(lavie_debug_fused_mask(0x30) == 0);                  // without the row-resident kernels (a combination prepare() plans)
        const long plain = launches();
        REQUIRE(plain != def);
        REQUIRE(lavie_debug_fused_mask(0x08) != 0 && lavie_debug_fused_mask(0x30 | 0x80) != 0 && lavie_debug_fused_mask(0x200) != 0);
        REQUIRE(launches() == plain);
        REQUIRE(lavie_debug_fused_mask(0x137) == 0);
        REQUIRE(launches() == def);
        REQUIRE(lavie_debug_force_tile(3) == 0);                     // ping-pong kernel wherever N % 320 == 0: other split-K plans
        REQUIRE(lavie_unet_prepare(h, B, F, H, W, 77) == 0);
        const long pp = launches();
        REQUIRE(pp != def);
        REQUIRE(lavie_debug_force_tile(0x75) != 0 && lavie_debug_force_tile(10) != 0 && lavie_debug_force_tile(-1) != 0);
        REQUIRE(launches() == pp);
        REQUIRE(lavie_debug_force_tile(0) == 0);
        REQUIRE(launches() == def);
    }
    {   // the adapter registry's slots on two square targets: two adapters of different rank share one target and one base copy, a
        // re-weight, a slot replaced by another rank, slots cleared one by one (the entry and its base go with the last), the
        // refusals; exactly sized buffers, so an over-long copy or a leaked / twice-freed slot is the sanitizers' to find
        std::string tq, to;
        long long nq = 0;
        for (int i = 0; i < n; ++i) {
            const char* name = nullptr;
            long long numel = 0;
            REQUIRE(lavie_unet_param_info(h, i, &name, &numel) == 0);
            const std::string s = name;
            const auto ends = [&](const char* e) { return s.size() > strlen(e) && s.compare(s.size() - strlen(e), strlen(e), e) == 0; };
            if (tq.empty() && ends("attn1.to_q.weight")) { tq = s; nq = numel; }
            if (to.empty() && ends("attn1.to_out.0.weight")) to = s;
        }
        REQUIRE(!tq.empty() && !to.empty());
        int C = 1;
        while ((long long)C * C < nq) ++C;
        REQUIRE((long long)C * C == nq);
        std::vector<unsigned short> w0((size_t)C * C);
        std::vector<float> a16((size_t)16 * C), b16((size_t)C * 16), a3((size_t)3 * C), b3((size_t)C * 3);
        const long b0 = lavie_hostcheck_launches();
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0 && lavie_hostcheck_launches() == b0);       // nothing to do: no launch
        REQUIRE(lavie_unet_lora_set(h, tq.c_str(), w0.data(), a16.data(), b16.data(), 16, 1.f, nullptr) == 0);      // slot 0
        REQUIRE(lavie_unet_lora_set_slot(h, 3, tq.c_str(), w0.data(), a3.data(), b3.data(), 3, 0.5f, nullptr) == 0);
        REQUIRE(lavie_unet_lora_set_slot(h, 3, to.c_str(), w0.data(), a3.data(), b3.data(), 3, 0.5f, nullptr) == 0);
        REQUIRE(lavie_unet_lora_set_slot_weight(h, 3, -0.5f) == 0);
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0);
        const long per_apply = lavie_hostcheck_launches() - b0;
        REQUIRE(per_apply >= 2);
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0 && lavie_hostcheck_launches() == b0 + per_apply);
        REQUIRE(lavie_unet_lora_set_slot_weight(h, 3, -0.5f) == 0);                                  // unchanged: nothing dirty
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0 && lavie_hostcheck_launches() == b0 + per_apply);
        REQUIRE(lavie_unet_lora_set_slot_weight(h, 5, 2.f) == 0);                                    // an empty slot: nothing dirty
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0 && lavie_hostcheck_launches() == b0 + per_apply);
        REQUIRE(lavie_unet_lora_set_slot_weight(h, 3, 0.f) == 0);                                    // off, resident: one term on tq
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0 && lavie_hostcheck_launches() > b0 + per_apply);
        REQUIRE(lavie_unet_lora_set_slot(h, 3, tq.c_str(), w0.data(), a16.data(), b16.data(), 16, 1.f, nullptr) == 0);   // another rank
        REQUIRE(lavie_unet_lora_set_slot_weight(h, 3, 1.f) == 0);
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0);
        REQUIRE(lavie_unet_lora_set_slot(h, -1, tq.c_str(), w0.data(), a3.data(), b3.data(), 3, 1.f, nullptr) != 0);
        REQUIRE(lavie_unet_lora_set_slot(h, 8, tq.c_str(), w0.data(), a3.data(), b3.data(), 3, 1.f, nullptr) != 0);
        REQUIRE(lavie_unet_lora_set_slot(h, 1, tq.c_str(), w0.data(), a3.data(), b3.data(), 129, 1.f, nullptr) != 0);
        REQUIRE(lavie_unet_lora_set_slot(h, 1, "conv_in.weight", w0.data(), a3.data(), b3.data(), 3, 1.f, nullptr) != 0);
        REQUIRE(lavie_unet_lora_set_slot_weight(h, 8, 1.f) != 0 && lavie_unet_lora_set_slot_weight(h, 1, __builtin_nanf("")) != 0);
        REQUIRE(lavie_unet_lora_clear_slot(h, 8, nullptr, nullptr) != 0);
        REQUIRE(lavie_unet_lora_clear(h, nullptr, nullptr) == 0);                                    // slot 0 only
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0);
        REQUIRE(lavie_unet_lora_clear_slot(h, 3, tq.c_str(), nullptr) == 0);                         // tq's last slot: its entry goes
        REQUIRE(lavie_unet_lora_apply(h, nullptr) == 0);
        if (!labels) REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H, W, 77, nullptr) == 0);
        // slot 3 still holds `to`: the destructor frees what is left
    }
    REQUIRE(lavie_unet_forward(h, x, t, ctx, y, B, F, H * 2, W * 2, 77, nullptr) != 0);    // larger than prepared: workspace refuses
    REQUIRE(lavie_unet_forward(h, nullptr, t, ctx, y, B, F, H, W, 77, nullptr) != 0);
    REQUIRE(lavie_unet_forward(h, x, t, ctx, y, 9, F, H, W, 77, nullptr) != 0);
    REQUIRE(lavie_unet_destroy(h) == 0);
    free(x); free(y); free(ctx); free(t);
    for (void* p : bufs) free(p);
}

// ---- launch trace (hip_stub.cpp): every launch of the cases below, each case headed by a "== name" line
static FILE* g_out = nullptr;
__attribute__((format(printf, 1, 2))) static void trace_case(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(g_out, "== ");
    vfprintf(g_out, fmt, ap);
    fprintf(g_out, "\n");
    va_end(ap);
}

struct Model {      // a finalized engine with zero weights
    lavie_unet_t h = nullptr;
    std::vector<void*> bufs;
    explicit Model(const lavie_unet_config& cfg) {
        REQUIRE(lavie_unet_create(&cfg, &h) == 0);
        const int n = lavie_unet_num_params(h);
        for (int i = 0; i < n; ++i) {
            const char* name = nullptr;
            long long numel = 0;
            REQUIRE(lavie_unet_param_info(h, i, &name, &numel) == 0);
            bufs.push_back(calloc((size_t)numel, 2));
            REQUIRE(lavie_unet_set_param(h, name, bufs.back(), numel) == 0);
        }
        REQUIRE(lavie_unet_finalize(h, nullptr) == 0);
    }
    ~Model() {
        REQUIRE(lavie_unet_destroy(h) == 0);
        for (void* p : bufs) free(p);
    }
};

// A handle that lacks one tensor: finalize refuses it by name before anything is allocated; with the tensor supplied, the second
// finalize enqueues exactly what the finalize of a handle that was complete from the start enqueues.  The `...rotary_emb.freqs`
// keys are never sent to it: they are listed, and nothing asks for them.
static void run_withheld_tensor(const lavie_unet_config& cfg, const char* withheld) {
    auto trace_of = [](const std::function<void()>& body) {
        FILE* f = tmpfile();
        REQUIRE(f != nullptr);
        lavie_hostcheck_trace_to(f);
        lavie_hostcheck_trace_copies(1);
        body();
        lavie_hostcheck_trace_copies(0);
        lavie_hostcheck_trace_to(nullptr);
        std::string text((size_t)ftell(f), '\0');
        rewind(f);
        REQUIRE(fread(&text[0], 1, text.size(), f) == text.size());
        fclose(f);
        return text;
    };
    const std::string complete = trace_of([&] { Model m(cfg); });
    REQUIRE(!complete.empty());
    lavie_unet_t h = nullptr;
    REQUIRE(lavie_unet_create(&cfg, &h) == 0);
    std::vector<void*> bufs;
    void* late = nullptr;
    long long late_numel = 0;
    for (int i = 0; i < lavie_unet_num_params(h); ++i) {
        const char* name = nullptr;
        long long numel = 0;
        REQUIRE(lavie_unet_param_info(h, i, &name, &numel) == 0);
        const size_t len = strlen(name);
        if (len >= 16 && strcmp(name + len - 16, "rotary_emb.freqs") == 0) continue;
        bufs.push_back(calloc((size_t)numel, 2));
        if (strcmp(name, withheld) == 0) {
            late = bufs.back();
            late_numel = numel;
        } else {
            REQUIRE(lavie_unet_set_param(h, name, bufs.back(), numel) == 0);
        }
    }
    REQUIRE(late != nullptr);
    const long before = lavie_hostcheck_launches();
    REQUIRE(lavie_unet_finalize(h, nullptr) != 0 && strstr(lavie_last_error(), "was never set") && strstr(lavie_last_error(), withheld));
    REQUIRE(lavie_unet_weight_bytes(h) == 0 && lavie_hostcheck_launches() == before);
    REQUIRE(lavie_unet_set_param(h, withheld, late, late_numel) == 0);
    const std::string second = trace_of([&] { REQUIRE(lavie_unet_finalize(h, nullptr) == 0); });
    REQUIRE(second == complete);
    REQUIRE(lavie_unet_weight_bytes(h) > 0);
    REQUIRE(lavie_unet_destroy(h) == 0);
    for (void* p : bufs) free(p);
}

// prepare for the shape (the switches in force decide the workspace plan; its size is recorded), then one forward: cached context
// and shared classifier-free-guidance prefix where the variant allows them, labels for a class-embedded model
static void trace_forward(const lavie_unet_config& cfg, Model& m, int B, int F, int H, int W, bool cached, bool shared, int ctx_len = 77) {
    REQUIRE(lavie_unet_prepare(m.h, B, F, H, W, ctx_len) == 0);
    fprintf(g_out, "workspace %lld\n", lavie_unet_workspace_bytes(m.h));
    std::vector<unsigned short> x((size_t)B * cfg.in_channels * F * H * W), y((size_t)B * cfg.out_channels * F * H * W);
    std::vector<unsigned short> ctx((size_t)B * ctx_len * cfg.cross_attention_dim);
    std::vector<float> t(B, 500.f);
    std::vector<int> lab(B, 3);
    if (cached) REQUIRE(lavie_unet_cache_context(m.h, ctx.data(), B, ctx_len, nullptr) == 0);
    REQUIRE(lavie_unet_set_cfg_shared_input(m.h, shared ? 1 : 0) == 0);
    const int rc = cfg.num_class_embeds
                       ? lavie_unet_forward_labels(m.h, x.data(), t.data(), ctx.data(), lab.data(), y.data(), B, F, H, W, ctx_len, nullptr)
                       : lavie_unet_forward(m.h, x.data(), t.data(), ctx.data(), y.data(), B, F, H, W, ctx_len, nullptr);
    if (rc != 0) {       // a launch the library refuses ends the forward: recorded, the message goes to stderr
        fprintf(g_out, "!! forward refused\n");
        fprintf(stderr, "hostcheck trace: forward refused: %s\n", lavie_last_error());
    }
    REQUIRE(lavie_unet_set_cfg_shared_input(m.h, 0) == 0);
    if (cached) REQUIRE(lavie_unet_cache_context(m.h, nullptr, 0, 0, nullptr) == 0);
}

// the operator entry points at level shapes of the base model (B * F = 32 frames of 40 x 64 latents); tensors are never read
static void trace_operators() {
    static std::vector<unsigned short> buf(64);
    void* d = buf.data();
    const int lin[][3] = {{81920, 320, 320}, {81920, 960, 320}, {81920, 320, 1280}, {20480, 640, 640}, {20480, 640, 2560},
                          {5120, 1280, 1280}, {5120, 3840, 1280}, {5120, 1280, 5120}, {2464, 1280, 768}};
    for (const auto& s : lin) {
        trace_case("op linear M=%d N=%d K=%d", s[0], s[1], s[2]);
        REQUIRE(lavie_linear_f16(d, s[2], d, nullptr, nullptr, 0, 0, nullptr, 0, d, s[1], s[0], s[1], s[2], 0, nullptr) == 0);
        REQUIRE(lavie_linear_f16(d, s[2], d, nullptr, nullptr, 0, 0, d, s[1], d, s[1], s[0], s[1], s[2], 0, nullptr) == 0);
    }
    const int geglu[][3] = {{81920, 2560, 320}, {20480, 5120, 640}, {5120, 10240, 1280}};
    for (const auto& s : geglu) {
        trace_case("op geglu M=%d N=%d K=%d", s[0], s[1], s[2]);
        REQUIRE(lavie_linear_f16(d, s[2], d, nullptr, nullptr, 0, 0, nullptr, 0, d, s[1] / 2, s[0], s[1], s[2], 1, nullptr) == 0);
    }
    // {H, W, C1, C2 (skip), SC1 (shortcut), Cout, stride, ups}
    const int conv[][8] = {{40, 64, 320, 0, 0, 320, 1, 0},   {40, 64, 320, 320, 0, 320, 1, 0}, {40, 64, 640, 320, 640, 320, 1, 0},
                           {40, 64, 320, 0, 0, 320, 2, 0},   {20, 32, 640, 0, 0, 640, 1, 0},   {20, 32, 1280, 640, 0, 640, 1, 0},
                           {10, 16, 1280, 0, 0, 1280, 1, 0}, {10, 16, 1280, 0, 0, 1280, 2, 0}, {5, 8, 1280, 0, 0, 1280, 1, 0},
                           {5, 8, 1280, 0, 0, 1280, 1, 1},   {20, 32, 640, 0, 0, 640, 1, 1}};
    for (const auto& s : conv) {
        trace_case("op conv3x3 %dx%d C=%d+%d shortcut=%d Cout=%d stride=%d ups=%d", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
        REQUIRE(lavie_conv3x3_f16(d, s[2], s[3] ? d : nullptr, s[3], s[4] ? d : nullptr, s[4], nullptr, 0, d, nullptr, nullptr, 0, 1,
                                  nullptr, d, 32, s[0], s[1], s[5], s[6], s[7], d, nullptr) == 0);
    }
    const int ups[][3] = {{5, 8, 1280}, {10, 16, 1280}, {20, 32, 640}};
    for (const auto& s : ups) {
        trace_case("op upsample_conv3x3 %dx%d C=%d", s[0], s[1], s[2]);
        REQUIRE(lavie_upsample_conv3x3_f16(d, d, nullptr, d, 32, s[0], s[1], s[2], d, nullptr) == 0);
    }
}

static lavie_unet_config production_config() {        // the base model: 4 levels 320 / 640 / 1280 / 1280
    lavie_unet_config c = base_config();
    c.num_levels = 4;
    const int w[4] = {320, 640, 1280, 1280}, a[4] = {1, 1, 1, 0};
    for (int i = 0; i < 4; ++i) { c.block_out_channels[i] = w[i]; c.attn_levels[i] = a[i]; }
    c.cross_attention_dim = 768;
    return c;
}

// The layer cache's entries: argument refusals, the states in which a reuse call is refused, and what each mode launches (a refresh call
// launches what the plain forward does, a reuse call fewer, the deeper the cut the more), on three-level models at reduced widths
static void run_layer_cache(bool vsr) {
    lavie_unet_config cfg = base_config();
    cfg.num_levels = 3;
    cfg.block_out_channels[2] = 640; cfg.attn_levels[1] = 1; cfg.attn_levels[2] = 0;
    if (vsr) {
        cfg.in_channels = 8; cfg.block_out_channels[0] = 256; cfg.block_out_channels[1] = 512; cfg.block_out_channels[2] = 512;
        cfg.vsr_blocks = 1; cfg.only_cross_attention[0] = 1; cfg.vsr_temporal_modules = 1; cfg.num_class_embeds = 10;
    }
    auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
    {   // fewer than three levels: refused
        Model two(base_config());
        REQUIRE(refused(lavie_unet_set_layer_cache(two.h, 1), "levels"));
        REQUIRE(lavie_unet_set_layer_cache(two.h, 0) == 0 && lavie_unet_layer_cache_bytes(two.h) == 0);
    }
    Model m(cfg);
    const int B = 2, F = 4, H = 8, W = 8, L = 77;
    std::vector<unsigned short> x((size_t)B * cfg.in_channels * F * H * W), y((size_t)B * cfg.out_channels * F * H * W);
    std::vector<unsigned short> ctx((size_t)B * L * cfg.cross_attention_dim);
    std::vector<float> t(B, 500.f);
    std::vector<int> lab(B, 3);
    const int* labels = vsr ? lab.data() : nullptr;
    auto fwd = [&](int mode, int b = B) {
        return lavie_unet_forward_cached(m.h, x.data(), t.data(), ctx.data(), labels, y.data(), b, F, H, W, L, mode, nullptr);
    };
    auto launches = [&](int mode) {
        const long b = lavie_hostcheck_launches();
        REQUIRE(fwd(mode) == 0);
        return lavie_hostcheck_launches() - b;
    };
    REQUIRE(refused(lavie_unet_set_layer_cache(nullptr, 1), "null handle") && lavie_unet_layer_cache_bytes(nullptr) == -1);
    REQUIRE(refused(lavie_unet_set_layer_cache(m.h, -1), "depth=-1"));
    REQUIRE(refused(lavie_unet_set_layer_cache(m.h, cfg.layers_per_block + 1), "depth=3"));
    REQUIRE(lavie_unet_set_layer_cache(m.h, 1) == 0);
    REQUIRE(lavie_unet_layer_cache_bytes(m.h) == 0);                       // no shape yet: prepare() allocates
    REQUIRE(lavie_unet_prepare(m.h, B, F, H, W, L) == 0);
    const long long rows0 = (long long)B * F * H * W;
    REQUIRE(lavie_unet_layer_cache_bytes(m.h) >= rows0 * cfg.block_out_channels[0] * 2);
    REQUIRE(refused(lavie_unet_forward_cached(nullptr, x.data(), t.data(), ctx.data(), labels, y.data(), B, F, H, W, L, 0, nullptr), "null handle"));
    REQUIRE(refused(fwd(3), "mode=3") && refused(fwd(-1), "mode=-1"));
    REQUIRE(refused(fwd(LAVIE_LAYER_CACHE_REUSE), "refresh"));            // reuse before any refresh
    REQUIRE(fwd(LAVIE_LAYER_CACHE_OFF) == 0);                             // (the first forward builds the per-F tables)
    REQUIRE(refused(fwd(LAVIE_LAYER_CACHE_REUSE), "refresh"));            // a plain forward fills nothing
    const long plain = launches(LAVIE_LAYER_CACHE_OFF);
    REQUIRE(launches(LAVIE_LAYER_CACHE_REFRESH) == plain);                // the full walk, launch for launch
    const long shallow1 = launches(LAVIE_LAYER_CACHE_REUSE);
    REQUIRE(shallow1 > 0 && shallow1 < plain);
    REQUIRE(launches(LAVIE_LAYER_CACHE_OFF) == plain && launches(LAVIE_LAYER_CACHE_REUSE) == shallow1);      // a plain forward in between keeps it
    REQUIRE(refused(fwd(LAVIE_LAYER_CACHE_REUSE, 1), "B=1"));             // another batch than the recorded one
    REQUIRE(launches(LAVIE_LAYER_CACHE_REUSE) == shallow1);
    if (!vsr) {     // the shared CFG prefix lies in front of cut A: the same saving in a reuse call as in the plain forward
        REQUIRE(lavie_unet_cache_context(m.h, ctx.data(), B, L, nullptr) == 0);
        const long plain_c = launches(LAVIE_LAYER_CACHE_OFF);
        REQUIRE(lavie_unet_set_cfg_shared_input(m.h, 1) == 0);
        REQUIRE(launches(LAVIE_LAYER_CACHE_REFRESH) == launches(LAVIE_LAYER_CACHE_OFF));
        REQUIRE(launches(LAVIE_LAYER_CACHE_REUSE) < plain_c);
        REQUIRE(lavie_unet_set_cfg_shared_input(m.h, 0) == 0);
        REQUIRE(lavie_unet_cache_context(m.h, nullptr, 0, 0, nullptr) == 0);
    }
    REQUIRE(lavie_unet_set_layer_cache(m.h, 2) == 0);                      // another depth: the held cache is invalid
    REQUIRE(lavie_unet_layer_cache_bytes(m.h) >= rows0 * cfg.block_out_channels[1] * 2);      // B now lies behind the upsampler: level 1's width
    REQUIRE(refused(fwd(LAVIE_LAYER_CACHE_REUSE), "refresh"));
    REQUIRE(launches(LAVIE_LAYER_CACHE_REFRESH) == plain);
    const long shallow2 = launches(LAVIE_LAYER_CACHE_REUSE);
    REQUIRE(shallow2 > shallow1 && shallow2 < plain);
    REQUIRE(lavie_unet_prepare(m.h, B, F, H, W, L) == 0);                  // the same shape again: kept
    REQUIRE(launches(LAVIE_LAYER_CACHE_REUSE) == shallow2);
    REQUIRE(lavie_unet_prepare(m.h, B, F, 2 * H, W, L) == 0);              // another shape: invalid
    REQUIRE(refused(fwd(LAVIE_LAYER_CACHE_REUSE), "refresh"));
    REQUIRE(launches(LAVIE_LAYER_CACHE_REFRESH) == plain && launches(LAVIE_LAYER_CACHE_REUSE) == shallow2);
    REQUIRE(lavie_unet_set_layer_cache(m.h, 0) == 0 && lavie_unet_layer_cache_bytes(m.h) == 0);
    REQUIRE(refused(fwd(LAVIE_LAYER_CACHE_REUSE), "set_layer_cache") && refused(fwd(LAVIE_LAYER_CACHE_REFRESH), "set_layer_cache"));
    REQUIRE(launches(LAVIE_LAYER_CACHE_OFF) == plain);
}

static void run_traces(const char* path) {
    g_out = fopen(path, "w");
    REQUIRE(g_out != nullptr);
    lavie_hostcheck_trace_to(g_out);
    lavie_hostcheck_trace_copies(1);
    {   // base model at the production shape (cached context, shared prefix): every force_tile mode, forced split-K, fused mask 0x30
        const lavie_unet_config cfg = production_config();
        trace_case("base finalize");
        Model m(cfg);
        for (int mode = 0; mode <= 9; ++mode) {
            REQUIRE(lavie_debug_force_tile(mode) == 0);
            trace_case("base force_tile=%d", mode);
            trace_forward(cfg, m, 2, 16, 40, 64, true, true);
        }
        REQUIRE(lavie_debug_force_tile(0) == 0);
        for (int s = 2; s <= 3; ++s) {
            REQUIRE(lavie_debug_force_splits(s) == 0);
            trace_case("base force_splits=%d", s);
            trace_forward(cfg, m, 2, 16, 40, 64, true, true);
        }
        REQUIRE(lavie_debug_force_splits(0) == 0);
        REQUIRE(lavie_debug_fused_mask(0x30) == 0);
        trace_case("base fused_mask=0x30");
        trace_forward(cfg, m, 2, 16, 40, 64, true, true);
        REQUIRE(lavie_debug_fused_mask(0x137) == 0);
    }
    {   // the routes of a forward, on a fresh base model (its workspace has not grown under the forced modes above; its finalize is
        // the one traced above): 8 frames, where the fused temporal block does not apply; no fused kernel at all and the default mask
        // with each of bits 0, 1, 2, 4, 5, 8 off in turn, each with and without the context cache and the shared prefix; explicit
        // LayerNorms; the long fused text cross-attention
        const lavie_unet_config cfg = production_config();
        lavie_hostcheck_trace_to(nullptr);
        Model m(cfg);
        lavie_hostcheck_trace_to(g_out);
        trace_case("base F=8");
        trace_forward(cfg, m, 2, 8, 40, 64, true, true);
        const int masks[] = {0, 0x136, 0x135, 0x133, 0x127, 0x117, 0x037};
        for (int mask : masks) {
            REQUIRE(lavie_debug_fused_mask(mask) == 0);
            for (int v = 0; v < 4; ++v) {
                trace_case("base fused_mask=0x%03x cached=%d shared=%d", mask, v >> 1, v & 1);
                trace_forward(cfg, m, 2, 16, 40, 64, (v >> 1) != 0, (v & 1) != 0);
            }
        }
        REQUIRE(lavie_debug_fused_mask(0x137) == 0);
        REQUIRE(lavie_unet_set_ln_fold(m.h, 0) == 0);
        trace_case("base ln_fold=0");
        trace_forward(cfg, m, 2, 16, 40, 64, true, true);
        REQUIRE(lavie_unet_set_ln_fold(m.h, 1) == 0);
        trace_case("base 154-token context");
        trace_forward(cfg, m, 2, 16, 40, 64, true, true, 154);
    }
    {   // interpolation model (feed-forward before temporal): 61 frames, eight input channels; without the fused feed-forward, and
        // without the fused text cross-attention
        lavie_unet_config cfg = production_config();
        cfg.in_channels = 8; cfg.sparse_causal_attn1 = 1; cfg.temporal_plain = 1; cfg.ff_before_temporal = 1;
        trace_case("interpolation");
        Model m(cfg);
        trace_forward(cfg, m, 2, 61, 40, 64, true, false);
        for (int mask : {0x136, 0x133}) {
            REQUIRE(lavie_debug_fused_mask(mask) == 0);
            trace_case("interpolation fused_mask=0x%03x", mask);
            trace_forward(cfg, m, 2, 61, 40, 64, true, false);
        }
        REQUIRE(lavie_debug_fused_mask(0x137) == 0);
    }
    {   // VSR UNet: 256 / 512 / 512 / 1024, noise-level labels, 8 frames at 320 x 512
        lavie_unet_config cfg = production_config();
        const int w[4] = {256, 512, 512, 1024}, a[4] = {0, 1, 1, 1}, oc[4] = {1, 1, 1, 0};
        for (int i = 0; i < 4; ++i) { cfg.block_out_channels[i] = w[i]; cfg.attn_levels[i] = a[i]; cfg.only_cross_attention[i] = oc[i]; }
        cfg.in_channels = 8; cfg.cross_attention_dim = 1024; cfg.vsr_blocks = 1; cfg.vsr_temporal_modules = 1; cfg.num_class_embeds = 1000;
        trace_case("vsr 8 frames 320x512");
        Model m(cfg);
        trace_forward(cfg, m, 2, 8, 320, 512, false, false);
    }
    {   // the reduced variants of the sanitizer run
        lavie_unet_config interp = base_config();
        interp.in_channels = 8; interp.sparse_causal_attn1 = 1; interp.temporal_plain = 1; interp.ff_before_temporal = 1;
        lavie_unet_config vsr = base_config();
        vsr.in_channels = 8; vsr.block_out_channels[0] = 256; vsr.block_out_channels[1] = 512; vsr.attn_levels[1] = 1;
        vsr.vsr_blocks = 1; vsr.only_cross_attention[0] = 1; vsr.vsr_temporal_modules = 1; vsr.num_class_embeds = 10;
        struct { const char* name; lavie_unet_config cfg; int B, F, H, W; bool cached, shared; } cases[] = {
            {"reduced base", base_config(), 2, 16, 16, 16, true, true}, {"reduced base odd batch", base_config(), 1, 4, 8, 8, false, false},
            {"reduced interpolation", interp, 2, 7, 8, 8, true, false}, {"reduced vsr", vsr, 2, 4, 8, 8, false, false}};
        for (auto& c : cases) {
            trace_case("%s", c.name);
            Model m(c.cfg);
            trace_forward(c.cfg, m, c.B, c.F, c.H, c.W, c.cached, c.shared);
        }
    }
    {   // what else a forward decides, on the reduced base model: perturbed-attention guidance (three entries, the last one perturbed in
        // one level-0 and the mid-block transformer) and FreeU, each followed by the plain forward again; and the two block entry
        // points, which build their own per-call state and workspace: a resnet with two inputs and a shortcut, one transformer
        const lavie_unet_config cfg = base_config();
        Model m(cfg);
        const char* layers[2] = {"down_blocks.0.attentions.0", "mid_block"};
        REQUIRE(lavie_unet_set_pag(m.h, layers, 2, 1) == 0);
        trace_case("reduced base pag");
        trace_forward(cfg, m, 3, 16, 16, 16, true, false);
        REQUIRE(lavie_unet_set_pag(m.h, nullptr, 0, 0) == 0);
        trace_case("reduced base pag off");
        trace_forward(cfg, m, 3, 16, 16, 16, true, false);
        REQUIRE(lavie_unet_set_freeu(m.h, 0.9f, 0.2f, 1.5f, 1.6f) == 0);
        trace_case("reduced base freeu");
        trace_forward(cfg, m, 2, 16, 16, 16, true, true);
        REQUIRE(lavie_unet_set_freeu(m.h, 1.f, 1.f, 1.f, 1.f) == 0);
        trace_case("reduced base freeu off");
        trace_forward(cfg, m, 2, 16, 16, 16, true, true);
        const int B = 2, F = 16, H = 16, W = 16, C0 = cfg.block_out_channels[0], C1 = cfg.block_out_channels[1];
        std::vector<unsigned short> x((size_t)B * F * H * W * C0), ctx((size_t)B * 77 * cfg.cross_attention_dim);
        std::vector<float> temb((size_t)B * C0 * 4);
        trace_case("reduced base resnet_forward");       // up_blocks.0.resnets.0: 640 + 640 -> 640 channels at level 1; one video of two frames (its private workspace leaves 4 MiB for split-K slabs)
        REQUIRE(lavie_unet_resnet_forward(m.h, "up_blocks.0.resnets.0", x.data(), C1, x.data(), C1, temb.data(), x.data(), 1, 2, H / 2, W / 2,
                                          nullptr) == 0);
        trace_case("reduced base transformer_forward");
        REQUIRE(lavie_unet_transformer_forward(m.h, "down_blocks.0.attentions.0", x.data(), ctx.data(), B, F, H, W, 77, nullptr) == 0);
    }
    for (int mode = 0; mode <= 9; ++mode) {
        REQUIRE(lavie_debug_force_tile(mode) == 0);
        trace_case("operators force_tile=%d", mode);
        trace_operators();
    }
    REQUIRE(lavie_debug_force_tile(0) == 0);
    lavie_hostcheck_trace_to(nullptr);
    fclose(g_out);
    printf("hostcheck: trace written (%ld stubbed kernel launches)\n", lavie_hostcheck_launches());
}

// ---- operator launch trace: IN holds one operator call per line, "<entry> key=int ..." — the entry point without lavie_ / _f16,
// its integer arguments under the names of include/lavie_hip.h, 0 / 1 for each optional operand (bias, bias2, R, x2, sc1, sc2) and
// force_tile / force_splits (default 0); the end and glue kernels' entries (timestep_sinusoid ... f16_to_f32) and the pack / bind steps
// of the row-resident blocks (pack_geglu_mlp, bind_cross_block[_long]: pack + bind) likewise, and the blocks themselves (geglu_mlp, temporal_block,
// cross_block[_long], proj_qkv), temporal_attention, group_norm[_affine], conv_edge_in / conv_edge_out, attention, sparse_causal_attention and freeu (b_milli / s_milli: the factors in thousandths) on exactly sized buffers, under rowfuse_grid / temporal_budget (default 0).  Tensors are never read.  OUT: "== <line>", then the stub's launch lines of that call, or
// stats_cs=1 / stats_rs=1 on a GEMM-family line arm the statistics sink around the call (planned first, the sink sized exactly); behind the
// launch lines comes "## stats ..." with the plan (written or not, rows, span, sets, blocks, slots); group_norm_stats takes descriptors
// as cs1_C / cs1_rows / cs1_nsets / cs1_set_blocks / cs1_span (cs2_ likewise) and prints "## fold=<producer-count delta>"; rowstat_finalize.
// "!! refused" where the library returns an error (its message goes to stderr).  A line the driver cannot parse ends the run.
static int run_optrace(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "r");
    REQUIRE(in != nullptr);
    g_out = fopen(out_path, "w");
    REQUIRE(g_out != nullptr);
    lavie_hostcheck_trace_to(g_out);
    static std::vector<unsigned short> buf(64);
    void* d = buf.data();
    const float* fd = (const float*)buf.data();
    char line[1024];
    int calls = 0;
    while (fgets(line, sizeof(line), in)) {
        std::string s = line;
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ')) s.pop_back();
        if (s.empty() || s[0] == '#') continue;
        std::istringstream is(s);
        std::string entry, tok;
        is >> entry;
        std::map<std::string, long> a;
        while (is >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || eq == 0 || eq + 1 == tok.size()) { fprintf(stderr, "hostcheck optrace: bad token '%s' in '%s'\n", tok.c_str(), s.c_str()); return 2; }
            char* end = nullptr;
            a[tok.substr(0, eq)] = strtol(tok.c_str() + eq + 1, &end, 10);
            if (*end) { fprintf(stderr, "hostcheck optrace: bad value in '%s'\n", tok.c_str()); return 2; }
        }
        std::map<std::string, bool> used;
        bool missing = false;
        auto I = [&](const char* k) -> int {            // a required integer
            used[k] = true;
            auto it = a.find(k);
            if (it == a.end()) { fprintf(stderr, "hostcheck optrace: '%s' lacks %s\n", s.c_str(), k); missing = true; return 0; }
            return (int)it->second;
        };
        auto O = [&](const char* k) -> int {            // an optional one: 0 when absent
            used[k] = true;
            auto it = a.find(k);
            return it == a.end() ? 0 : (int)it->second;
        };
        auto P = [&](const char* k) -> void* { return O(k) ? d : nullptr; };
        auto F = [&](const char* k) -> const float* { return O(k) ? fd : nullptr; };
        const int tile = O("force_tile"), splits = O("force_splits"), grid_cap = O("rowfuse_grid"), budget = O("temporal_budget");
        const int stats_cs = O("stats_cs"), stats_rs = O("stats_rs");      // the statistics sink around a GEMM-family call
        std::function<int()> gemm;                                          // the GEMM-family call of this line, run below
        fprintf(g_out, "== %s\n", s.c_str());
        int rc = lavie_debug_force_tile(tile);
        lavie_debug_force_splits(splits);
        if (rc == 0) rc = lavie_debug_rowfuse_grid(grid_cap);
        lavie_debug_temporal_budget(budget);
        if (rc == 0) {
            if (entry == "linear") {
                const int lda = I("lda"), ldb2 = I("ldb2"), rpb = I("rows_per_batch"), ldr = I("ldr"), ldc = I("ldc"), M = I("M"), N = I("N"), K = I("K"), g = I("geglu");
                if (!missing) gemm = [=] { return lavie_linear_f16(d, lda, d, F("bias"), F("bias2"), ldb2, rpb, P("R"), ldr, d, ldc, M, N, K, g, nullptr); };
            } else if (entry == "linear_lnfold" || entry == "linear_lnfold_geglu") {
                const int M = I("M"), N = I("N"), K = I("K");
                if (!missing)
                    gemm = [=] { return entry == "linear_lnfold" ? lavie_linear_lnfold_f16(d, d, F("bias"), fd, fd, d, M, N, K, nullptr)
                                                                 : lavie_linear_lnfold_geglu_f16(d, d, F("bias"), fd, fd, d, M, N, K, nullptr); };
            } else if (entry == "conv3x3") {
                const int C1 = I("C1"), C2 = I("C2"), SC1 = I("SC1"), SC2 = I("SC2"), ldb2 = I("ldb2"), rpb = I("rows_per_batch"), NI = I("NI"), Hi = I("Hi"),
                          Wi = I("Wi"), Cout = I("Cout"), stride = I("stride"), ups = I("ups");
                if (!missing)
                    gemm = [=] { return lavie_conv3x3_f16(d, C1, P("x2"), C2, P("sc1"), SC1, P("sc2"), SC2, d, F("bias"), F("bias2"), ldb2, rpb, P("R"), d, NI, Hi, Wi,
                                                          Cout, stride, ups, d, nullptr); };
            } else if (entry == "conv3x3_down") {
                const int C = I("C"), NI = I("NI"), Hi = I("Hi"), Wi = I("Wi"), Cout = I("Cout"), stride = I("stride"), pad_lo = I("pad_lo");
                if (!missing) gemm = [=] { return lavie_conv3x3_down_f16(d, C, d, F("bias"), d, NI, Hi, Wi, Cout, stride, pad_lo, d, nullptr); };
            } else if (entry == "upsample_conv3x3") {
                const int NI = I("NI"), Hi = I("Hi"), Wi = I("Wi"), C = I("C");
                if (!missing) gemm = [=] { return lavie_upsample_conv3x3_f16(d, d, F("bias"), d, NI, Hi, Wi, C, d, nullptr); };
            } else if (entry == "temporal_conv") {
                const int C = I("C"), ldb2 = I("ldb2"), rpb = I("rows_per_batch"), B = I("B"), Fr = I("F"), D = I("D"), Cout = I("Cout"), taps = I("taps");
                if (!missing) gemm = [=] { return lavie_temporal_conv_f16(d, C, d, F("bias"), F("bias2"), ldb2, rpb, P("R"), d, B, Fr, D, Cout, taps, d, nullptr); };
            } else if (entry == "timestep_sinusoid") {
                const int B = I("B"), dim = I("dim");
                if (!missing) rc = lavie_timestep_sinusoid_f32(fd, (float*)d, B, dim, nullptr);
            } else if (entry == "gemv") {
                const int B = I("B"), N = I("N"), K = I("K"), ai = I("act_in"), ao = I("act_out");
                if (!missing) rc = lavie_gemv_f16(fd, d, F("bias"), (float*)d, B, N, K, ai, ao, nullptr);
            } else if (entry == "pack_conv_in" || entry == "pack_conv_out") {
                const int Cout = I("Cout"), Cin = I("Cin");
                if (!missing) rc = entry == "pack_conv_in" ? lavie_pack_conv_in_f16(d, d, Cout, Cin, nullptr) : lavie_pack_conv_out_f16(d, d, Cout, Cin, nullptr);
            } else if (entry == "conv_in" || entry == "conv_out") {
                const int B = I("B"), Cin = I("Cin"), Fr = I("F"), Hh = I("H"), Ww = I("W"), Cout = I("Cout");
                if (!missing)
                    rc = entry == "conv_in" ? lavie_conv_in_f16(d, d, fd, d, B, Cin, Fr, Hh, Ww, Cout, nullptr)
                                            : lavie_conv_out_f16(d, d, fd, d, B, Cin, Fr, Hh, Ww, Cout, nullptr);
            } else if (entry == "add_class_emb_silu") {
                const int B = I("B"), N = I("N"), nc = I("num_classes"), label = O("label");
                int labels[16];
                for (int& v : labels) v = label;
                if (!missing) rc = lavie_add_class_emb_silu_f32((float*)d, d, labels, B, N, nc, nullptr);
            } else if (entry == "fill_relpos_bias") {
                const int heads = I("heads"), Fr = I("F"), nb = I("num_buckets");
                if (!missing) rc = lavie_fill_relpos_bias_f32(d, (const int*)d, (float*)d, heads, Fr, nb, nullptr);
            } else if (entry == "ln_fold") {
                const int N = I("N"), K = I("K");
                if (!missing) rc = lavie_ln_fold_f16(d, fd, fd, P("bias_f16"), d, (float*)d, (float*)d, N, K, nullptr);
            } else if (entry == "pack_geglu_vec") {
                const int N = I("N");
                if (!missing) rc = lavie_pack_geglu_vec_f32(fd, (float*)d, N, nullptr);
            } else if (entry == "copy_rows") {
                const int ls = I("ld_src"), ld = I("ld_dst"), rows = I("rows"), cols = I("cols"), col0 = I("col0");
                if (!missing) rc = lavie_copy_rows_f16(d, ls, d, ld, rows, cols, col0, nullptr);
            } else if (entry == "f16_to_f32") {
                const int n = I("n");
                if (!missing) rc = lavie_f16_to_f32(d, P("b"), (float*)d, n, nullptr);
            } else if (entry == "pack_geglu_mlp") {         // the pack_* / bind_* steps of the row-resident blocks copy index lists: exactly sized buffers
                const int C = I("C");
                const long long ib = lavie_geglu_mlp_image_bytes(C), bf = lavie_geglu_mlp_bias_floats(C);
                if (!missing) {
                    std::vector<unsigned short> w1((size_t)8 * C * C), b1((size_t)8 * C), w2((size_t)4 * C * C), img((size_t)(ib > 0 ? ib / 2 : 1));
                    std::vector<float> b1img((size_t)(bf > 0 ? bf : 1));
                    rc = ib > 0 ? lavie_pack_geglu_mlp_f16(w1.data(), b1.data(), w2.data(), C, img.data(), b1img.data(), nullptr) : -1;
                }
            } else if (entry == "bind_cross_block" || entry == "bind_cross_block_long") {
                const int B = I("B"), L = I("ctx_len"), C = I("C");
                const bool lng = entry == "bind_cross_block_long";
                const long long ib = lng ? lavie_cross_block_long_image_bytes(C, 8) : lavie_cross_block_image_bytes(C, 8);
                if (!missing) {
                    std::vector<unsigned short> w((size_t)C * C), tmpl((size_t)(ib > 0 ? ib / 2 : 1)), kv((size_t)B * L * 2 * C), img((size_t)B * (ib > 0 ? ib / 2 : 1));
                    rc = ib > 0 ? (lng ? lavie_pack_cross_block_long_f16(w.data(), w.data(), w.data(), C, tmpl.data(), nullptr)
                                       : lavie_pack_cross_block_f16(w.data(), w.data(), w.data(), C, tmpl.data(), nullptr)) : -1;
                    if (rc == 0)
                        rc = lng ? lavie_bind_cross_block_long_f16(tmpl.data(), kv.data(), B, L, C, img.data(), nullptr)
                                 : lavie_bind_cross_block_f16(tmpl.data(), kv.data(), B, L, C, img.data(), nullptr);
                }
            } else if (entry == "geglu_mlp") {              // the row-resident blocks, temporal attention and GroupNorm: exactly sized buffers too
                const int M = I("M"), C = I("C");
                const long long ib = lavie_geglu_mlp_image_bytes(C), bf = lavie_geglu_mlp_bias_floats(C);
                if (!missing) {
                    std::vector<unsigned short> x((size_t)M * C), y((size_t)M * C), img((size_t)(ib > 0 ? ib / 2 : 1));
                    std::vector<float> b1img((size_t)(bf > 0 ? bf : 1)), v((size_t)C);
                    rc = lavie_geglu_mlp_f16(x.data(), y.data(), M, C, img.data(), b1img.data(), v.data(), v.data(), v.data(), 1e-5f, nullptr);
                }
            } else if (entry == "temporal_block") {
                const int B = I("B"), Fr = I("F"), D = I("D"), C = I("C"), heads = I("heads"), rot = I("rot_dim");
                const long long ib = lavie_temporal_block_image_bytes(C, heads, Fr, rot);
                if (!missing) {
                    std::vector<unsigned short> x((size_t)B * Fr * D * C), y(x.size()), img((size_t)(ib > 0 ? ib / 2 : 1));
                    std::vector<float> v((size_t)C), rb((size_t)heads * Fr * Fr), tab((size_t)Fr * (rot / 2) + 1);
                    rc = lavie_temporal_block_f16(x.data(), y.data(), B, Fr, D, C, heads, img.data(), v.data(), v.data(), v.data(), rb.data(), tab.data(),
                                                  tab.data(), rot, 0.1f, 1e-5f, nullptr);
                }
            } else if (entry == "cross_block" || entry == "cross_block_long") {
                const int M = I("M"), rpb = I("rows_per_batch"), C = I("C"), heads = I("heads"), L = I("ctx_len");
                const bool lng = entry == "cross_block_long";
                const long long ib = lng ? lavie_cross_block_long_image_bytes(C, heads) : lavie_cross_block_image_bytes(C, heads);
                if (!missing) {
                    const size_t nb = rpb > 0 ? (size_t)(M / rpb) : 1;
                    std::vector<unsigned short> att((size_t)M * C), x(att.size()), y(att.size()), img((nb ? nb : 1) * (size_t)(ib > 0 ? ib / 2 : 1));
                    std::vector<float> v((size_t)C);
                    rc = lng ? lavie_cross_block_long_f16(att.data(), x.data(), y.data(), M, rpb, C, heads, img.data(), v.data(), v.data(), v.data(), v.data(), L, 0.1f, 1e-5f, nullptr)
                             : lavie_cross_block_f16(att.data(), x.data(), y.data(), M, rpb, C, heads, img.data(), v.data(), v.data(), v.data(), v.data(), L, 0.1f, 1e-5f, nullptr);
                }
            } else if (entry == "proj_qkv") {
                const int rpd = I("rows_per_domain"), M = I("M"), C = I("C");
                const long long ib = lavie_proj_qkv_image_bytes(C);
                if (!missing) {
                    const size_t doms = rpd > 0 ? (size_t)((M + rpd - 1) / rpd) : 1;
                    std::vector<unsigned short> x((size_t)M * C), tx(x.size()), qkv((size_t)M * 3 * C), img((size_t)(ib > 0 ? ib / 2 : 1));
                    std::vector<float> ab(doms * C * 2), v((size_t)C);
                    rc = lavie_proj_qkv_f16(x.data(), ab.data(), rpd, img.data(), v.data(), v.data(), v.data(), 1e-5f, tx.data(), qkv.data(), M, C, nullptr);
                }
            } else if (entry == "temporal_attention") {
                const int ld = I("ld"), ldo = I("ldo"), B = I("B"), Fr = I("F"), D = I("D"), heads = I("heads"), dh = I("dh"), rot = I("rot_dim");
                if (!missing) {
                    const size_t rows = (size_t)B * Fr * D;
                    std::vector<unsigned short> qkv(rows * ld), o(rows * ldo);
                    std::vector<float> bias((size_t)heads * Fr * Fr), tab((size_t)Fr * (rot / 2) + 1);
                    rc = lavie_temporal_attention_f16(qkv.data(), ld, o.data(), ldo, B, Fr, D, heads, dh, bias.data(), rot ? tab.data() : nullptr,
                                                      rot ? tab.data() : nullptr, rot, 0.1f, nullptr);
                }
            } else if (entry == "group_norm" || entry == "group_norm_affine") {
                const bool aff = entry == "group_norm_affine";
                const int C1 = aff ? I("C") : I("C1"), C2 = aff ? 0 : I("C2"), NB = I("NB"), Pr = I("P"), groups = I("groups"), silu = aff ? 0 : I("silu");
                if (!missing) {
                    const size_t rows = (size_t)NB * Pr;
                    std::vector<unsigned short> x1(rows * C1), x2(rows * C2 + 1), y(rows * (C1 + C2));
                    std::vector<float> v((size_t)C1 + C2), ws((size_t)lavie_group_norm_ws_floats(NB, groups)), ab((size_t)NB * (C1 + C2) * 2);
                    rc = aff ? lavie_group_norm_affine_f16(x1.data(), C1, NB, Pr, groups, v.data(), v.data(), 1e-5f, ws.data(), ab.data(), nullptr)
                             : lavie_group_norm_f16(x1.data(), C1, O("x2") ? x2.data() : nullptr, C2, NB, Pr, groups, v.data(), v.data(), 1e-5f, silu, ws.data(),
                                                    y.data(), nullptr);
                }
            } else if (entry == "group_norm_stats") {       // producer-statistics descriptors cs1_* / cs2_* (absent: none) over exactly sized partials
                const int C1 = I("C1"), C2 = I("C2"), NB = I("NB"), Pr = I("P"), groups = I("groups"), silu = I("silu");
                lavie_gn_producer_stats ds[2];
                std::vector<float> parts[2];
                bool have[2] = {false, false};
                for (int t = 0; t < 2; ++t) {
                    const std::string pre = t ? "cs2_" : "cs1_";
                    if (!a.count(pre + "rows")) continue;
                    have[t] = true;
                    memset(&ds[t], 0, sizeof(ds[t]));
                    ds[t].struct_size = (int)sizeof(ds[t]);
                    ds[t].C = I((pre + "C").c_str()); ds[t].rows = I((pre + "rows").c_str()); ds[t].nsets = I((pre + "nsets").c_str());
                    ds[t].set_blocks = I((pre + "set_blocks").c_str()); ds[t].span = I((pre + "span").c_str());
                    const long long n = (long long)ds[t].nsets * ds[t].set_blocks * 2 * ds[t].C;
                    parts[t].resize((size_t)(n > 0 ? n : 1));
                    ds[t].partials = parts[t].data(); ds[t].partials_floats = n;
                }
                if (!missing) {
                    const size_t rows = (size_t)NB * Pr;
                    std::vector<unsigned short> x1(rows * C1), x2(rows * C2 + 1), y(rows * (C1 + C2));
                    std::vector<float> v((size_t)C1 + C2), ws((size_t)lavie_group_norm_ws_floats(NB, groups));
                    const long long before = lavie_debug_gn_producer_count();
                    rc = lavie_group_norm_stats_f16(x1.data(), C1, O("x2") ? x2.data() : nullptr, C2, NB, Pr, groups, v.data(), v.data(), 1e-5f, silu, ws.data(),
                                                    y.data(), have[0] ? &ds[0] : nullptr, have[1] ? &ds[1] : nullptr, nullptr);
                    if (rc == 0) fprintf(g_out, "## fold=%lld\n", lavie_debug_gn_producer_count() - before);
                }
            } else if (entry == "rowstat_finalize") {
                const int slots = I("slots"), M = I("M"), row_len = I("row_len");
                if (!missing) {
                    std::vector<float> part((size_t)(M > 0 && slots > 0 ? (size_t)M * slots * 2 : 1)), out((size_t)(M > 0 ? M * 2 : 1));
                    rc = lavie_rowstat_finalize_f32(part.data(), slots, M, row_len, 1e-5f, out.data(), nullptr);
                }
            } else if (entry == "conv_edge_in" || entry == "conv_edge_out") {     // the autoencoder's kernels: exactly sized buffers as well
                const bool in = entry == "conv_edge_in";
                const int dt = I(in ? "x_dtype" : "y_dtype"), N = I("N"), Cin = I("Cin"), Hh = I("H"), Ww = I("W"), Cout = I("Cout");
                if (!missing) {
                    const size_t px = (size_t)N * Hh * Ww, cmax = (size_t)(Cin > Cout ? Cin : Cout), cmin = (size_t)(Cin < Cout ? Cin : Cout);
                    const long long oh = in ? 0 : lavie_conv_edge_out_image_halfs(Cin);
                    std::vector<unsigned short> rows(px * cmax), wp(in ? (size_t)9 * ((Cin + 1) & ~1) * Cout : (size_t)(oh > 0 ? oh : 1));
                    std::vector<float> img(px * cmin), b((size_t)Cout), tb((size_t)9 * Cout);      // the NCHW side, large enough in either dtype
                    rc = in ? lavie_conv_edge_in_f16(img.data(), dt, wp.data(), O("bias") ? b.data() : nullptr, O("tap_bias") ? tb.data() : nullptr,
                                                     rows.data(), N, Cin, Hh, Ww, Cout, nullptr)
                            : lavie_conv_edge_out_f16(rows.data(), wp.data(), O("bias") ? b.data() : nullptr, img.data(), dt, N, Cin, Hh, Ww, Cout, nullptr);
                }
            } else if (entry == "freeu") {                  // b / s in thousandths (the replay takes integers); in_place: h_out = h, skip_out = skip
                const int Ch = I("C_h"), C2 = I("C2"), NI = I("NI"), Hh = I("H"), Ww = I("W"), bm = I("b_milli"), sm = I("s_milli"), inpl = O("in_place");
                if (!missing) {
                    const size_t px = (size_t)(NI > 0 ? NI : 0) * (Hh > 0 ? Hh : 0) * (Ww > 0 ? Ww : 0);
                    const long long wb = lavie_freeu_workspace_bytes(C2, NI, Hh, Ww);
                    std::vector<unsigned short> h(px * (Ch > 0 ? Ch : 0) + 8), sk(px * (C2 > 0 ? C2 : 0) + 8), ho(h.size()), so(sk.size());
                    std::vector<float> ws((size_t)(wb > 0 ? wb / 4 : 1) + 4);
                    rc = lavie_freeu_f16(h.data(), Ch, sk.data(), C2, NI, Hh, Ww, bm / 1000.f, sm / 1000.f, inpl ? h.data() : ho.data(),
                                         inpl ? sk.data() : so.data(), ws.data(), nullptr);
                }
            } else if (entry == "attention") {
                const int ldq = I("ldq"), ldk = I("ldk"), ldv = I("ldv"), ldo = I("ldo"), NB = I("NB"), Lq = I("Lq"), Lk = I("Lk"), heads = I("heads"),
                          dh = I("dh"), div = I("kv_batch_div");
                if (!missing) {
                    const size_t rq = (size_t)NB * Lq, rk = (size_t)(div > 0 ? NB / div : NB) * Lk;
                    std::vector<unsigned short> q(rq * ldq), k(rk * ldk), v(rk * ldv), o(rq * ldo);
                    rc = lavie_attention_f16(q.data(), ldq, k.data(), ldk, v.data(), ldv, o.data(), ldo, NB, Lq, Lk, heads, dh, div, 0.05f, nullptr);
                }
            } else if (entry == "sparse_causal_attention") {
                const int ldq = I("ldq"), ldk = I("ldk"), ldv = I("ldv"), ldo = I("ldo"), NB = I("NB"), frames = I("frames"), D = I("D"), heads = I("heads"), dh = I("dh");
                if (!missing) {
                    const size_t rows = (size_t)NB * D;
                    std::vector<unsigned short> q(rows * ldq), k(rows * ldk), v(rows * ldv), o(rows * ldo);
                    rc = lavie_sparse_causal_attention_f16(q.data(), ldq, k.data(), ldk, v.data(), ldv, o.data(), ldo, NB, frames, D, heads, dh, 0.05f, nullptr);
                }
            } else {
                fprintf(stderr, "hostcheck optrace: unknown entry point '%s'\n", entry.c_str());
                return 2;
            }
        }
        if (missing) return 2;
        if (gemm && rc == 0) {
            if (stats_cs || stats_rs) {      // plan as if armed (nothing is launched), size the sink exactly, arm it, launch, report the plan
                lavie_op_statistics_info info;
                memset(&info, 0, sizeof(info));
                info.struct_size = (int)sizeof(info);
                REQUIRE(lavie_debug_op_statistics_plan(stats_cs, stats_rs) == 0);
                const long before = lavie_hostcheck_launches();
                rc = gemm();
                REQUIRE(lavie_debug_op_statistics_plan(0, 0) == 0);
                REQUIRE(lavie_hostcheck_launches() == before);
                if (rc == 0) {
                    REQUIRE(lavie_debug_op_statistics_last(&info) == 0);
                    std::vector<float> cs((size_t)(info.colstat_floats > 0 ? info.colstat_floats : 1)), rs((size_t)(info.rowstat_floats > 0 ? info.rowstat_floats : 1));
                    REQUIRE(lavie_debug_op_statistics(stats_cs ? cs.data() : nullptr, info.colstat_floats, stats_rs ? rs.data() : nullptr, info.rowstat_floats) == 0);
                    rc = gemm();
                    REQUIRE(lavie_debug_op_statistics(nullptr, 0, nullptr, 0) == 0);
                    if (rc == 0)
                        fprintf(g_out, "## stats colstat=%d rows=%d span=%d sets=%d set_blocks=%d contiguous=%d blocks_stored=%lld cs_floats=%lld rowstat=%d cols=%d slots=%d "
                                "rs_floats=%lld M=%d N=%d splits=%d\n", info.colstat_written, info.colstat_rows, info.colstat_span, info.nsets, info.set_blocks,
                                info.colstat_contiguous, info.colstat_blocks_stored, info.colstat_floats, info.rowstat_written, info.rowstat_cols, info.rowstat_slots,
                                info.rowstat_floats, info.M, info.N, info.splits);
                }
            } else {
                rc = gemm();
            }
        }
        for (const auto& kv : a)
            if (!used.count(kv.first)) { fprintf(stderr, "hostcheck optrace: '%s' does not take %s\n", entry.c_str(), kv.first.c_str()); return 2; }
        if (rc != 0) {
            fprintf(g_out, "!! refused\n");
            fprintf(stderr, "hostcheck optrace: '%s' refused: %s\n", s.c_str(), lavie_last_error());
        }
        ++calls;
    }
    REQUIRE(lavie_debug_force_tile(0) == 0);
    lavie_debug_force_splits(0);
    REQUIRE(lavie_debug_rowfuse_grid(0) == 0);
    lavie_debug_temporal_budget(0);
    lavie_hostcheck_trace_to(nullptr);
    fclose(g_out);
    fclose(in);
    printf("hostcheck: optrace written (%d calls, %ld stubbed kernel launches)\n", calls, lavie_hostcheck_launches());
    return 0;
}

static int run_optrace(const char* in_path, const char* out_path);

// The autoencoder's kernels past one workgroup, through the optrace entries themselves (tests/opcases.py vae_cases(): the integers of
// the largest case of each kernel): exactly sized buffers under the sanitizers, and the launches the walk mirrors of opcases.py state.
static void run_vae_optrace() {
    char in_path[] = "/tmp/hostcheck_in_XXXXXX", out_path[] = "/tmp/hostcheck_out_XXXXXX";
    const int fi = mkstemp(in_path), fo = mkstemp(out_path);
    REQUIRE(fi >= 0 && fo >= 0);
    close(fo);
    FILE* in = fdopen(fi, "w");
    REQUIRE(in != nullptr);
    fputs("conv_edge_out y_dtype=1 N=1 Cin=128 H=257 W=513 Cout=3 bias=1\n"
          "conv_edge_out y_dtype=0 N=1 Cin=8 H=257 W=513 Cout=8 bias=1\n"
          "conv_edge_out y_dtype=0 N=2 Cin=40 H=7 W=9 Cout=3 bias=1\n"
          "conv_edge_in x_dtype=0 N=1 Cin=4 H=129 W=128 Cout=512 bias=1 tap_bias=1\n"
          "conv_edge_in x_dtype=1 N=1 Cin=3 H=129 W=128 Cout=512 bias=1 tap_bias=0\n"
          "attention ldq=3088 ldk=3088 ldv=3088 ldo=1024 NB=3 Lq=129 Lk=129 heads=2 dh=512 kv_batch_div=1\n"
          "attention ldq=528 ldk=1040 ldv=1040 ldo=512 NB=4 Lq=40 Lk=97 heads=1 dh=512 kv_batch_div=2\n"
          "attention ldq=784 ldk=784 ldv=784 ldo=256 NB=1 Lq=161 Lk=161 heads=1 dh=256 kv_batch_div=1\n"
          "conv_edge_out y_dtype=0 N=1 Cin=12 H=2 W=2 Cout=3 bias=1\n", in);
    fclose(in);
    REQUIRE(run_optrace(in_path, out_path) == 0);
    FILE* out = fopen(out_path, "r");
    REQUIRE(out != nullptr);
    std::string got;
    char line[1024];
    while (fgets(line, sizeof(line), out)) got += line;
    fclose(out);
    unlink(in_path);
    unlink(out_path);
    for (const char* want : {"conv_edge_out_kernel<4, float> 1031,1,1 256,1,1", "conv_edge_out_kernel<0, half> 1031,1,1 256,1,1", "conv_edge_out_kernel<0, half> 2,1,1",
                             "conv_edge_in_kernel<half> 4096,1,1 256,1,1", "conv_edge_in_kernel<float> 4096,1,1 256,1,1", "attention_wide_kernel<512> 12,1,1 256,1,1",
                             "attention_wide_kernel<512> 4,1,1", "attention_wide_kernel<256> 2,1,1", "Cout=3 bias=1\n!! refused"})
        if (got.find(want) == std::string::npos) {
            fprintf(stderr, "hostcheck: the optrace of the autoencoder's kernels lacks '%s':\n%s", want, got.c_str());
            exit(2);
        }
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "trace") == 0) {
        run_traces(argv[2]);
        return 0;
    }
    if (argc == 4 && strcmp(argv[1], "optrace") == 0) return run_optrace(argv[2], argv[3]);
    if (argc == 3 && strcmp(argv[1], "kernels") == 0) {
        FILE* f = fopen(argv[2], "w");
        REQUIRE(f != nullptr);
        lavie_hostcheck_kernel_names_to(f);
        fclose(f);
        printf("hostcheck: kernel names written\n");
        return 0;
    }
    REQUIRE(lavie_abi_version() == LAVIE_ABI_VERSION);
    {   // argument checks of create
        lavie_unet_config c = base_config();
        lavie_unet_t h = nullptr;
        REQUIRE(lavie_unet_create(nullptr, &h) != 0);
        c.struct_size -= 4;
        REQUIRE(lavie_unet_create(&c, &h) != 0);
        c = base_config();
        c.num_levels = 9;
        REQUIRE(lavie_unet_create(&c, &h) != 0);
        c = base_config();
        c.block_out_channels[0] = 100;
        REQUIRE(lavie_unet_create(&c, &h) != 0);
    }
    run_model(base_config(), 2, 16, 16, 16, false, true);            // base block order, fused level-0 kernels in reach (C = 320, F = 16)
    run_model(base_config(), 1, 4, 8, 8, false);                     // odd batch, ragged tiles
    {
        lavie_unet_config c = base_config();                         // interpolation variant
        c.in_channels = 8; c.sparse_causal_attn1 = 1; c.temporal_plain = 1; c.ff_before_temporal = 1;
        run_model(c, 2, 7, 8, 8, false);
    }
    {
        lavie_unet_config c = base_config();                         // VSR variant
        c.in_channels = 8; c.block_out_channels[0] = 256; c.block_out_channels[1] = 512; c.attn_levels[1] = 1;
        c.vsr_blocks = 1; c.only_cross_attention[0] = 1; c.vsr_temporal_modules = 1; c.num_class_embeds = 10;
        run_model(c, 2, 4, 8, 8, true);
        run_withheld_tensor(c, "class_embedding.weight");           // listed under a condition, packed late
    }
    run_withheld_tensor(base_config(), "mid_block.attentions.0.transformer_blocks.0.attn_temp.to_out.0.bias");
    run_layer_cache(false);
    run_layer_cache(true);
    // operator-level argument checks
    REQUIRE(lavie_linear_f16(nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, 0, 16, 64, 63, 0, nullptr) != 0);
    REQUIRE(lavie_geglu_mlp_image_bytes(123) == 0);
    {   // lavie_debug_rowfuse_grid: 0 = min(tiles, 256), 1..256 = the cap; any other value is refused and leaves the setting as it was;
        // it reaches the four row-resident launchers and nothing else
        const int M = 4160, C = 320;                                 // 260 tiles of 16 rows, one video of 260 tiles, 13 frames of 20
        std::vector<unsigned short> x((size_t)M * C), y(x.size()), qkv((size_t)M * 3 * C), img((size_t)lavie_geglu_mlp_image_bytes(C) / 2),
            ximg((size_t)lavie_cross_block_image_bytes(C, 8) / 2), limg((size_t)lavie_cross_block_long_image_bytes(C, 8) / 2),
            timg((size_t)lavie_temporal_block_image_bytes(C, 8, 16, 32) / 2), pimg((size_t)lavie_proj_qkv_image_bytes(C) / 2);
        std::vector<float> b1img((size_t)lavie_geglu_mlp_bias_floats(C)), v((size_t)C), rb(8 * 16 * 16), tab(16 * 16), ab((size_t)13 * C * 2),
            ws((size_t)lavie_group_norm_ws_floats(1, 32));
        auto grids = [&](long* g) {
            REQUIRE(lavie_geglu_mlp_f16(x.data(), y.data(), M, C, img.data(), b1img.data(), v.data(), v.data(), v.data(), 1e-5f, nullptr) == 0);
            g[0] = lavie_hostcheck_last_grid_x();
            REQUIRE(lavie_temporal_block_f16(x.data(), y.data(), 1, 16, 260, C, 8, timg.data(), v.data(), v.data(), v.data(), rb.data(), tab.data(), tab.data(), 32,
                                             0.1f, 1e-5f, nullptr) == 0);
            g[1] = lavie_hostcheck_last_grid_x();
            REQUIRE(lavie_cross_block_f16(x.data(), x.data(), y.data(), M, M, C, 8, ximg.data(), v.data(), v.data(), v.data(), v.data(), 77, 0.1f, 1e-5f, nullptr) == 0);
            g[2] = lavie_hostcheck_last_grid_x();
            REQUIRE(lavie_cross_block_long_f16(x.data(), x.data(), y.data(), M, M, C, 8, limg.data(), v.data(), v.data(), v.data(), v.data(), 154, 0.1f, 1e-5f, nullptr) == 0);
            g[3] = lavie_hostcheck_last_grid_x();
            REQUIRE(lavie_proj_qkv_f16(x.data(), ab.data(), 320, pimg.data(), v.data(), v.data(), v.data(), 1e-5f, y.data(), qkv.data(), M, C, nullptr) == 0);
            g[4] = lavie_hostcheck_last_grid_x();
        };
        long g[5];
        grids(g);
        for (long v_ : g) REQUIRE(v_ == 256);
        REQUIRE(lavie_debug_rowfuse_grid(3) == 0);
        grids(g);
        for (long v_ : g) REQUIRE(v_ == 3);
        REQUIRE(lavie_debug_rowfuse_grid(257) != 0 && lavie_debug_rowfuse_grid(-1) != 0);
        REQUIRE(strstr(lavie_last_error(), "rowfuse_grid") != nullptr);
        grids(g);
        for (long v_ : g) REQUIRE(v_ == 3);                             // the refused values changed nothing
        REQUIRE(lavie_debug_rowfuse_grid(256) == 0 && lavie_debug_rowfuse_grid(1) == 0);
        grids(g);
        for (long v_ : g) REQUIRE(v_ == 1);
        REQUIRE(lavie_debug_rowfuse_grid(256) == 0);
        REQUIRE(lavie_geglu_mlp_f16(x.data(), y.data(), 48, C, img.data(), b1img.data(), v.data(), v.data(), v.data(), 1e-5f, nullptr) == 0);
        REQUIRE(lavie_hostcheck_last_grid_x() == 3);                      // never more workgroups than tiles
        REQUIRE(lavie_debug_rowfuse_grid(2) == 0);
        REQUIRE(lavie_group_norm_f16(x.data(), C, nullptr, 0, 1, M, 32, v.data(), v.data(), 1e-5f, 1, ws.data(), y.data(), nullptr) == 0);
        REQUIRE(lavie_hostcheck_last_grid_x() > 2);                       // another family's launch is not capped
        REQUIRE(lavie_debug_rowfuse_grid(0) == 0);
        grids(g);
        for (long v_ : g) REQUIRE(v_ == 256);
    }
    {   // the long fused text cross-attention (81..160 keys): sizes, and lengths / widths refused before any HIP call
        REQUIRE(lavie_cross_block_long_image_bytes(320, 8) == 840 * 1024 && lavie_cross_block_long_image_bytes(256, 8) == 0);
        std::vector<unsigned short> w(320 * 320), tmpl(840 * 512), kv(161 * 640), img(840 * 512), x(128 * 320);
        std::vector<float> v(320, 1.f);
        REQUIRE(lavie_pack_cross_block_long_f16(w.data(), w.data(), w.data(), 256, tmpl.data(), nullptr) != 0);
        REQUIRE(lavie_pack_cross_block_long_f16(w.data(), w.data(), w.data(), 320, tmpl.data(), nullptr) == 0);
        REQUIRE(lavie_bind_cross_block_long_f16(tmpl.data(), kv.data(), 1, 161, 320, img.data(), nullptr) != 0);
        REQUIRE(lavie_bind_cross_block_long_f16(tmpl.data(), kv.data(), 1, 80, 320, img.data(), nullptr) != 0);
        REQUIRE(lavie_bind_cross_block_long_f16(tmpl.data(), nullptr, 1, 154, 320, img.data(), nullptr) != 0);
        REQUIRE(lavie_bind_cross_block_long_f16(tmpl.data(), kv.data(), 1, 154, 320, img.data(), nullptr) == 0);
        REQUIRE(lavie_cross_block_long_f16(x.data(), x.data(), x.data(), 128, 128, 320, 8, img.data(), v.data(), v.data(), v.data(), v.data(),
                                           161, 0.1f, 1e-5f, nullptr) != 0);
        REQUIRE(lavie_cross_block_long_f16(x.data(), x.data(), x.data(), 128, 128, 320, 8, img.data(), v.data(), v.data(), v.data(), v.data(),
                                           154, 0.1f, 1e-5f, nullptr) == 0);
        REQUIRE(lavie_bind_cross_block_f16(tmpl.data(), kv.data(), 1, 81, 320, img.data(), nullptr) != 0);     // the short kernel: <= 80
    }
    {   // attention head dims: multiples of 8 up to 160, and the wide kernel's 256 / 512; the others are refused before any HIP call
        std::vector<unsigned short> qkv(64 * 3 * 520), o(64 * 520);
        const long before = lavie_hostcheck_launches();
        for (int dh : {40, 160, 256, 512})
            REQUIRE(lavie_attention_f16(qkv.data(), 3 * dh, qkv.data() + dh, 3 * dh, qkv.data() + 2 * dh, 3 * dh, o.data(), dh, 2, 32, 32, 1,
                                        dh, 1, 0.05f, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 4);
        for (int dh : {168, 384, 520}) {
            REQUIRE(lavie_attention_f16(qkv.data(), 3 * dh, qkv.data() + dh, 3 * dh, qkv.data() + 2 * dh, 3 * dh, o.data(), dh, 2, 32, 32, 1,
                                        dh, 1, 0.05f, nullptr) != 0);
            REQUIRE(strstr(lavie_last_error(), "512") != nullptr);
        }
        REQUIRE(lavie_sparse_causal_attention_f16(qkv.data(), 1536, qkv.data() + 512, 1536, qkv.data() + 1024, 1536, o.data(), 512, 2, 2, 16,
                                                  1, 512, 0.05f, nullptr) != 0);
        REQUIRE(lavie_hostcheck_launches() == before + 4);
    }
    {   // the text encoder: every refusal of its three operators and of lavie_text_* names the argument and launches
        // nothing; an accepted encode walks 2 + 8 layers launches inside the handle's own allocation (exactly sized: the sanitizers' to judge)
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const int C = 128, I = 256, V = 50, P = 77, Lyr = 2, heads = 4;
        std::vector<unsigned short> qkv(2 * 128 * 3 * C + 8), o(2 * 128 * C + 8), big(64 * 1024);
        std::vector<int> ids(16 * P, 3);
        const long before = lavie_hostcheck_launches();
        auto att = [&](void* q, int ld, void* out, int ldo, int NB, int L, int h, int dh, float sc) {
            return lavie_causal_attention_f16(q, ld, out, ldo, NB, L, h, dh, sc, nullptr);
        };
        REQUIRE(refused(att(qkv.data(), 3 * C, o.data(), C, 1, 129, heads, 32, 0.1f), "L=129"));
        REQUIRE(refused(att(qkv.data(), 3 * C, o.data(), C, 1, 0, heads, 32, 0.1f), "L=0"));
        REQUIRE(refused(att(qkv.data(), 3 * C, o.data(), C, 1, 77, heads, 40, 0.1f), "dh=40"));
        REQUIRE(refused(att(qkv.data(), 3 * C, o.data(), C, 0, 77, heads, 32, 0.1f), "NB=0"));
        REQUIRE(refused(att(qkv.data(), 3 * C - 8, o.data(), C, 1, 77, heads, 32, 0.1f), "ld=376"));
        REQUIRE(refused(att(qkv.data(), 3 * C + 4, o.data(), C, 1, 77, heads, 32, 0.1f), "ld=388"));
        REQUIRE(refused(att(qkv.data(), 3 * C, o.data(), C - 8, 1, 77, heads, 32, 0.1f), "ldo=120"));
        REQUIRE(refused(att(nullptr, 3 * C, o.data(), C, 1, 77, heads, 32, 0.1f), "null"));
        REQUIRE(refused(att(qkv.data() + 1, 3 * C, o.data(), C, 1, 77, heads, 32, 0.1f), "aligned"));
        REQUIRE(refused(att(qkv.data(), 3 * C, o.data(), C, 1, 77, heads, 32, INFINITY), "scale"));
        REQUIRE(refused(lavie_token_embed_f16(ids.data(), big.data(), big.data(), o.data(), 1, 4, 100, V, nullptr), "C=100"));
        REQUIRE(refused(lavie_token_embed_f16(ids.data(), big.data(), big.data(), o.data(), 1, 4, C, 0, nullptr), "V=0"));
        REQUIRE(refused(lavie_token_embed_f16(ids.data(), big.data(), big.data(), o.data(), 0, 4, C, V, nullptr), "B=0"));
        REQUIRE(refused(lavie_token_embed_f16(nullptr, big.data(), big.data(), o.data(), 1, 4, C, V, nullptr), "null"));
        REQUIRE(refused(lavie_act_f16(big.data(), 0, 0, nullptr), "n=0"));
        REQUIRE(refused(lavie_act_f16(big.data(), 8, 2, nullptr), "kind=2"));
        REQUIRE(refused(lavie_act_f16(nullptr, 8, 0, nullptr), "null"));
        REQUIRE(lavie_hostcheck_launches() == before);
        REQUIRE(att(qkv.data(), 3 * C + 8, o.data(), C + 8, 2, 128, heads, 32, 0.1f) == 0);
        REQUIRE(lavie_token_embed_f16(ids.data(), big.data(), big.data(), o.data(), 2, 4, C, V, nullptr) == 0);
        REQUIRE(lavie_act_f16(big.data(), 4099, 1, nullptr) == 0 && lavie_act_f16(big.data() + 1, 7, 0, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 4);

        lavie_text_config cfg = {};
        cfg.struct_size = lavie_text_config_size();
        cfg.vocab_size = V; cfg.hidden = C; cfg.intermediate = I; cfg.layers = Lyr; cfg.heads = heads; cfg.max_positions = P;
        cfg.act = LAVIE_TEXT_ACT_QUICK_GELU; cfg.eps = 1e-5f;
        lavie_text_t h = nullptr;
        auto create_with = [&](auto&& change) { lavie_text_config c = cfg; change(c); return lavie_text_create(&c, &h); };
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.struct_size -= 4; }), "struct_size"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.hidden = 96; }), "hidden=96"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.intermediate = 200; }), "intermediate=200"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.layers = 0; }), "layers=0"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.heads = 1; }), "heads=1"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.max_positions = 129; }), "max_positions=129"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.act = 2; }), "act=2"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.vocab_size = 0; }), "vocab_size=0"));
        REQUIRE(refused(create_with([](lavie_text_config& c) { c.eps = 0.f; }), "eps"));
        REQUIRE(refused(lavie_text_create(nullptr, &h), "null") && h == nullptr);
        REQUIRE(lavie_text_create(&cfg, &h) == 0 && h != nullptr);
        REQUIRE(lavie_text_num_params(h) == 2 + 16 * Lyr + 2 && lavie_text_num_params(nullptr) == -1);
        REQUIRE(refused(lavie_text_param_info(h, 99, nullptr, nullptr), "out of range"));
        REQUIRE(refused(lavie_text_set_param(h, "text_model.nope", big.data(), 8), "unknown state-dict key"));
        REQUIRE(refused(lavie_text_set_param(h, "final_layer_norm.bias", big.data(), C), "unknown state-dict key"));      // no flat spelling
        {
            const char *first = nullptr, *last = nullptr;
            REQUIRE(lavie_text_param_info(h, 0, &first, nullptr) == 0 && lavie_text_param_info(h, 2 + 16 * Lyr + 1, &last, nullptr) == 0);
            REQUIRE(!strcmp(first, "text_model.embeddings.token_embedding.weight") && !strcmp(last, "text_model.final_layer_norm.bias"));
        }
        REQUIRE(refused(lavie_text_encode(h, ids.data(), 1, P, o.data(), nullptr), "not finalized"));
        REQUIRE(refused(lavie_text_finalize(h, nullptr), "was never set"));
        std::vector<std::vector<unsigned short>> held;
        for (int i = 0; i < lavie_text_num_params(h); ++i) {
            const char* name = nullptr;
            long long numel = 0;
            REQUIRE(lavie_text_param_info(h, i, &name, &numel) == 0 && name && numel > 0);
            held.emplace_back((size_t)numel, (unsigned short)0x2e66);
            REQUIRE(refused(lavie_text_set_param(h, name, held.back().data(), numel + 1), "expected"));
            REQUIRE(refused(lavie_text_set_param(h, name, nullptr, numel), "null data"));
            REQUIRE(lavie_text_set_param(h, name, held.back().data(), numel) == 0);
        }
        REQUIRE(lavie_text_finalize(h, nullptr) == 0);
        REQUIRE(refused(lavie_text_finalize(h, nullptr), "finalized already"));
        REQUIRE(refused(lavie_text_set_param(h, "text_model.final_layer_norm.bias", big.data(), C), "finalized"));
        held.clear();                                                      // the loan has ended: the handle reads its own copies
        REQUIRE(lavie_text_workspace_bytes(h, 0, P) == -1 && strstr(lavie_last_error(), "B=0"));
        REQUIRE(lavie_text_workspace_bytes(h, 17, P) == -1 && strstr(lavie_last_error(), "B=17"));
        REQUIRE(lavie_text_workspace_bytes(h, 1, P + 1) == -1 && strstr(lavie_last_error(), "L=78"));
        REQUIRE(lavie_text_workspace_bytes(nullptr, 1, 1) == -1);
        REQUIRE(lavie_text_workspace_bytes(h, 16, P) == (long long)16 * P * (2 * C + 3 * C) * 2);
        std::vector<unsigned short> out((size_t)16 * P * C);
        const long e0 = lavie_hostcheck_launches();
        REQUIRE(refused(lavie_text_encode(h, ids.data(), 0, P, out.data(), nullptr), "B=0"));
        REQUIRE(refused(lavie_text_encode(h, ids.data(), 17, P, out.data(), nullptr), "B=17"));
        REQUIRE(refused(lavie_text_encode(h, ids.data(), 1, P + 1, out.data(), nullptr), "L=78"));
        REQUIRE(refused(lavie_text_encode(h, nullptr, 1, P, out.data(), nullptr), "ids_dev"));
        REQUIRE(refused(lavie_text_encode(h, ids.data(), 1, P, nullptr, nullptr), "out_f16"));
        REQUIRE(refused(lavie_text_encode(nullptr, ids.data(), 1, P, out.data(), nullptr), "null handle"));
        REQUIRE(lavie_hostcheck_launches() == e0);
        for (int B : {1, 16}) {
            const long b0 = lavie_hostcheck_launches();
            REQUIRE(lavie_text_encode(h, ids.data(), B, P, out.data(), nullptr) == 0);
            REQUIRE(lavie_hostcheck_launches() == b0 + 2 + 8 * Lyr);       // no split-K reduce, no second kernel at the larger batch
        }
        REQUIRE(lavie_text_destroy(h) == 0 && lavie_text_destroy(nullptr) == 0);
    }
    {   // image conditioning: every refusal of the new operators and of lavie_vision_* / lavie_mapper_* names the
        // argument and launches nothing; accepted encodes walk their launches inside the handles' own, exactly sized allocations
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const int C = 128;
        std::vector<unsigned short> q(2 * 320 * 3 * C + 8), o(2 * 320 * C + 8), big(64 * 1024);
        const long before = lavie_hostcheck_launches();
        auto att = [&](void* qp, int ldq, int ldk, int ldv, int ldo, int NB, int Lq, int Lk, int h, int dh, float sc) {
            return lavie_short_attention_f16(qp, ldq, q.data() + C, ldk, q.data() + 2 * C, ldv, o.data(), ldo, NB, Lq, Lk, h, dh, sc, nullptr);
        };
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 1, 321, 77, 4, 32, 0.1f), "Lq=321"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 1, 77, 321, 4, 32, 0.1f), "Lk=321"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 1, 77, 0, 4, 32, 0.1f), "Lk=0"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 1, 0, 77, 4, 32, 0.1f), "Lq=0"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 1, 77, 77, 4, 40, 0.1f), "dh=40"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 0, 77, 77, 4, 32, 0.1f), "NB=0"));
        REQUIRE(refused(att(q.data(), 3 * C + 4, 3 * C, 3 * C, C, 1, 77, 77, 4, 32, 0.1f), "ldq=388"));
        REQUIRE(refused(att(q.data(), 3 * C, C - 8, 3 * C, C, 1, 77, 77, 4, 32, 0.1f), "ldk=120"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C + 2, C, 1, 77, 77, 4, 32, 0.1f), "ldv=386"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C + 4, 1, 77, 77, 4, 32, 0.1f), "ldo=132"));
        REQUIRE(refused(att(nullptr, 3 * C, 3 * C, 3 * C, C, 1, 77, 77, 4, 32, 0.1f), "null"));
        REQUIRE(refused(att(q.data() + 1, 3 * C, 3 * C, 3 * C, C, 1, 77, 77, 4, 32, 0.1f), "aligned"));
        REQUIRE(refused(att(q.data(), 3 * C, 3 * C, 3 * C, C, 1, 77, 77, 4, 32, INFINITY), "scale"));
        REQUIRE(refused(lavie_relu_f16(big.data(), 0, nullptr), "n=0") && refused(lavie_relu_f16(nullptr, 8, nullptr), "null"));
        REQUIRE(lavie_patch_embed_k(14) == 640 && lavie_patch_embed_k(16) == 768 && lavie_patch_embed_k(0) == -1);
        REQUIRE(lavie_patch_embed_workspace_bytes(2, 56, 14) == 2 * 16 * 640 * 2 && lavie_patch_embed_workspace_bytes(1, 57, 14) == -1);
        std::vector<float> px(2 * 3 * 56 * 56);
        std::vector<unsigned short> wp(C * 640), emb(2 * 17 * C), cols(2 * 16 * 640);
        auto pe = [&](void* x, int dt, int B, int S, int P, int Cc) {
            return lavie_patch_embed_f16(x, dt, wp.data(), big.data(), big.data(), emb.data(), cols.data(), B, S, P, Cc, nullptr);
        };
        REQUIRE(refused(pe(px.data(), 2, 2, 56, 14, C), "x_dtype=2"));
        REQUIRE(refused(pe(px.data(), 1, 0, 56, 14, C), "B=0"));
        REQUIRE(refused(pe(px.data(), 1, 2, 57, 14, C), "S=57"));
        REQUIRE(refused(pe(px.data(), 1, 2, 56, 0, C), "P=0"));
        REQUIRE(refused(pe(px.data(), 1, 2, 56, 14, 96), "C=96"));
        REQUIRE(refused(pe(nullptr, 1, 2, 56, 14, C), "null"));
        REQUIRE(refused(lavie_pack_patch_embed_f16(big.data(), wp.data(), 96, 14, nullptr), "C=96"));
        REQUIRE(lavie_hostcheck_launches() == before);
        REQUIRE(att(q.data(), 3 * C + 8, 3 * C + 8, 3 * C + 8, C + 8, 2, 319, 320, 4, 32, 0.1f) == 0);
        REQUIRE(lavie_relu_f16(big.data(), 4099, nullptr) == 0 && lavie_relu_f16(big.data() + 1, 7, nullptr) == 0);
        REQUIRE(lavie_pack_patch_embed_f16(big.data(), wp.data(), C, 14, nullptr) == 0);
        REQUIRE(pe(px.data(), 1, 2, 56, 14, C) == 0);                      // the gather + one GEMM per image
        REQUIRE(lavie_hostcheck_launches() == before + 1 + 2 + 1 + 1 + 2);

        const int I = 256, Lyr = 2, heads = 4, T = 17;
        lavie_vision_config vc = {};
        vc.struct_size = lavie_vision_config_size();
        vc.hidden = C; vc.intermediate = I; vc.layers = Lyr; vc.heads = heads; vc.image_size = 56; vc.patch_size = 14;
        vc.act = LAVIE_TEXT_ACT_QUICK_GELU; vc.eps = 1e-5f;
        lavie_vision_t vh = nullptr;
        auto vcreate = [&](auto&& change) { lavie_vision_config c = vc; change(c); return lavie_vision_create(&c, &vh); };
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.struct_size -= 4; }), "struct_size"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.hidden = 96; }), "hidden=96"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.intermediate = 200; }), "intermediate=200"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.layers = 0; }), "layers=0"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.heads = 1; }), "heads=1"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.image_size = 57; }), "image_size=57"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.image_size = 336; }), "577 tokens"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.patch_size = 0; }), "patch_size=0"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.act = 2; }), "act=2"));
        REQUIRE(refused(vcreate([](lavie_vision_config& c) { c.eps = 0.f; }), "eps"));
        REQUIRE(refused(lavie_vision_create(nullptr, &vh), "null") && vh == nullptr);
        REQUIRE(lavie_vision_create(&vc, &vh) == 0 && vh != nullptr);
        REQUIRE(lavie_vision_num_params(vh) == 5 + 16 * Lyr && lavie_vision_num_params(nullptr) == -1);
        REQUIRE(refused(lavie_vision_param_info(vh, 99, nullptr, nullptr), "out of range"));
        REQUIRE(refused(lavie_vision_set_param(vh, "vision_model.nope", big.data(), 8), "unknown state-dict key"));
        {
            const char* first = nullptr;
            REQUIRE(lavie_vision_param_info(vh, 0, &first, nullptr) == 0 && !strcmp(first, "vision_model.embeddings.class_embedding"));
        }
        REQUIRE(lavie_vision_set_param(vh, "post_layernorm.weight", big.data(), C) == 0);                  // accepted and ignored,
        REQUIRE(lavie_vision_set_param(vh, "vision_model.post_layernorm.bias", big.data(), C) == 0);       // in either spelling
        REQUIRE(refused(lavie_vision_encode(vh, px.data(), 1, 1, emb.data(), nullptr), "not finalized"));
        REQUIRE(refused(lavie_vision_finalize(vh, nullptr), "was never set"));
        std::vector<std::vector<unsigned short>> held;
        for (int i = 0; i < lavie_vision_num_params(vh); ++i) {
            const char* name = nullptr;
            long long numel = 0;
            REQUIRE(lavie_vision_param_info(vh, i, &name, &numel) == 0 && name && numel > 0);
            held.emplace_back((size_t)numel, (unsigned short)0x2e66);
            REQUIRE(refused(lavie_vision_set_param(vh, name, held.back().data(), numel + 1), "expected"));
            REQUIRE(refused(lavie_vision_set_param(vh, name, nullptr, numel), "null data"));
            // every other tensor under the flat spelling of transformers 5
            REQUIRE(lavie_vision_set_param(vh, (i & 1) ? name + strlen("vision_model.") : name, held.back().data(), numel) == 0);
        }
        REQUIRE(lavie_vision_finalize(vh, nullptr) == 0);
        REQUIRE(refused(lavie_vision_finalize(vh, nullptr), "finalized already"));
        REQUIRE(refused(lavie_vision_set_param(vh, "pre_layrnorm.bias", big.data(), C), "finalized"));
        held.clear();
        REQUIRE(lavie_vision_workspace_bytes(vh, 0) == -1 && strstr(lavie_last_error(), "B=0"));
        REQUIRE(lavie_vision_workspace_bytes(vh, 17) == -1 && strstr(lavie_last_error(), "B=17"));
        REQUIRE(lavie_vision_workspace_bytes(nullptr, 1) == -1);
        REQUIRE(lavie_vision_workspace_bytes(vh, 16) == (long long)16 * T * (2 * C + 3 * C) * 2 + 16 * 16 * 640 * 2);
        std::vector<float> pxl((size_t)16 * 3 * 56 * 56);
        std::vector<unsigned short> vout((size_t)16 * T * C);
        const long v0 = lavie_hostcheck_launches();
        REQUIRE(refused(lavie_vision_encode(vh, pxl.data(), 1, 0, vout.data(), nullptr), "B=0"));
        REQUIRE(refused(lavie_vision_encode(vh, pxl.data(), 1, 17, vout.data(), nullptr), "B=17"));
        REQUIRE(refused(lavie_vision_encode(vh, pxl.data(), 3, 1, vout.data(), nullptr), "x_dtype=3"));
        REQUIRE(refused(lavie_vision_encode(vh, nullptr, 1, 1, vout.data(), nullptr), "pixel_values"));
        REQUIRE(refused(lavie_vision_encode(vh, pxl.data(), 1, 1, nullptr, nullptr), "out_f16"));
        REQUIRE(refused(lavie_vision_encode(nullptr, pxl.data(), 1, 1, vout.data(), nullptr), "null handle"));
        REQUIRE(lavie_hostcheck_launches() == v0);
        for (int B : {1, 16}) {
            const long b0 = lavie_hostcheck_launches();
            REQUIRE(lavie_vision_encode(vh, pxl.data(), 1, B, vout.data(), nullptr) == 0);
            REQUIRE(lavie_hostcheck_launches() == b0 + 2 + B + 8 * Lyr);
        }
        REQUIRE(lavie_vision_destroy(vh) == 0 && lavie_vision_destroy(nullptr) == 0);

        const int Si = 17, So = 7, FF = 256;
        lavie_mapper_config mc = {};
        mc.struct_size = lavie_mapper_config_size();
        mc.input_dim = C; mc.output_dim = C; mc.layers = Lyr; mc.heads = heads; mc.dim_feedforward = FF; mc.seq_in = Si; mc.seq_out = So;
        mc.eps = 1e-5f;
        lavie_mapper_t mh = nullptr;
        auto mcreate = [&](auto&& change) { lavie_mapper_config c = mc; change(c); return lavie_mapper_create(&c, &mh); };
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.struct_size += 4; }), "struct_size"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.input_dim = 100; }), "input_dim=100"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.output_dim = 96; }), "output_dim=96"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.layers = 0; }), "layers=0"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.heads = 3; }), "heads=3"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.dim_feedforward = 200; }), "dim_feedforward=200"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.seq_in = 321; }), "seq_in=321"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.seq_out = 0; }), "seq_out=0"));
        REQUIRE(refused(mcreate([](lavie_mapper_config& c) { c.eps = -1.f; }), "eps"));
        REQUIRE(refused(lavie_mapper_create(&mc, nullptr), "null"));
        REQUIRE(lavie_mapper_create(&mc, &mh) == 0 && mh != nullptr);
        REQUIRE(lavie_mapper_num_params(mh) == 4 + 18 * Lyr && lavie_mapper_num_params(nullptr) == -1);
        REQUIRE(refused(lavie_mapper_param_info(mh, 99, nullptr, nullptr), "out of range"));
        REQUIRE(refused(lavie_mapper_set_param(mh, "nope", big.data(), 8), "unknown state-dict key"));
        REQUIRE(lavie_mapper_set_param(mh, "text_proj.weight", big.data(), C * C) == 0 && lavie_mapper_set_param(mh, "text_proj.bias", big.data(), C) == 0);
        REQUIRE(refused(lavie_mapper_encode(mh, big.data(), 1, big.data(), 1, vout.data(), So, 0, nullptr), "not finalized"));
        REQUIRE(refused(lavie_mapper_finalize(mh, nullptr), "was never set"));
        for (int i = 0; i < lavie_mapper_num_params(mh); ++i) {
            const char* name = nullptr;
            long long numel = 0;
            REQUIRE(lavie_mapper_param_info(mh, i, &name, &numel) == 0 && name && numel > 0);
            held.emplace_back((size_t)numel, (unsigned short)0x2e66);
            REQUIRE(refused(lavie_mapper_set_param(mh, name, held.back().data(), numel - 1), "expected"));
            REQUIRE(refused(lavie_mapper_set_param(mh, name, nullptr, numel), "null data"));
            REQUIRE(lavie_mapper_set_param(mh, name, held.back().data(), numel) == 0);
        }
        REQUIRE(lavie_mapper_finalize(mh, nullptr) == 0);
        REQUIRE(refused(lavie_mapper_finalize(mh, nullptr), "finalized already"));
        REQUIRE(refused(lavie_mapper_set_param(mh, "image_proj.bias", big.data(), C), "finalized"));
        held.clear();
        REQUIRE(lavie_mapper_workspace_bytes(mh, 0) == -1 && strstr(lavie_last_error(), "B=0"));
        REQUIRE(lavie_mapper_workspace_bytes(mh, 17) == -1 && strstr(lavie_last_error(), "B=17"));
        REQUIRE(lavie_mapper_workspace_bytes(nullptr, 1) == -1);
        REQUIRE(lavie_mapper_workspace_bytes(mh, 16) == (long long)16 * Si * 3 * C * 2 + (long long)16 * So * (3 * C + 3 * C) * 2);
        std::vector<unsigned short> img((size_t)16 * Si * C), txt((size_t)16 * So * C), ctx((size_t)16 * 2 * So * C);
        const long m0 = lavie_hostcheck_launches();
        auto enc = [&](void* im, int Bi, void* tx, int B, void* out, int ld, int r0) {
            return lavie_mapper_encode(mh, im, Bi, tx, B, out, ld, r0, nullptr);
        };
        REQUIRE(refused(enc(img.data(), 1, txt.data(), 0, ctx.data(), So, 0), "B=0"));
        REQUIRE(refused(enc(img.data(), 1, txt.data(), 17, ctx.data(), So, 0), "B=17"));
        REQUIRE(refused(enc(img.data(), 2, txt.data(), 3, ctx.data(), So, 0), "Bi=2"));
        REQUIRE(refused(enc(img.data(), 0, txt.data(), 3, ctx.data(), So, 0), "Bi=0"));
        REQUIRE(refused(enc(img.data(), 1, txt.data(), 1, ctx.data(), 2 * So, So + 1), "row0=8"));
        REQUIRE(refused(enc(img.data(), 1, txt.data(), 1, ctx.data(), 2 * So, -1), "row0=-1"));
        REQUIRE(refused(enc(nullptr, 1, txt.data(), 1, ctx.data(), So, 0), "image_feats"));
        REQUIRE(refused(enc(img.data(), 1, nullptr, 1, ctx.data(), So, 0), "text is null"));
        REQUIRE(refused(enc(img.data(), 1, txt.data(), 1, nullptr, So, 0), "out is null"));
        REQUIRE(refused(lavie_mapper_encode(nullptr, img.data(), 1, txt.data(), 1, ctx.data(), So, 0, nullptr), "null handle"));
        REQUIRE(lavie_hostcheck_launches() == m0);
        for (int Bi : {1, 16}) {
            const long b0 = lavie_hostcheck_launches();
            REQUIRE(enc(img.data(), Bi, txt.data(), 16, ctx.data(), 2 * So, So) == 0);      // behind the text rows of a context buffer
            REQUIRE(lavie_hostcheck_launches() == b0 + Bi + 16 + 13 * Lyr);
        }
        REQUIRE(enc(img.data(), 1, txt.data(), 1, ctx.data(), So, 0) == 0);
        REQUIRE(lavie_mapper_destroy(mh) == 0 && lavie_mapper_destroy(nullptr) == 0);
    }
    {   // round 4 operators: widths that are not built, null tensors, a frame height that is not a whole number of 16-row tiles
        REQUIRE(lavie_proj_qkv_image_bytes(256) == 0 && lavie_proj_qkv_image_bytes(320) > 0);
        std::vector<unsigned short> x(64 * 320), wq(3 * 320 * 320), wp(320 * 320), tx(64 * 320), qkv(64 * 960);
        std::vector<unsigned short> img((size_t)lavie_proj_qkv_image_bytes(320) / 2);
        std::vector<float> ab(2 * 320 * 2), v(320, 1.f), ws(1 << 16);
        REQUIRE(lavie_pack_proj_qkv_f16(wp.data(), wq.data(), 256, img.data(), nullptr) != 0);
        REQUIRE(lavie_pack_proj_qkv_f16(wp.data(), wq.data(), 320, img.data(), nullptr) == 0);
        REQUIRE(lavie_group_norm_affine_f16(x.data(), 320, 2, 32, 32, v.data(), v.data(), 1e-6f, ws.data(), ab.data(), nullptr) == 0);
        REQUIRE(lavie_group_norm_affine_f16(x.data(), 320, 2, 32, 32, v.data(), v.data(), 1e-6f, ws.data(), nullptr, nullptr) != 0);
        REQUIRE(lavie_proj_qkv_f16(x.data(), ab.data(), 32, img.data(), v.data(), v.data(), v.data(), 1e-5f, tx.data(), qkv.data(), 64, 320, nullptr) == 0);
        REQUIRE(lavie_proj_qkv_f16(x.data(), ab.data(), 24, img.data(), v.data(), v.data(), v.data(), 1e-5f, tx.data(), qkv.data(), 48, 320, nullptr) != 0);
        REQUIRE(lavie_proj_qkv_f16(x.data(), nullptr, 32, img.data(), v.data(), v.data(), v.data(), 1e-5f, tx.data(), qkv.data(), 64, 320, nullptr) != 0);
        std::vector<float> st(64 * 2, 1.f), s3(960, 0.f);
        REQUIRE(lavie_linear_lnfold_f16(x.data(), wq.data(), v.data(), s3.data(), st.data(), qkv.data(), 64, 960, 320, nullptr) == 0);
        REQUIRE(lavie_linear_lnfold_f16(x.data(), wq.data(), v.data(), nullptr, st.data(), qkv.data(), 64, 960, 320, nullptr) != 0);
        REQUIRE(lavie_linear_lnfold_f16(x.data(), wq.data(), v.data(), s3.data(), st.data(), qkv.data(), 64, 960, 300, nullptr) != 0);
        // GEGLU behind the fold: [64, 960 / 2 ... ] needs N % 128 == 0 (640 of the 960 packed rows are used), null operands and a
        // K off the 64-tile are refused before any HIP call
        const long lg = lavie_hostcheck_launches();
        REQUIRE(lavie_linear_lnfold_geglu_f16(x.data(), wq.data(), v.data(), s3.data(), st.data(), qkv.data(), 64, 640, 320, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == lg + 1);
        REQUIRE(lavie_linear_lnfold_geglu_f16(x.data(), wq.data(), v.data(), s3.data(), nullptr, qkv.data(), 64, 640, 320, nullptr) != 0);
        REQUIRE(lavie_linear_lnfold_geglu_f16(x.data(), wq.data(), v.data(), nullptr, st.data(), qkv.data(), 64, 640, 320, nullptr) != 0);
        REQUIRE(lavie_linear_lnfold_geglu_f16(x.data(), wq.data(), v.data(), s3.data(), st.data(), qkv.data(), 64, 640, 300, nullptr) != 0);
        REQUIRE(lavie_linear_lnfold_geglu_f16(x.data(), wq.data(), v.data(), s3.data(), st.data(), qkv.data(), 64, 960, 320, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "128") != nullptr);
        REQUIRE(lavie_hostcheck_launches() == lg + 1);
    }
    {   // the multistep sampler step: every refusal comes before a HIP call; accepted calls reach the (stubbed) launch, vector body,
        // ragged tail and the one-element-per-lane form under guidance with n % 8 != 0
        alignas(16) static unsigned short eps[2 * 40], min2[2 * 40];
        alignas(16) static float x[40], hist[40];
        const float nan = __builtin_nanf(""), inf = __builtin_inff();
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) == 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, 37, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr) == 0);
        REQUIRE(lavie_multistep_step(eps, x, hist, min2, 37, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 0.9f, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 3);
        REQUIRE(lavie_cfg_multistep_step(nullptr, x, hist, min2, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, nullptr, hist, min2, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, nullptr, min2, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, nullptr, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, 0, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, -8, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, 40, nan, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, inf, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x, hist, min2, 40, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, nan, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps + 1, x, hist, min2, 32, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_cfg_multistep_step(eps, x + 1, hist, min2, 32, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_multistep_step(eps, x, hist + 2, min2, 32, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_multistep_step(eps, x, hist, min2 + 4, 32, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_multistep_step(nullptr, x, hist, min2, 32, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_multistep_step(eps, x, hist, min2, 0, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_multistep_step(eps, x, hist, min2, 32, 1.f, -inf, 1.f, 0.f, 0.f, 1.f, nullptr) != 0);
        REQUIRE(lavie_hostcheck_launches() == before + 3);
    }
    {   // the UniPC step: accepted calls reach the (stubbed) launch in the eight-element form, the one-element form and the table form;
        // every refusal comes before a HIP call and names the argument
        alignas(16) static unsigned short eps[2 * 48], min2[2 * 48];
        alignas(16) static float x[48], xl[48], m1[48], m2[48 + 8], table[4] = {7.5f, 1.f, 5.f, 0.9f};
        const float nan = __builtin_nanf(""), inf = __builtin_inff();
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        lavie_unipc_coeffs k{};
        k.struct_size = (int)sizeof(k); k.corr = 1; k.guidance = 7.5f; k.k_x = 1.f; k.k_eps = 0.5f;
        k.c_l = 0.9f; k.c_0 = 0.05f; k.c_1 = 0.04f; k.c_2 = 0.01f; k.p_x = 0.8f; k.p_0 = 0.3f; k.p_1 = -0.1f; k.next_input_scale = 1.f;
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_cfg_unipc_step(eps, x, xl, m1, m2, min2, 48, k, nullptr) == 0);
        REQUIRE(lavie_cfg_unipc_step(eps, x, xl, m1, m2, min2, 37, k, nullptr) == 0);
        REQUIRE(lavie_unipc_step(eps + 1, x + 1, xl + 1, m1 + 1, m2 + 1, min2 + 1, 37, k, nullptr) == 0);      // one element per lane: no alignment rule
        REQUIRE(lavie_cfg_unipc_step_scaled(eps, x, xl, m1, m2, min2, 48, table, 24, k, nullptr) == 0);
        REQUIRE(lavie_cfg_unipc_step_scaled(eps, x, xl, m1, m2, min2, 30, table, 15, k, nullptr) == 0);
        lavie_unipc_coeffs first = k;
        first.corr = 0; first.p_1 = 0.f;
        REQUIRE(lavie_unipc_step(eps, x, xl, m1, m2, min2, 48, first, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 6);
        lavie_unipc_coeffs q = k;
        q.struct_size = (int)sizeof(k) - 4;
        REQUIRE(refused(lavie_cfg_unipc_step(eps, x, xl, m1, m2, min2, 48, q, nullptr), "struct_size"));
        REQUIRE(refused(lavie_cfg_unipc_step(nullptr, x, xl, m1, m2, min2, 48, k, nullptr), "eps is null"));
        REQUIRE(refused(lavie_cfg_unipc_step(eps, nullptr, xl, m1, m2, min2, 48, k, nullptr), "x is null"));
        REQUIRE(refused(lavie_cfg_unipc_step(eps, x, nullptr, m1, m2, min2, 48, k, nullptr), "x_last is null"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, nullptr, m2, min2, 48, first, nullptr), "m1 is null"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1, nullptr, min2, 48, first, nullptr), "m2 is null"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1, m2, nullptr, 48, k, nullptr), "model_in is null"));
        REQUIRE(refused(lavie_cfg_unipc_step_scaled(eps, x, xl, m1, m2, min2, 48, nullptr, 24, k, nullptr), "table is null"));
        REQUIRE(refused(lavie_cfg_unipc_step(eps, x, xl, m1, m2, min2, 0, k, nullptr), "n=0"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1, m2, min2, -8, k, nullptr), "n=-8"));
        float* const fields[11] = {&q.guidance, &q.k_x, &q.k_eps, &q.c_l, &q.c_0, &q.c_1, &q.c_2, &q.p_x, &q.p_0, &q.p_1, &q.next_input_scale};
        for (int i = 0; i < 11; ++i) {
            q = k;
            *fields[i] = i % 3 == 0 ? nan : i % 3 == 1 ? inf : -inf;
            REQUIRE(refused(lavie_cfg_unipc_step(eps, x, xl, m1, m2, min2, 48, q, nullptr), "not finite"));
        }
        REQUIRE(refused(lavie_cfg_unipc_step(eps + 1, x, xl, m1, m2, min2, 40, k, nullptr), "eps at"));
        REQUIRE(refused(lavie_cfg_unipc_step(eps, x + 1, xl, m1, m2, min2, 40, k, nullptr), "x at"));
        REQUIRE(refused(lavie_cfg_unipc_step(eps, x, xl + 2, m1, m2, min2, 40, k, nullptr), "x_last at"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1 + 3, m2, min2, 40, k, nullptr), "m1 at"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1, m2 + 1, min2, 40, k, nullptr), "m2 at"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1, m2, min2 + 4, 40, k, nullptr), "model_in at"));
        REQUIRE(refused(lavie_cfg_unipc_step_scaled(eps, x, xl + 1, m1, m2, min2, 48, table, 24, k, nullptr), "16-byte"));
        REQUIRE(refused(lavie_unipc_step(eps, x, x, m1, m2, min2, 48, k, nullptr), "x and x_last overlap"));
        REQUIRE(refused(lavie_unipc_step(eps, x, xl, m1, m1 + 8, min2, 40, k, nullptr), "m1 and m2 overlap"));
        REQUIRE(refused(lavie_cfg_unipc_step_scaled(eps, x, xl, m1, m2, min2, 48, table, 1, k, nullptr), "per=1"));
        REQUIRE(refused(lavie_cfg_unipc_step_scaled(eps, x, xl, m1, m2, min2, 48, table, 36, k, nullptr), "whole number"));
        REQUIRE(lavie_hostcheck_launches() == before + 6);
    }
    {   // the steps around known latents: accepted calls reach the (stubbed) launch in the eight-element form (inner % 8 == 0) and the
        // one-element form; every refusal comes before a HIP call and names the argument
        alignas(16) static unsigned short eps[2 * 48], min2[2 * 48];
        alignas(16) static float x[48], hist[48], nz[48], known[48], noise[48], mask[24];
        const float nan = __builtin_nanf(""), inf = __builtin_inff();
        lavie_known_region r{};
        r.struct_size = (int)sizeof(r);
        r.channels = 3; r.inner = 8;                        // P = 2: n = 48
        r.known = known; r.mask = mask; r.noise_known = noise; r.a_next = 0.8f; r.s_next = 0.6f;
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_cfg_sampler_step_known(eps, x, nz, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, &r) == 0);
        REQUIRE(lavie_sampler_step_known(eps, x, nullptr, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, nullptr, &r) == 0);
        REQUIRE(lavie_cfg_multistep_step_known(eps, x, hist, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr, &r) == 0);
        REQUIRE(lavie_multistep_step_known(eps, x, hist, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr, &r) == 0);
        REQUIRE(lavie_known_blend_f32(x, min2, 1, 48, 0.9f, nullptr, &r) == 0);
        lavie_known_region q = r;                           // the end of a run, the add_noise form, the one-element form off alignment
        q.a_next = 1.f; q.s_next = 0.f; q.noise_known = nullptr;
        REQUIRE(lavie_cfg_multistep_step_known(eps, x, hist, min2, 48, 7.5f, 1.f, 0.5f, 1.f, 0.f, 0.f, 1.f, nullptr, &q) == 0);
        q = r; q.mask = nullptr;
        REQUIRE(lavie_known_blend_f32(x, min2, 0, 48, 1.f, nullptr, &q) == 0);
        q = r; q.inner = 7; q.known = known + 1; q.mask = mask + 1; q.noise_known = noise + 3;
        REQUIRE(lavie_sampler_step_known(eps + 1, x + 1, nz + 1, min2 + 1, 42, 1.f, 0.5f, 0.3f, 0.7f, 0.2f, 1.f, nullptr, &q) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 8);
        REQUIRE(refused(lavie_cfg_sampler_step_known(eps, x, nz, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, nullptr), "region"));
        q = r; q.struct_size -= 4;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "struct_size"));
        REQUIRE(refused(lavie_cfg_sampler_step_known(nullptr, x, nz, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, &r), "eps"));
        REQUIRE(refused(lavie_sampler_step_known(eps, nullptr, nz, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, &r), "x is null"));
        REQUIRE(refused(lavie_sampler_step_known(eps, x, nullptr, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, &r), "noise"));
        REQUIRE(refused(lavie_multistep_step_known(eps, x, nullptr, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr, &r), "x0_prev"));
        REQUIRE(refused(lavie_multistep_step_known(eps, x, hist, nullptr, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr, &r), "model_in"));
        q = r; q.known = nullptr;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "known"));
        q = r; q.mask = nullptr;                            // only the blend takes "no mask"
        REQUIRE(refused(lavie_multistep_step_known(eps, x, hist, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr, &q), "mask"));
        q = r; q.noise_known = nullptr;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "noise_known"));
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 40, 1.f, nullptr, &r), "n=40"));
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 0, 1.f, nullptr, &r), "n=0"));
        q = r; q.channels = 0;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "channels"));
        q = r; q.inner = -8;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "inner"));
        q = r; q.a_next = nan;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "a_next"));
        q = r; q.s_next = inf;
        REQUIRE(refused(lavie_cfg_multistep_step_known(eps, x, hist, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr, &q), "s_next"));
        REQUIRE(refused(lavie_cfg_multistep_step_known(eps, x, hist, min2, 48, nan, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr, &r), "finite"));
        REQUIRE(refused(lavie_cfg_sampler_step_known(eps, x, nz, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, inf, nullptr, &r), "finite"));
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, nan, nullptr, &r), "finite"));
        REQUIRE(refused(lavie_cfg_sampler_step_known(eps + 1, x, nz, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, &r), "eps at"));
        REQUIRE(refused(lavie_cfg_sampler_step_known(eps, x, nz + 1, min2, 48, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 1.f, nullptr, &r), "noise at"));
        REQUIRE(refused(lavie_multistep_step_known(eps, x, hist + 2, min2, 48, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr, &r), "x0_prev at"));
        q = r; q.mask = mask + 1;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "region->mask at"));
        q = r; q.noise_known = noise + 2;
        REQUIRE(refused(lavie_known_blend_f32(x, min2, 1, 48, 1.f, nullptr, &q), "region->noise_known at"));
        REQUIRE(lavie_hostcheck_launches() == before + 8);
    }
    {   // the step over overlapping frame windows: accepted calls reach the (stubbed) launch in the eight-element and the one-element
        // form with exactly sized buffers; every refusal comes before a table entry is dereferenced and names its argument
        const int P = 1, C = 2, F = 13, L = 8, hw = 8, nclip = P * C * F * hw, nwin = 2 * P * C * L * hw;
        alignas(16) static float x[nclip + 8], aux[nclip + 8];
        alignas(16) static unsigned short e0[nwin + 8], e1[nwin + 8], m0[nwin + 8], m1[nwin + 8];
        const float nan = __builtin_nanf(""), inf = __builtin_inff();
        int starts[2] = {0, 5};
        float profile[8] = {1, 2, 3, 4, 4, 3, 2, 1};
        const void* eps[2] = {e0, e1};
        void* min_[2] = {m0, m1};
        lavie_window_step_args r{};
        r.struct_size = (int)sizeof(r);
        r.family = 0; r.cfg = 1; r.P = P; r.C = C; r.F = F; r.hw = hw; r.W = 2; r.L = L;
        r.starts_host = starts; r.profile_host = profile; r.eps_host = eps; r.model_in_host = min_;
        r.x = x; r.aux = aux;
        r.guidance = 7.5f; r.k_x = 1.f; r.k_eps = 0.5f; r.c_x0 = 0.3f; r.c_xt = 0.7f; r.c4 = 0.1f; r.next_input_scale = 0.9f;
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_window_step(&r, nullptr) == 0);
        lavie_window_step_args q = r;
        q.family = 1; q.c4 = 0.5f;                          // the multistep family, with and without history, with and without guidance
        REQUIRE(lavie_window_step(&q, nullptr) == 0);
        q.c4 = 0.f; q.cfg = 0;
        REQUIRE(lavie_window_step(&q, nullptr) == 0);
        q = r; q.c4 = 0.f; q.aux = nullptr;                 // sigma == 0: the noise is not read and may be absent
        REQUIRE(lavie_window_step(&q, nullptr) == 0);
        const void* eps_odd[2] = {e0 + 1, e1 + 1};          // the one-element form off alignment: hw = 7 inside the same buffers
        void* min_odd[2] = {m0 + 1, m1 + 1};
        q = r; q.hw = 7; q.x = x + 1; q.aux = aux + 1; q.eps_host = eps_odd; q.model_in_host = min_odd;
        REQUIRE(lavie_window_step(&q, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 5);
        REQUIRE(refused(lavie_window_step(nullptr, nullptr), "args"));
        q = r; q.struct_size -= 4;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "struct_size"));
        q = r; q.family = 2;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "family"));
        q = r; q.C = 0;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "C=0"));
        q = r; q.hw = 0;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "hw=0"));
        q = r; q.P = 4000;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "planes"));
        q = r; q.W = 0;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "W=0"));
        q = r; q.W = 33;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "W=33"));
        q = r; q.L = 0;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "L=0"));
        q = r; q.L = 65;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "L=65"));
        q = r; q.starts_host = nullptr;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "starts_host"));
        q = r; q.profile_host = nullptr;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "profile_host"));
        q = r; q.eps_host = nullptr;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "eps_host"));
        q = r; q.model_in_host = nullptr;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "model_in_host"));
        int bad[2] = {5, 0};
        q = r; q.starts_host = bad;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "ascending"));
        bad[0] = 0; bad[1] = 0;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "ascending"));
        bad[0] = -1; bad[1] = 5;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "starts[0]"));
        bad[0] = 0; bad[1] = 6;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "past F"));
        q = r; q.F = 12;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "past F"));
        q = r; q.L = 4;                                     // frames 4 and 9..12 fall between / behind the windows
        REQUIRE(refused(lavie_window_step(&q, nullptr), "frame 4 is uncovered"));
        int five[5] = {0, 1, 2, 3, 4};                      // frame 4 under five windows of 8 frames
        const void* eps5[5] = {e0, e0, e0, e0, e0};
        void* min5[5] = {m0, m0, m0, m0, m0};
        q = r; q.W = 5; q.F = 12; q.starts_host = five; q.eps_host = eps5; q.model_in_host = min5;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "cover count of 5"));
        float badp[8] = {1, 2, 3, 4, 4, 3, 2, 1};
        q = r; q.profile_host = badp;
        badp[3] = 0.f;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "profile[3]"));
        badp[3] = -1.f;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "profile[3]"));
        badp[3] = 4.f; badp[7] = nan;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "profile[7]"));
        badp[7] = inf;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "profile[7]"));
        const void* eps_null[2] = {e0, nullptr};
        void* min_null[2] = {nullptr, m1};
        q = r; q.eps_host = eps_null;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "eps[1] is null"));
        q = r; q.model_in_host = min_null;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "model_in[0] is null"));
        q = r; q.x = nullptr;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "x is null"));
        q = r; q.aux = nullptr;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "aux is null"));
        q = r; q.family = 1; q.c4 = 0.f; q.aux = nullptr;   // the multistep family always writes its history
        REQUIRE(refused(lavie_window_step(&q, nullptr), "aux is null"));
        q = r; q.aux = x;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "x and aux overlap"));
        q = r; q.aux = x + 8;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "x and aux overlap"));
        void* min_same[2] = {m0, m0 + 16};
        q = r; q.model_in_host = min_same;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "model_in[0] and model_in[1] overlap"));
        void* min_eps[2] = {m0, e0};
        q = r; q.model_in_host = min_eps;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "eps[0] and model_in[1] overlap"));
        void* min_x[2] = {x, m1};
        q = r; q.model_in_host = min_x;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "x and model_in[0] overlap"));
        const void* eps_aux[2] = {e0, aux};
        q = r; q.eps_host = eps_aux;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "aux and eps[1] overlap"));
        q = r; q.guidance = nan;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "guidance"));
        q = r; q.c4 = inf;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "c4"));
        q = r; q.next_input_scale = nan;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "next_input_scale"));
        q = r; q.x = x + 1;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "x at"));
        q = r; q.eps_host = eps_odd;
        REQUIRE(refused(lavie_window_step(&q, nullptr), "eps[0] at"));
        REQUIRE(lavie_hostcheck_launches() == before + 5);
        const void* eps_both[2] = {e0, e0};                  // two windows reading one prediction tensor: only read, accepted
        q = r; q.eps_host = eps_both;
        REQUIRE(lavie_window_step(&q, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 6);
    }
    {   // guidance from a per-latent table: the table's two launches (one when rescale == 0), the five steps that read it in the
        // eight-element and the one-element form with exactly sized buffers; every refusal comes before a launch and names its argument
        const int P = 2, C = 2, inner = 12, per = C * inner, n = P * per;
        alignas(16) static unsigned short eps[2 * n], min2[2 * n];
        alignas(16) static float x[n], nz[n], hist[n], known[n], mask[P * inner], noise[n];
        alignas(16) static float table[2 * 2 * P], gdev[P] = {5.f, 9.f};
        alignas(16) static double moments[4 * P];
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const long long need = lavie_guidance_partials_floats(P, per);
        REQUIRE(need == P * 1 * 4 && lavie_guidance_partials_floats(1, 655360) == 320 * 4 && lavie_guidance_partials_floats(3, 2049) == 3 * 2 * 4);
        REQUIRE(lavie_guidance_partials_floats(0, 8) == -1 && lavie_guidance_partials_floats(1, 1) == -1);
        std::vector<float> partials((size_t)need + 4);
        float* part = partials.data() + (((uintptr_t)partials.data() & 15) ? (16 - ((uintptr_t)partials.data() & 15)) / 4 : 0);
        const void* srcs[1] = {eps};
        lavie_guidance_table_args g{};
        g.struct_size = (int)sizeof(g);
        g.W = 1; g.P = P; g.per = per; g.eps_host = srcs; g.guidance_dev = gdev; g.guidance = 7.5f; g.rescale = 0.7f;
        g.partials = part; g.partials_floats = need; g.table = table; g.moments = moments;
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_guidance_table(&g, nullptr) == 0);                       // moments + fold
        lavie_guidance_table_args h = g;
        h.rescale = 0.f; h.partials = nullptr; h.partials_floats = 0; h.guidance_dev = nullptr; h.moments = nullptr;
        REQUIRE(lavie_guidance_table(&h, nullptr) == 0);                       // the fold alone
        h = g; h.per = per - 1; h.eps_host = srcs;                             // one element per lane: no alignment asked of eps
        const void* odd[1] = {eps + 1};
        h.eps_host = odd;
        REQUIRE(lavie_guidance_table(&h, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 5);
        REQUIRE(refused(lavie_guidance_table(nullptr, nullptr), "args"));
        h = g; h.struct_size -= 8;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "struct_size"));
        h = g; h.W = 0;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "W=0"));
        h = g; h.W = 33;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "W=33"));
        h = g; h.P = 0;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "P=0"));
        h = g; h.P = 70000;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "P=70000"));
        h = g; h.per = 1;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "per=1"));
        h = g; h.eps_host = nullptr;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "eps_host"));
        const void* none[1] = {nullptr};
        h = g; h.eps_host = none;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "eps[0] is null"));
        h = g; h.eps_host = odd;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "eps[0] at"));
        h = g; h.guidance = __builtin_nanf("");
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "guidance"));
        h = g; h.rescale = 1.5f;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "rescale=1.5"));
        h = g; h.rescale = -0.1f;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "rescale"));
        h = g; h.rescale = __builtin_nanf("");
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "rescale"));
        h = g; h.table = nullptr;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "table is null"));
        h = g; h.partials = nullptr;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "partials is null"));
        h = g; h.partials_floats = need - 1;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "partials_floats"));
        h = g; h.partials = part + 1;
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "partials at"));
        h = g; h.moments = (double*)((char*)moments + 4);
        REQUIRE(refused(lavie_guidance_table(&h, nullptr), "moments at"));
        REQUIRE(lavie_hostcheck_launches() == before + 5);
        // the two plain scaled steps
        REQUIRE(lavie_cfg_sampler_step_scaled(eps, x, nz, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr) == 0);
        REQUIRE(lavie_cfg_sampler_step_scaled(eps, x, nullptr, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, nullptr) == 0);
        REQUIRE(lavie_cfg_multistep_step_scaled(eps, x, hist, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr) == 0);
        REQUIRE(lavie_cfg_multistep_step_scaled(eps, x, hist, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr) == 0);
        REQUIRE(lavie_cfg_sampler_step_scaled(eps + 1, x + 1, nz + 1, min2 + 1, 2 * 21, table, 21, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 10);
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x, nz, min2, n, nullptr, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "table is null"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(nullptr, x, nz, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "null argument"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x, nullptr, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "noise is null"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x, nz, min2, n, table, 1, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "per=1"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x, nz, min2, n - 1, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "whole number"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x, nz, min2, 0, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "n=0"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x, nz, min2, n, table, per, 1.f, __builtin_nanf(""), 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "finite"));
        REQUIRE(refused(lavie_cfg_sampler_step_scaled(eps, x + 1, nz, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr), "16-byte"));
        REQUIRE(refused(lavie_cfg_multistep_step_scaled(eps, x, nullptr, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr), "x0_prev"));
        REQUIRE(refused(lavie_cfg_multistep_step_scaled(eps, x, hist + 2, min2, n, table, per, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr), "16-byte"));
        // the two steps around known latents
        lavie_known_region r{};
        r.struct_size = (int)sizeof(r);
        r.channels = C; r.inner = inner; r.known = known; r.mask = mask; r.noise_known = noise; r.a_next = 0.9f; r.s_next = 0.4f;
        REQUIRE(lavie_cfg_sampler_step_known_scaled(eps, x, nz, min2, n, table, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &r) == 0);
        REQUIRE(lavie_cfg_multistep_step_known_scaled(eps, x, hist, min2, n, table, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr, &r) == 0);
        REQUIRE(lavie_cfg_multistep_step_known_scaled(eps, x, hist, min2, n, table, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 1.f, nullptr, &r) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 13);
        REQUIRE(refused(lavie_cfg_sampler_step_known_scaled(eps, x, nz, min2, n, nullptr, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &r), "table is null"));
        REQUIRE(refused(lavie_cfg_multistep_step_known_scaled(eps, x, hist, min2, n, nullptr, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 1.f, nullptr, &r), "table is null"));
        REQUIRE(refused(lavie_cfg_sampler_step_known_scaled(eps, x, nz, min2, n, table, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, nullptr), "region"));
        // the windowed step: P 1, C 2, F 6, L 4, starts 0 and 2, hw 8 then 3
        {
            const int hw = 8, nclip = 1 * 2 * 6 * hw, nwin = 2 * 1 * 2 * 4 * hw;
            alignas(16) static float wx[nclip], waux[nclip], wtable[2 * 1 * 2] = {7.5f, 1.f, 7.5f, 0.9f};
            alignas(16) static unsigned short e0[nwin], e1[nwin], m0[nwin], m1[nwin];
            int starts[2] = {0, 2};
            float profile[4] = {1, 2, 2, 1};
            const void* weps[2] = {e0, e1};
            void* wmin[2] = {m0, m1};
            lavie_window_step_args a{};
            a.struct_size = (int)sizeof(a);
            a.family = 0; a.cfg = 1; a.P = 1; a.C = 2; a.F = 6; a.hw = hw; a.W = 2; a.L = 4;
            a.starts_host = starts; a.profile_host = profile; a.eps_host = weps; a.model_in_host = wmin; a.x = wx; a.aux = waux;
            a.guidance = 1.f; a.k_x = 1.f; a.k_eps = 0.5f; a.c_x0 = 0.3f; a.c_xt = 0.7f; a.c4 = 0.1f; a.next_input_scale = 0.9f;
            REQUIRE(lavie_window_step_scaled(&a, wtable, nullptr) == 0);
            lavie_window_step_args b = a;
            b.family = 1; b.c4 = 0.5f;
            REQUIRE(lavie_window_step_scaled(&b, wtable, nullptr) == 0);
            b.c4 = 0.f;
            REQUIRE(lavie_window_step_scaled(&b, wtable, nullptr) == 0);
            b = a; b.hw = 3;
            REQUIRE(lavie_window_step_scaled(&b, wtable, nullptr) == 0);
            const void* both[2] = {e0, e1};
            lavie_guidance_table_args t = g;
            t.W = 2; t.P = 1; t.per = 2 * 4 * hw; t.eps_host = both; t.guidance_dev = nullptr; t.table = wtable; t.moments = nullptr;
            std::vector<float> wpart((size_t)lavie_guidance_partials_floats(2, t.per) + 4);
            t.partials = wpart.data() + (((uintptr_t)wpart.data() & 15) ? (16 - ((uintptr_t)wpart.data() & 15)) / 4 : 0);
            t.partials_floats = lavie_guidance_partials_floats(2, t.per);
            REQUIRE(lavie_guidance_table(&t, nullptr) == 0);
            REQUIRE(lavie_hostcheck_launches() == before + 19);
            REQUIRE(refused(lavie_window_step_scaled(&a, nullptr, nullptr), "table is null"));
            REQUIRE(refused(lavie_window_step_scaled(nullptr, wtable, nullptr), "args"));
            b = a; b.cfg = 0;
            REQUIRE(refused(lavie_window_step_scaled(&b, wtable, nullptr), "cfg=0"));
            b = a; b.W = 0;
            REQUIRE(refused(lavie_window_step_scaled(&b, wtable, nullptr), "W=0"));
            REQUIRE(lavie_hostcheck_launches() == before + 19);
        }
    }
    {   // seeded engine noise: the host Philox against Random123's known answers, the materialised form, the two seeded plain steps
        // and the seeded window step in both launch forms; every refusal comes before a launch and names its argument
        const int P = 2, per = 24, n = P * per;
        alignas(16) static unsigned short eps[2 * n + 8], min2[2 * n + 8];
        alignas(16) static float x[n + 4], out[n + 4];
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const unsigned kat_key[3][2] = {{0u, 0u}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
        const unsigned kat_ctr[3][4] = {{0u, 0u, 0u, 0u}, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                        {0x243f6a88u, 0x85a308d3u, 0x13198a2e, 0x03707344u}};
        const unsigned kat_out[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                                        {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
        for (int i = 0; i < 3; ++i) {
            unsigned w[4] = {1, 2, 3, 4};
            REQUIRE(lavie_philox4x32_host(kat_key[i], kat_ctr[i], w) == 0 && memcmp(w, kat_out[i], sizeof w) == 0);
        }
        REQUIRE(refused(lavie_philox4x32_host(nullptr, kat_ctr[0], nullptr), "null"));
        unsigned long long seeds[17] = {1, 2, 3};
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_philox_normal_f32(out, seeds, P, per, 0, 5, nullptr) == 0);                      // eight elements per lane
        REQUIRE(lavie_philox_normal_f32(out + 1, seeds, 1, 7, (1ll << 34) - 3, ~0ull, nullptr) == 0);   // one
        REQUIRE(lavie_hostcheck_launches() == before + 2);
        REQUIRE(refused(lavie_philox_normal_f32(nullptr, seeds, P, per, 0, 0, nullptr), "out is null"));
        REQUIRE(refused(lavie_philox_normal_f32(out, nullptr, P, per, 0, 0, nullptr), "seeds_host is null"));
        REQUIRE(refused(lavie_philox_normal_f32(out, seeds, 0, per, 0, 0, nullptr), "P=0"));
        REQUIRE(refused(lavie_philox_normal_f32(out, seeds, 17, per, 0, 0, nullptr), "P=17"));
        REQUIRE(refused(lavie_philox_normal_f32(out, seeds, P, 0, 0, 0, nullptr), "per=0"));
        REQUIRE(refused(lavie_philox_normal_f32(out, seeds, P, per, -1, 0, nullptr), "first_element=-1"));
        REQUIRE(refused(lavie_philox_normal_f32(out, seeds, P, per, (1ll << 62) - per + 1, 0, nullptr), "first_element"));
        REQUIRE(refused(lavie_philox_normal_f32((float*)((char*)out + 2), seeds, P, per, 0, 0, nullptr), "4-byte"));
        lavie_noise_key k{};
        k.struct_size = (int)sizeof(k);
        k.count = P; k.seeds_host = seeds; k.per = per; k.draw = 3;
        REQUIRE(lavie_cfg_sampler_step_seeded(eps, x, min2, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &k) == 0);
        REQUIRE(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, nullptr, &k) == 0);
        lavie_noise_key odd = k;
        odd.count = 1; odd.per = 21;                                                                    // one element per lane: any alignment
        REQUIRE(lavie_cfg_sampler_step_seeded(eps + 1, x + 1, min2 + 1, 21, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &odd) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 5);
        REQUIRE(refused(lavie_cfg_sampler_step_seeded(eps, x, min2, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, nullptr), "key is null"));
        lavie_noise_key q = k;
        q.struct_size -= 8;
        REQUIRE(refused(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &q), "struct_size"));
        q = k; q.count = 17;
        REQUIRE(refused(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &q), "key->count=17"));
        q = k; q.count = 0;
        REQUIRE(refused(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &q), "key->count=0"));
        q = k; q.seeds_host = nullptr;
        REQUIRE(refused(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &q), "seeds_host is null"));
        q = k; q.per = 0;
        REQUIRE(refused(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &q), "key->per=0"));
        REQUIRE(refused(lavie_sampler_step_seeded(eps, x, min2, n - 1, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &k), "is not key->count=2"));
        REQUIRE(refused(lavie_sampler_step_seeded(nullptr, x, min2, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &k), "eps is null"));
        REQUIRE(lavie_hostcheck_launches() == before + 5);
        // no alignment rule and the scalars as they come, as the plain entries: an offset view and a NaN coefficient are launched
        REQUIRE(lavie_cfg_sampler_step_seeded(eps + 8, x + 1, min2 + 8, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &k) == 0);
        REQUIRE(lavie_sampler_step_seeded(eps, x, min2, n, 1.f, __builtin_nanf(""), 0.3f, 0.7f, 0.1f, 0.9f, nullptr, &k) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 7);
        // the launchers' own refusals of a key beside an operand without a seeded form, by name; nothing is launched
        const char* const words[7] = {"", "not combined with `known`", "not combined with `table`", "not combined with `eps_pag`",
                                      "seeded sampler step: the multistep family", "window step: a noise key is not combined with `table`",
                                      "window step: the multistep family"};
        for (int combine = 1; combine <= 6; ++combine) REQUIRE(refused(lavie_debug_noise_key_refusal(combine), words[combine]));
        REQUIRE(refused(lavie_debug_noise_key_refusal(0), "combine=0") && refused(lavie_debug_noise_key_refusal(7), "combine=7"));
        REQUIRE(lavie_hostcheck_launches() == before + 7);
        {   // the windowed step: P 1, C 2, F 6, L 4, starts 0 and 2, hw 8 then 3; aux is not read and may be null
            const int hw = 8, nclip = 1 * 2 * 6 * hw, nwin = 2 * 1 * 2 * 4 * hw;
            alignas(16) static float wx[nclip];
            alignas(16) static unsigned short e0[nwin], e1[nwin], m0[nwin], m1[nwin];
            int starts[2] = {0, 2};
            float profile[4] = {1, 2, 2, 1};
            const void* weps[2] = {e0, e1};
            void* wmin[2] = {m0, m1};
            lavie_window_step_args a{};
            a.struct_size = (int)sizeof(a);
            a.family = 0; a.cfg = 1; a.P = 1; a.C = 2; a.F = 6; a.hw = hw; a.W = 2; a.L = 4;
            a.starts_host = starts; a.profile_host = profile; a.eps_host = weps; a.model_in_host = wmin; a.x = wx; a.aux = nullptr;
            a.guidance = 7.5f; a.k_x = 1.f; a.k_eps = 0.5f; a.c_x0 = 0.3f; a.c_xt = 0.7f; a.c4 = 0.1f; a.next_input_scale = 0.9f;
            lavie_noise_key wk = k;
            wk.count = 1; wk.per = nclip;
            REQUIRE(lavie_window_step_seeded(&a, &wk, nullptr) == 0);
            lavie_window_step_args b = a;
            b.cfg = 0; b.hw = 3;
            wk.per = 2 * 6 * 3;
            REQUIRE(lavie_window_step_seeded(&b, &wk, nullptr) == 0);
            REQUIRE(lavie_hostcheck_launches() == before + 9);
            REQUIRE(refused(lavie_window_step_seeded(&a, &wk, nullptr), "key->count=1 per=36"));
            wk.per = nclip;
            REQUIRE(refused(lavie_window_step_seeded(&a, nullptr, nullptr), "key is null"));
            REQUIRE(refused(lavie_window_step_seeded(nullptr, &wk, nullptr), "args"));
            wk.count = 2;
            REQUIRE(refused(lavie_window_step_seeded(&a, &wk, nullptr), "the clip has P=1"));
            wk.count = 1;
            b = a; b.family = 1;
            REQUIRE(refused(lavie_window_step_seeded(&b, &wk, nullptr), "takes no noise key"));
            REQUIRE(refused(lavie_window_step(&a, nullptr), "aux is null"));                            // without a key the noise is needed
            REQUIRE(lavie_hostcheck_launches() == before + 9);
        }
    }
    {   // the four steps with perturbed-attention guidance: both launch forms with exactly sized buffers; every refusal comes before a
        // launch and names its argument
        const int n = 48;
        alignas(16) static unsigned short eps[3 * n + 8], min3[3 * n + 8];
        alignas(16) static float x[n + 4], nz[n + 4], hist[n + 4];
        const float nan = __builtin_nanf("");
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_cfg_pag_sampler_step(eps, x, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr) == 0);
        REQUIRE(lavie_cfg_pag_sampler_step(eps, x, nullptr, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, 0.f, nullptr) == 0);
        REQUIRE(lavie_pag_sampler_step(eps, x, nz, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr) == 0);
        REQUIRE(lavie_cfg_pag_multistep_step(eps, x, hist, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 0.9f, 3.f, nullptr) == 0);
        REQUIRE(lavie_pag_multistep_step(eps, x, hist, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, 3.f, nullptr) == 0);
        // one element per lane: no alignment asked of anything
        REQUIRE(lavie_cfg_pag_sampler_step(eps + 1, x + 1, nz + 1, min3 + 1, n - 1, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr) == 0);
        REQUIRE(lavie_pag_multistep_step(eps + 1, x + 1, hist + 1, min3 + 1, n - 3, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 0.9f, 3.f, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 7);
        REQUIRE(refused(lavie_cfg_pag_sampler_step(nullptr, x, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "eps is null"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps, nullptr, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "x is null"));
        REQUIRE(refused(lavie_pag_sampler_step(eps, x, nz, nullptr, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "model_in is null"));
        REQUIRE(refused(lavie_pag_sampler_step(eps, x, nullptr, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "noise is null"));
        REQUIRE(refused(lavie_cfg_pag_multistep_step(eps, x, nullptr, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, 3.f, nullptr), "x0_prev is null"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps, x, nz, min3, 0, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "n=0"));
        REQUIRE(refused(lavie_pag_multistep_step(eps, x, hist, min3, -8, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, 3.f, nullptr), "n=-8"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps, x, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, nan, nullptr), "pag_scale"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps, x, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, INFINITY, nullptr), "pag_scale"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps, x, nz, min3, n, nan, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "guidance"));
        REQUIRE(refused(lavie_pag_sampler_step(eps, x, nz, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, nan, 3.f, nullptr), "next_input_scale"));
        REQUIRE(refused(lavie_pag_multistep_step(eps, x, hist, min3, n, 1.f, 0.5f, 0.3f, 0.7f, nan, 0.9f, 3.f, nullptr), "c_prev"));
        REQUIRE(refused(lavie_pag_sampler_step(eps, x, nz, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, -0.5f, nullptr), "pag_scale=-0.5"));
        REQUIRE(refused(lavie_cfg_pag_multistep_step(eps, x, hist, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.5f, 0.9f, -1.f, nullptr), "pag_scale=-1"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps + 1, x, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "eps at"));
        REQUIRE(refused(lavie_cfg_pag_sampler_step(eps, x + 1, nz, min3, n, 7.5f, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "x at"));
        REQUIRE(refused(lavie_pag_sampler_step(eps, x, nz + 2, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "noise at"));
        REQUIRE(refused(lavie_pag_sampler_step(eps, x, nz, min3 + 4, n, 1.f, 0.5f, 0.3f, 0.7f, 0.1f, 0.9f, 3.f, nullptr), "model_in at"));
        REQUIRE(refused(lavie_pag_multistep_step(eps, x, hist + 1, min3, n, 1.f, 0.5f, 0.3f, 0.7f, 0.f, 0.9f, 3.f, nullptr), "x0_prev at"));
        REQUIRE(lavie_hostcheck_launches() == before + 7);
    }
    {   // the VAE's edge convolutions and the asymmetric-pad stride-2 conv: accepted calls reach the (stubbed) launch with exactly
        // sized buffers (packing, odd Cin, ragged last tile); every refusal comes before a HIP call and names its argument
        const int N = 2, Hh = 5, Ww = 7, px = N * Hh * Ww;
        std::vector<unsigned short> w3(128 * 3 * 9), wp3(9 * 4 * 128), x3(N * 3 * Hh * Ww), rows128(px * 128);
        std::vector<unsigned short> wo(3 * 128 * 9), wpo((size_t)lavie_conv_edge_out_image_halfs(128)), y16(N * 3 * Hh * Ww);
        std::vector<float> x3f(N * 3 * Hh * Ww), y32(N * 3 * Hh * Ww), b128(128, 0.f), tb(9 * 128, 0.f), b3(3, 0.f);
        REQUIRE(lavie_conv_edge_out_image_halfs(128) == 9 * 4 * 256 && lavie_conv_edge_out_image_halfs(12) == 0);
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_pack_conv_edge_in_f16(w3.data(), wp3.data(), 128, 3, nullptr) == 0);
        REQUIRE(lavie_conv_edge_in_f16(x3.data(), 0, wp3.data(), b128.data(), nullptr, rows128.data(), N, 3, Hh, Ww, 128, nullptr) == 0);
        REQUIRE(lavie_conv_edge_in_f16(x3f.data(), 1, wp3.data(), b128.data(), tb.data(), rows128.data(), N, 3, Hh, Ww, 128, nullptr) == 0);
        REQUIRE(lavie_pack_conv_edge_out_f16(wo.data(), wpo.data(), 3, 128, nullptr) == 0);
        REQUIRE(lavie_conv_edge_out_f16(rows128.data(), wpo.data(), b3.data(), y16.data(), 0, N, 128, Hh, Ww, 3, nullptr) == 0);
        REQUIRE(lavie_conv_edge_out_f16(rows128.data(), wpo.data(), b3.data(), y32.data(), 1, N, 128, Hh, Ww, 3, nullptr) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 6);
        std::vector<unsigned short> wd(128 * 9 * 128), yd(N * 2 * 3 * 128), zero(128);      // 5 x 7 -> 2 x 3 output pixels per image
        REQUIRE(lavie_conv3x3_down_f16(rows128.data(), 128, wd.data(), b128.data(), yd.data(), N, Hh, Ww, 128, 2, 0, zero.data(), nullptr) == 0);
        const long accepted = lavie_hostcheck_launches();
        REQUIRE(accepted > before + 6);
        REQUIRE(lavie_conv_edge_in_f16(x3.data(), 0, wp3.data(), nullptr, nullptr, rows128.data(), N, 9, Hh, Ww, 128, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "Cin=9") != nullptr);
        REQUIRE(lavie_conv_edge_in_f16(x3.data(), 0, wp3.data(), nullptr, nullptr, rows128.data(), N, 3, Hh, Ww, 100, nullptr) != 0);
        REQUIRE(lavie_conv_edge_in_f16(x3.data(), 2, wp3.data(), nullptr, nullptr, rows128.data(), N, 3, Hh, Ww, 128, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "x_dtype") != nullptr);
        REQUIRE(lavie_conv_edge_in_f16(nullptr, 0, wp3.data(), nullptr, nullptr, rows128.data(), N, 3, Hh, Ww, 128, nullptr) != 0);
        REQUIRE(lavie_pack_conv_edge_in_f16(w3.data(), wp3.data(), 128, 9, nullptr) != 0);
        REQUIRE(lavie_conv_edge_out_f16(rows128.data(), wpo.data(), nullptr, y16.data(), 0, N, 128, Hh, Ww, 9, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "Cout=9") != nullptr);
        REQUIRE(lavie_conv_edge_out_f16(rows128.data(), wpo.data(), nullptr, y16.data(), 0, N, 100, Hh, Ww, 3, nullptr) != 0);
        REQUIRE(lavie_conv_edge_out_f16(rows128.data(), wpo.data(), nullptr, y16.data(), 2, N, 128, Hh, Ww, 3, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "y_dtype") != nullptr);
        REQUIRE(lavie_conv_edge_out_f16(rows128.data(), nullptr, nullptr, y16.data(), 0, N, 128, Hh, Ww, 3, nullptr) != 0);
        REQUIRE(lavie_pack_conv_edge_out_f16(wo.data(), wpo.data(), 9, 128, nullptr) != 0);
        REQUIRE(lavie_conv3x3_down_f16(rows128.data(), 128, wd.data(), nullptr, yd.data(), N, Hh, Ww, 128, 1, 0, zero.data(), nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "pad_lo") != nullptr);
        REQUIRE(lavie_conv3x3_down_f16(rows128.data(), 100, wd.data(), nullptr, yd.data(), N, Hh, Ww, 128, 2, 0, zero.data(), nullptr) != 0);
        REQUIRE(lavie_conv3x3_down_f16(rows128.data(), 128, wd.data(), nullptr, yd.data(), N, Hh, Ww, 128, 2, 0, nullptr, nullptr) != 0);
        REQUIRE(lavie_hostcheck_launches() == accepted);
    }
    {   // the end and glue kernels' entry points: accepted calls reach the (stubbed) launch, every refusal comes before a HIP call
        std::vector<unsigned short> h(4096 * 9);
        std::vector<float> f(4096, 0.f);
        int lab[9] = {0, 4, 4, 0, 0, 0, 0, 0, 0}, lab5[2] = {0, 5}, labm[2] = {-1, 0};
        void* d = h.data();
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_timestep_sinusoid_f32(f.data(), f.data(), 8, 320, nullptr) == 0);
        REQUIRE(lavie_gemv_f16(f.data(), d, f.data(), f.data(), 2, 31, 320, 1, 1, nullptr) == 0);
        REQUIRE(lavie_gemv_f16(f.data(), d, nullptr, f.data(), 8, 32, 2048, 0, 0, nullptr) == 0);
        REQUIRE(lavie_pack_conv_in_f16(d, d, 8, 4, nullptr) == 0 && lavie_conv_in_f16(d, d, f.data(), d, 2, 4, 3, 3, 5, 8, nullptr) == 0);
        REQUIRE(lavie_pack_conv_out_f16(d, d, 4, 64, nullptr) == 0 && lavie_conv_out_f16(d, d, f.data(), d, 2, 336, 3, 3, 5, 4, nullptr) == 0);
        REQUIRE(lavie_conv_out_f16(d, d, f.data(), d, 2, 344, 3, 3, 5, 4, nullptr) == 0 && lavie_conv_out_f16(d, d, f.data(), d, 1, 64, 1, 1, 1, 3, nullptr) == 0);
        REQUIRE(lavie_add_class_emb_silu_f32(f.data(), d, lab, 3, 1024, 5, nullptr) == 0);
        REQUIRE(lavie_fill_relpos_bias_f32(d, (const int*)d, f.data(), 5, 17, 32, nullptr) == 0);
        REQUIRE(lavie_ln_fold_f16(d, f.data(), f.data(), nullptr, d, f.data(), f.data(), 3, 72, nullptr) == 0);
        REQUIRE(lavie_pack_geglu_vec_f32(f.data(), f.data(), 2560, nullptr) == 0);
        REQUIRE(lavie_copy_rows_f16(d, 9, d, 31, 5, 7, 11, nullptr) == 0);
        REQUIRE(lavie_f16_to_f32(d, nullptr, f.data(), 257, nullptr) == 0 && lavie_f16_to_f32(d, d, f.data(), 257, nullptr) == 0);
        const long accepted = lavie_hostcheck_launches();
        REQUIRE(accepted == before + 16);
        REQUIRE(lavie_timestep_sinusoid_f32(f.data(), f.data(), 1, 3, nullptr) != 0 && lavie_timestep_sinusoid_f32(nullptr, f.data(), 1, 2, nullptr) != 0);
        REQUIRE(lavie_gemv_f16(f.data(), d, nullptr, f.data(), 9, 32, 64, 0, 0, nullptr) != 0);
        REQUIRE(lavie_gemv_f16(f.data(), d, nullptr, f.data(), 2, 32, 12, 0, 0, nullptr) != 0);
        REQUIRE(lavie_gemv_f16(f.data(), d, nullptr, f.data(), 8, 32, 2056, 0, 0, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "LDS") != nullptr);
        REQUIRE(lavie_gemv_f16(f.data(), d, nullptr, f.data(), 2, 32, 64, 2, 0, nullptr) != 0 && lavie_gemv_f16(f.data(), nullptr, nullptr, f.data(), 2, 32, 64, 0, 0, nullptr) != 0);
        REQUIRE(lavie_conv_in_f16(d, d, f.data(), d, 1, 7, 1, 1, 2, 8, nullptr) != 0 && lavie_conv_in_f16(d, d, f.data(), d, 1, 4, 1, 1, 2, 12, nullptr) != 0);
        REQUIRE(lavie_conv_in_f16(d, d, f.data(), d, 1, 8, 1, 1, 2, 512, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "LDS") != nullptr);
        REQUIRE(lavie_conv_in_f16(d, d, nullptr, d, 1, 4, 1, 1, 2, 8, nullptr) != 0);
        REQUIRE(lavie_pack_conv_in_f16(d, d, 8, 7, nullptr) != 0 && lavie_pack_conv_in_f16(d, d, 12, 4, nullptr) != 0);
        REQUIRE(lavie_conv_out_f16(d, d, f.data(), d, 1, 60, 1, 1, 2, 4, nullptr) != 0 && lavie_conv_out_f16(d, d, f.data(), d, 1, 64, 1, 1, 2, 9, nullptr) != 0);
        REQUIRE(lavie_conv_out_f16(d, d, f.data(), d, 1, 4096, 1, 1, 2, 8, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "LDS") != nullptr);
        REQUIRE(lavie_pack_conv_out_f16(d, nullptr, 4, 64, nullptr) != 0);
        REQUIRE(lavie_add_class_emb_silu_f32(f.data(), d, lab5, 2, 8, 5, nullptr) != 0 && lavie_add_class_emb_silu_f32(f.data(), d, labm, 2, 8, 5, nullptr) != 0);
        REQUIRE(strstr(lavie_last_error(), "label") != nullptr);
        REQUIRE(lavie_add_class_emb_silu_f32(f.data(), d, lab, 9, 8, 5, nullptr) != 0);
        REQUIRE(lavie_fill_relpos_bias_f32(d, nullptr, f.data(), 8, 16, 32, nullptr) != 0);
        REQUIRE(lavie_ln_fold_f16(d, f.data(), f.data(), nullptr, d, nullptr, f.data(), 3, 72, nullptr) != 0);
        REQUIRE(lavie_pack_geglu_vec_f32(f.data(), f.data(), 48, nullptr) != 0);
        REQUIRE(lavie_copy_rows_f16(d, 7, d, 16, 3, 8, 0, nullptr) != 0 && lavie_copy_rows_f16(d, 8, d, 15, 3, 8, 8, nullptr) != 0);
        REQUIRE(lavie_f16_to_f32(d, nullptr, f.data(), 0, nullptr) != 0 && lavie_f16_to_f32(nullptr, nullptr, f.data(), 4, nullptr) != 0);
        REQUIRE(lavie_hostcheck_launches() == accepted);
    }
    {   // the statistics sink and the two statistics entries: exactly sized buffers; every refusal comes before a launch and names what is wrong
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        std::vector<unsigned short> d16(64);
        void* d = d16.data();
        lavie_op_statistics_info info;
        memset(&info, 0, sizeof(info));
        REQUIRE(refused(lavie_debug_op_statistics_last(nullptr), "out is null"));
        REQUIRE(refused(lavie_debug_op_statistics_last(&info), "struct_size"));
        info.struct_size = (int)sizeof(info);
        const int M = 161, N = 320, K = 320;            // ping-pong under mode 3: three blocks of 80 rows announced, four stored; 128-row kernel: 64-row blocks
        auto lin = [&] { return lavie_linear_f16(d, K, d, nullptr, nullptr, N, 0, nullptr, N, d, N, M, N, K, 0, nullptr); };
        for (int mode : {0, 3}) {
            REQUIRE(lavie_debug_force_tile(mode) == 0);
            REQUIRE(lavie_debug_op_statistics_plan(1, 1) == 0);
            long before = lavie_hostcheck_launches();
            REQUIRE(lin() == 0 && lavie_hostcheck_launches() == before);             // planned, not launched
            REQUIRE(lavie_debug_op_statistics_plan(0, 0) == 0);
            REQUIRE(lavie_debug_op_statistics_last(&info) == 0);
            REQUIRE(info.colstat_written == 1 && info.rowstat_written == 1 && info.splits == 1 && info.nsets == 1 && info.colstat_contiguous == 1);
            REQUIRE(info.set_blocks == (M + info.colstat_rows - 1) / info.colstat_rows && info.colstat_span == info.colstat_rows);
            REQUIRE(info.colstat_rows == (mode == 3 ? 80 : 64) && info.colstat_blocks_stored == 4 && info.colstat_floats == 4ll * 2 * N);
            REQUIRE(info.rowstat_slots * info.rowstat_cols == N && info.rowstat_floats == 2ll * M * info.rowstat_slots);
            std::vector<float> cs((size_t)info.colstat_floats), rs((size_t)info.rowstat_floats);
            REQUIRE(lavie_debug_op_statistics(cs.data(), info.colstat_floats - 1, rs.data(), info.rowstat_floats) == 0);
            before = lavie_hostcheck_launches();
            REQUIRE(refused(lin(), "this launch writes 2560"));
            REQUIRE(lavie_debug_op_statistics(cs.data(), info.colstat_floats, rs.data(), info.rowstat_floats - 1) == 0);
            REQUIRE(refused(lin(), "row-statistics sink holds"));
            REQUIRE(lavie_hostcheck_launches() == before);
            REQUIRE(lavie_debug_op_statistics(cs.data(), info.colstat_floats, rs.data(), info.rowstat_floats) == 0);
            REQUIRE(lin() == 0 && lavie_hostcheck_launches() == before + 1);
            REQUIRE(refused(lavie_debug_op_statistics(cs.data(), -1, nullptr, 0), "negative"));
            REQUIRE(lavie_debug_op_statistics(nullptr, 0, nullptr, 0) == 0);
            REQUIRE(lin() == 0 && lavie_hostcheck_launches() == before + 2);         // disarmed: as before
        }
        REQUIRE(lavie_debug_force_tile(0) == 0);
        // group_norm_stats: 2 domains of 160 rows, 320 channels, blocks of 80 rows
        const int NB = 2, P = 160, C = 320;
        std::vector<unsigned short> x((size_t)NB * P * C), y(x.size());
        std::vector<float> v((size_t)C), ws((size_t)lavie_group_norm_ws_floats(NB, 32)), part((size_t)4 * 2 * C);
        lavie_gn_producer_stats cs;
        memset(&cs, 0, sizeof(cs));
        cs.struct_size = (int)sizeof(cs);
        cs.C = C; cs.partials = part.data(); cs.partials_floats = (long long)part.size(); cs.rows = 80; cs.nsets = 1; cs.set_blocks = 4; cs.span = 80;
        auto gn = [&](const lavie_gn_producer_stats* c1) {
            return lavie_group_norm_stats_f16(x.data(), C, nullptr, 0, NB, P, 32, v.data(), v.data(), 1e-5f, 1, ws.data(), y.data(), c1, nullptr, nullptr);
        };
        long long folds = lavie_debug_gn_producer_count();
        REQUIRE(gn(&cs) == 0 && lavie_debug_gn_producer_count() == folds + 1);
        REQUIRE(gn(nullptr) == 0 && lavie_debug_gn_producer_count() == folds + 1);
        const long accepted = lavie_hostcheck_launches();
        lavie_gn_producer_stats q = cs;
        q.struct_size -= 4;
        REQUIRE(refused(gn(&q), "struct_size"));
        q = cs; q.partials = nullptr;
        REQUIRE(refused(gn(&q), "partials is null"));
        q = cs; q.rows = 0;
        REQUIRE(refused(gn(&q), "rows=0"));
        q = cs; q.partials_floats -= 1;
        REQUIRE(refused(gn(&q), "partials_floats"));
        q = cs; q.set_blocks = 3; q.partials_floats = 3ll * 2 * C;
        REQUIRE(refused(gn(&q), "blocks per set"));
        REQUIRE(refused(lavie_group_norm_stats_f16(nullptr, C, nullptr, 0, NB, P, 32, v.data(), v.data(), 1e-5f, 1, ws.data(), y.data(), &cs, nullptr, nullptr), "null tensor"));
        REQUIRE(refused(lavie_group_norm_stats_f16(x.data(), C, nullptr, 0, 0, P, 32, v.data(), v.data(), 1e-5f, 1, ws.data(), y.data(), &cs, nullptr, nullptr), "empty"));
        // rowstat_finalize
        std::vector<float> rp((size_t)257 * 5 * 2), ro((size_t)257 * 2);
        REQUIRE(refused(lavie_rowstat_finalize_f32(nullptr, 5, 257, 320, 1e-5f, ro.data(), nullptr), "null tensor"));
        REQUIRE(refused(lavie_rowstat_finalize_f32(rp.data(), 5, 257, 320, 1e-5f, nullptr, nullptr), "null tensor"));
        REQUIRE(refused(lavie_rowstat_finalize_f32(rp.data(), 0, 257, 320, 1e-5f, ro.data(), nullptr), "slots=0"));
        REQUIRE(refused(lavie_rowstat_finalize_f32(rp.data(), 5, 0, 320, 1e-5f, ro.data(), nullptr), "M=0"));
        REQUIRE(refused(lavie_rowstat_finalize_f32(rp.data(), 5, 257, 0, 1e-5f, ro.data(), nullptr), "row_len=0"));
        REQUIRE(refused(lavie_rowstat_finalize_f32(rp.data(), 5, 257, 320, -1.f, ro.data(), nullptr), "eps"));
        REQUIRE(lavie_hostcheck_launches() == accepted);
        REQUIRE(lavie_rowstat_finalize_f32(rp.data(), 5, 257, 320, 1e-5f, ro.data(), nullptr) == 0 && lavie_hostcheck_launches() == accepted + 1);
    }
    {   // CLIP image processor, feature heads, CLIPSIM: the host tables at two shapes, the refusals by their texts, two accepted calls
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const int shapes[2][2] = {{53, 320}, {2048, 358}};
        for (const auto& io : shapes) {
            const int in = io[0], out = io[1], ks = lavie_clip_resample_table_host(in, out, nullptr, nullptr, nullptr);
            REQUIRE(ks == (in < out ? 5 : 2 * (int)ceil(2.0 * in / out) + 1));
            std::vector<int> xmin(out), cnt(out), coeff((size_t)out * ks);
            REQUIRE(lavie_clip_resample_table_host(in, out, xmin.data(), cnt.data(), coeff.data()) == ks);
            for (int x = 0; x < out; ++x) {
                long sum = 0;
                for (int t = 0; t < ks; ++t) sum += coeff[(size_t)x * ks + t];
                REQUIRE(xmin[x] >= 0 && cnt[x] >= 1 && cnt[x] <= ks && xmin[x] + cnt[x] <= in && labs(sum - (1l << 22)) <= ks);
            }
        }
        REQUIRE(refused(lavie_clip_resample_table_host(0, 8, nullptr, nullptr, nullptr), "in=0"));
        REQUIRE(refused(lavie_clip_resample_table_host(330, 10, nullptr, nullptr, nullptr), "above 32"));
        std::vector<int> one(8);
        REQUIRE(refused(lavie_clip_resample_table_host(8, 8, one.data(), nullptr, nullptr), "all given or all null"));
        const int H = 64, W = 48, B = 2;
        std::vector<unsigned char> img((size_t)B * H * 3 * W);
        std::vector<float> px((size_t)B * 3 * 224 * 224);
        const long long need = lavie_clip_preprocess_workspace_bytes(B, H, W, 224, 224);
        REQUIRE(need > 0);
        std::vector<unsigned char> ws((size_t)need);
        auto pre = [&](int b, int h, int w, long long pitch, long long ipitch, int dt, const lavie_clip_preprocess_config* c, long long wsb) {
            return lavie_clip_preprocess_u8(img.data(), b, h, w, pitch, ipitch, px.data(), dt, c, ws.data(), wsb, nullptr);
        };
        const long before = lavie_hostcheck_launches();
        REQUIRE(pre(B, H, W, 3 * W, 3ll * W * H, 1, nullptr, need) == 0 && pre(1, H, W, 3 * W, 0, 0, nullptr, need) == 0);
        REQUIRE(lavie_hostcheck_launches() == before + 4);
        REQUIRE(refused(pre(0, H, W, 3 * W, 3ll * W * H, 1, nullptr, need), "B=0"));
        REQUIRE(refused(pre(B, 7, W, 3 * W, 3ll * W * H, 1, nullptr, need), "short edge 7 is below 8"));
        REQUIRE(refused(pre(B, H, W, 3 * W - 1, 3ll * W * H, 1, nullptr, need), "row_pitch=143 is below 3 W = 144"));
        REQUIRE(refused(pre(B, H, W, 3 * W, 100, 1, nullptr, need), "image_pitch=100"));
        REQUIRE(refused(pre(B, H, W, 3 * W, 3ll * W * H, 2, nullptr, need), "out_dtype=2"));
        REQUIRE(refused(pre(B, H, W, 3 * W, 3ll * W * H, 1, nullptr, need - 256), "the workspace holds"));
        lavie_clip_preprocess_config c = {(int)sizeof(lavie_clip_preprocess_config), 8, 8, {0.5f, 0.5f, 0.5f}, {0.5f, 0.5f, 0.5f}};
        REQUIRE(lavie_clip_preprocess_workspace_bytes(1, 300, 300, 8, 8) == -1 && strstr(lavie_last_error(), "is above 32") != nullptr);
        c.size = 32; c.crop = 64;
        REQUIRE(refused(pre(1, H, W, 3 * W, 0, 1, &c, need), "crop=64 is greater than the resized edge 32"));
        c.crop = 32; c.std[1] = 0.f;
        REQUIRE(refused(pre(1, H, W, 3 * W, 0, 1, &c, need), "std[1]"));
        c.std[1] = 0.5f; c.struct_size += 4;
        REQUIRE(refused(pre(1, H, W, 3 * W, 0, 1, &c, need), "struct_size"));
        REQUIRE(lavie_hostcheck_launches() == before + 4);
        std::vector<unsigned short> x16((size_t)2 * 77 * 128), w16((size_t)128 * 128);
        std::vector<float> f(2 * 128), vec(128);
        std::vector<int> ids(2 * 77);
        auto emb = [&](int b, int l, int cc, int d, int row, const float* g, const float* bt) {
            return lavie_clip_embed_f16(x16.data(), b, l, cc, nullptr, 2, row, g, bt, 1e-5f, w16.data(), d, 1, f.data(), nullptr);
        };
        REQUIRE(emb(2, 77, 128, 128, 0, vec.data(), vec.data()) == 0);
        REQUIRE(lavie_clip_embed_f16(x16.data(), 2, 77, 128, ids.data(), 49407, 0, nullptr, nullptr, 0.f, w16.data(), 128, 0, f.data(), nullptr) == 0);
        REQUIRE(refused(emb(0, 77, 128, 128, 0, nullptr, nullptr), "B=0") && refused(emb(2, 77, 192, 128, 0, nullptr, nullptr), "C=192"));
        REQUIRE(refused(emb(2, 77, 128, 2176, 0, nullptr, nullptr), "D=2176") && refused(emb(2, 77, 128, 128, 77, nullptr, nullptr), "row=77"));
        REQUIRE(refused(emb(2, 77, 128, 128, 0, vec.data(), nullptr), "both ln_weight and ln_bias"));
        REQUIRE(lavie_clip_similarity_f32(f.data(), f.data(), f.data(), 2, 2, 128, 0, 14.f, nullptr) == 0);
        REQUIRE(lavie_clip_similarity_f32(f.data(), f.data(), f.data(), 2, 1, 128, 2, 1.f, nullptr) == 0);
        REQUIRE(refused(lavie_clip_similarity_f32(f.data(), f.data(), f.data(), 8, 2, 128, 3, 1.f, nullptr), "N = P frames"));
        REQUIRE(refused(lavie_clip_similarity_f32(f.data(), nullptr, f.data(), 2, 2, 128, 0, 1.f, nullptr), "null tensor"));
        REQUIRE(lavie_hostcheck_launches() == before + 8);
    }
    {   // FVD: the 3-D conv operators, lavie_r3d_* and the video processor: every refusal names its argument and comes
        // before a launch; accepted calls reach the (stubbed) launch with exactly sized buffers
        auto refused = [&](int rc, const char* word) { return rc != 0 && strstr(lavie_last_error(), word) != nullptr; };
        const long before = lavie_hostcheck_launches();
        REQUIRE(lavie_conv3d_packed_halfs(64, 3, 3, 7, 7) == 64 * 448 && lavie_conv3d_packed_halfs(128, 64, 3, 3, 3) == 128 * 27 * 64);
        REQUIRE(lavie_conv3d_packed_halfs(64, 64, 9, 3, 3) == -1 && lavie_conv3d_packed_halfs(0, 64, 3, 3, 3) == -1);
        const int N = 2, T = 3, Hh = 5, Ww = 7;
        std::vector<unsigned short> w16((size_t)128 * 64 * 27), wp((size_t)128 * 27 * 64), x((size_t)N * T * Hh * Ww * 64);
        std::vector<unsigned short> y((size_t)N * T * Hh * Ww * 128), ys((size_t)N * 2 * 3 * 4 * 128);
        std::vector<float> bias(128);
        REQUIRE(lavie_conv3d_pack(w16.data(), wp.data(), 128, 64, 3, 3, 3, nullptr) == 0);
        REQUIRE(refused(lavie_conv3d_pack(nullptr, wp.data(), 128, 64, 3, 3, 3, nullptr), "null tensor"));
        REQUIRE(refused(lavie_conv3d_pack(w16.data(), wp.data(), 128, 64, 3, 8, 3, nullptr), "bad shape"));
        auto conv = [&](const void* xx, const void* ww, const float* bb, void* yy, int n, int t, int cin, int cout, int ks, int st) {
            return lavie_conv3d_f16(xx, ww, bb, nullptr, 1, yy, n, t, Hh, Ww, cin, cout, ks, st, nullptr);
        };
        REQUIRE(conv(x.data(), wp.data(), bias.data(), y.data(), N, T, 64, 128, 3, 1) == 0);
        REQUIRE(conv(x.data(), wp.data(), bias.data(), ys.data(), N, T, 64, 128, 3, 2) == 0);
        REQUIRE(conv(x.data(), wp.data(), bias.data(), ys.data(), N, T, 64, 128, 1, 2) == 0);
        REQUIRE(lavie_conv3d_f16(x.data(), wp.data(), bias.data(), y.data(), 0, y.data(), N, T, Hh, Ww, 64, 128, 3, 1, nullptr) == 0);
        REQUIRE(refused(conv(nullptr, wp.data(), bias.data(), y.data(), N, T, 64, 128, 3, 1), "null tensor"));
        REQUIRE(refused(conv(x.data(), wp.data(), nullptr, y.data(), N, T, 64, 128, 3, 1), "null tensor"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), N, T, 96, 128, 3, 1), "Cin=96"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), N, T, 64, 1024, 3, 1), "Cout=1024"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), N, T, 64, 128, 3, 3), "stride 3 is not built"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), N, T, 64, 128, 1, 1), "(1,1,1) stride 1 is not built"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), N, T, 64, 128, 5, 1), "(5,5,5)"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), N, 0, 64, 128, 3, 1), "T=0"));
        REQUIRE(refused(conv(x.data(), wp.data(), bias.data(), y.data(), 0, T, 64, 128, 3, 1), "N=0"));
        std::vector<float> px((size_t)N * 3 * T * Hh * Ww);
        std::vector<unsigned short> sw((size_t)64 * 448), sy((size_t)N * T * 3 * 4 * 64);
        const long long plane = Hh * Ww;
        auto stem = [&](const void* p, int dt, long long sn, long long st, long long sc, int n, int t) {
            return lavie_conv3d_stem_f16(p, dt, sn, st, sc, sw.data(), bias.data(), 1, sy.data(), n, t, Hh, Ww, nullptr);
        };
        REQUIRE(stem(px.data(), 1, 3 * T * plane, plane, T * plane, N, T) == 0);           // channels-first
        REQUIRE(stem(px.data(), 0, 3 * T * plane, 3 * plane, plane, N, T) == 0);           // frames-major planar (as fp16: half the bytes)
        REQUIRE(refused(stem(nullptr, 1, 3 * T * plane, plane, T * plane, N, T), "null tensor"));
        REQUIRE(refused(stem(px.data(), 2, 3 * T * plane, plane, T * plane, N, T), "x_dtype=2"));
        REQUIRE(refused(stem(px.data(), 1, 3 * T * plane, plane - 1, T * plane, N, T), "strides"));
        REQUIRE(refused(stem(px.data(), 1, 3 * T * plane, plane, T * plane, N, 0), "T=0"));
        REQUIRE(refused(stem(px.data(), 1, 3 * T * plane, plane, T * plane, 0, T), "N=0"));
        std::vector<float> feat((size_t)N * 512);
        REQUIRE(lavie_mean_rows_f32(y.data(), feat.data(), N, T * Hh * Ww, 128, nullptr) == 0);
        REQUIRE(refused(lavie_mean_rows_f32(nullptr, feat.data(), N, 4, 128, nullptr), "null tensor"));
        REQUIRE(refused(lavie_mean_rows_f32(y.data(), feat.data(), N, 0, 128, nullptr), "rows=0"));
        REQUIRE(refused(lavie_mean_rows_f32(y.data(), feat.data(), 0, 4, 128, nullptr), "N=0"));
        REQUIRE(lavie_hostcheck_launches() == before + 8);
        {   // the folded pack at operator level: every refusal before the launch
            std::vector<float> w32((size_t)128 * 64 * 27), bn(128), shift(128);
            auto fold = [&](const float* w, const float* g, const float* v, void* out, float* sh, int kh) {
                return lavie_conv3d_fold_pack_f32(w, g, bn.data(), bn.data(), v, 1e-5, out, sh, 128, 64, 3, kh, 3, nullptr);
            };
            const long at = lavie_hostcheck_launches();
            REQUIRE(fold(w32.data(), bn.data(), bn.data(), wp.data(), shift.data(), 3) == 0 && lavie_hostcheck_launches() == at + 1);
            REQUIRE(refused(fold(nullptr, bn.data(), bn.data(), wp.data(), shift.data(), 3), "null tensor"));
            REQUIRE(refused(fold(w32.data(), bn.data(), bn.data(), nullptr, shift.data(), 3), "null tensor"));
            REQUIRE(refused(fold(w32.data(), nullptr, bn.data(), wp.data(), shift.data(), 3), "null BatchNorm tensor"));
            REQUIRE(refused(fold(w32.data(), bn.data(), nullptr, wp.data(), shift.data(), 3), "null BatchNorm tensor"));
            REQUIRE(refused(fold(w32.data(), bn.data(), bn.data(), wp.data(), nullptr, 3), "null BatchNorm tensor"));
            REQUIRE(refused(fold(w32.data(), bn.data(), bn.data(), wp.data(), shift.data(), 8), "bad shape"));
            REQUIRE(lavie_hostcheck_launches() == at + 1);
        }
        {   // the encoders' own launches at operator level: lavie_pinned_linear_f16 refuses what check_clip_shape keeps
            // the encoders from forming, lavie_add_rows_f16 what the mapper's config does; accepted calls launch once
            const int M = 77, Nn = 256, K = 128;
            void* buf = nullptr;
            REQUIRE(posix_memalign(&buf, 16, (size_t)2 * (M * (K + 64) + Nn * K + 2 * M * (Nn + 128)) + 4 * Nn) == 0);
            memset(buf, 0, (size_t)2 * (M * (K + 64) + Nn * K + 2 * M * (Nn + 128)) + 4 * Nn);
            unsigned short* a = (unsigned short*)buf;
            unsigned short* w = a + M * (K + 64);
            unsigned short* c = w + Nn * K;
            unsigned short* r = c + M * (Nn + 128);
            const float* b = (const float*)(r + M * (Nn + 128));
            auto pin = [&](const void* A, int lda, const void* W, const float* bias, const void* R, int ldr, void* C, int ldc, int m, int n, int k) {
                return lavie_pinned_linear_f16(A, lda, W, bias, R, ldr, C, ldc, m, n, k, nullptr);
            };
            const long at = lavie_hostcheck_launches();
            REQUIRE(pin(a, K, w, b, nullptr, 0, c, Nn, M, Nn, K) == 0);
            REQUIRE(pin(a, K, w, b, c, Nn, c, Nn, M, Nn, K) == 0);                                   // R aliasing C
            REQUIRE(pin(a + 64, K + 64, w, b, r + 128, Nn + 128, c + 128, Nn + 128, M, Nn, K) == 0); // column blocks of wider buffers
            REQUIRE(pin(a, K, w, b, r, Nn + 128, c, Nn, 1, Nn, K) == 0);
            REQUIRE(lavie_hostcheck_launches() == at + 4);
            REQUIRE(refused(pin(nullptr, K, w, b, nullptr, 0, c, Nn, M, Nn, K), "null tensor"));
            REQUIRE(refused(pin(a, K, nullptr, b, nullptr, 0, c, Nn, M, Nn, K), "null tensor"));
            REQUIRE(refused(pin(a, K, w, nullptr, nullptr, 0, c, Nn, M, Nn, K), "null tensor"));
            REQUIRE(refused(pin(a, K, w, b, nullptr, 0, nullptr, Nn, M, Nn, K), "null tensor"));
            REQUIRE(refused(pin(a, K, w, b, nullptr, 0, c, Nn, 0, Nn, K), "M=0"));
            REQUIRE(refused(pin(a, K, w, b, nullptr, 0, c, 192, M, 192, K), "N=192"));
            REQUIRE(refused(pin(a, K, w, b, nullptr, 0, c, 64, M, 64, K), "N=64"));
            REQUIRE(refused(pin(a, 96, w, b, nullptr, 0, c, Nn, M, Nn, 96), "K=96"));
            REQUIRE(refused(pin(a, K, w, b, nullptr, 0, c, Nn, M, Nn, 0), "K=0"));
            REQUIRE(refused(pin(a, K - 8, w, b, nullptr, 0, c, Nn, M, Nn, K), "lda=120"));
            REQUIRE(refused(pin(a, K + 4, w, b, nullptr, 0, c, Nn, M, Nn, K), "lda=132"));
            REQUIRE(refused(pin(a, K, w, b, nullptr, 0, c, Nn - 4, M, Nn, K), "ldc=252"));
            REQUIRE(refused(pin(a, K, w, b, r, Nn + 2, c, Nn, M, Nn, K), "ldr=258"));
            REQUIRE(refused(pin(a + 4, K, w, b, nullptr, 0, c, Nn, M, Nn, K), "16-byte aligned"));
            REQUIRE(refused(pin(a, K, w, b, r + 4, Nn + 128, c, Nn, M, Nn, K), "16-byte aligned"));
            REQUIRE(lavie_hostcheck_launches() == at + 4);
            auto add = [&](const void* x, const void* pos, void* out, int bb, int l, int cc) { return lavie_add_rows_f16(x, pos, out, bb, l, cc, nullptr); };
            REQUIRE(add(a, w, c, 3, 7, 128) == 0 && add(a, w, c, 1, 1, 8) == 0 && lavie_hostcheck_launches() == at + 6);
            REQUIRE(refused(add(nullptr, w, c, 3, 7, 128), "null tensor") && refused(add(a, nullptr, c, 3, 7, 128), "null tensor"));
            REQUIRE(refused(add(a, w, nullptr, 3, 7, 128), "null tensor"));
            REQUIRE(refused(add(a, w, c, 3, 7, 100), "C=100") && refused(add(a, w, c, 3, 7, 0), "C=0"));
            REQUIRE(refused(add(a, w, c, 0, 7, 128), "B=0") && refused(add(a, w, c, 3, 0, 128), "L=0"));
            REQUIRE(refused(add(a + 4, w, c, 3, 7, 128), "16-byte aligned"));
            REQUIRE(lavie_hostcheck_launches() == at + 6);
            free(buf);
        }

        lavie_r3d_t rh = nullptr;
        REQUIRE(refused(lavie_r3d_create(nullptr), "null") && lavie_r3d_create(&rh) == 0 && rh != nullptr);
        REQUIRE(lavie_r3d_num_params(rh) == 100 && lavie_r3d_num_params(nullptr) == -1);
        REQUIRE(refused(lavie_r3d_param_info(rh, 100, nullptr, nullptr), "out of range"));
        std::vector<float> big((size_t)512 * 512 * 27);                        // the largest tensor; every parameter borrows it
        REQUIRE(refused(lavie_r3d_set_param(rh, "layer1.0.downsample.0.weight", big.data(), 64 * 64), "unknown state-dict key"));
        REQUIRE(refused(lavie_r3d_set_param(rh, "5.0.conv1.0.weight", big.data(), 8), "unknown state-dict key"));
        REQUIRE(refused(lavie_r3d_set_param(nullptr, "stem.0.weight", big.data(), 8), "null argument"));
        REQUIRE(refused(lavie_r3d_set_param(rh, nullptr, big.data(), 8), "null argument"));
        REQUIRE(lavie_r3d_set_param(rh, "fc.weight", big.data(), 400 * 512) == 0);                    // accepted and ignored
        REQUIRE(lavie_r3d_set_param(rh, "2.0.conv1.1.num_batches_tracked", big.data(), 1) == 0);      // likewise, numeric prefix
        REQUIRE(refused(lavie_r3d_features(rh, px.data(), 1, 3 * T * plane, plane, T * plane, N, T, Hh, Ww, feat.data(), big.data(), 1 << 20, nullptr),
                        "not finalized"));
        REQUIRE(refused(lavie_r3d_finalize(rh, nullptr), "was never set"));
        REQUIRE(refused(lavie_r3d_finalize(nullptr, nullptr), "null handle"));
        for (int i = 0; i < lavie_r3d_num_params(rh); ++i) {
            const char* name = nullptr;
            long long numel = 0;
            REQUIRE(lavie_r3d_param_info(rh, i, &name, &numel) == 0 && name && numel > 0 && numel <= (long long)big.size());
            REQUIRE(refused(lavie_r3d_set_param(rh, name, big.data(), numel + 1), "expected"));
            REQUIRE(refused(lavie_r3d_set_param(rh, name, nullptr, numel), "null data"));
            std::string key = name;                                            // every other one under its nn.Sequential prefix
            if (i & 1) key = key.compare(0, 4, "stem") == 0 ? "0" + key.substr(4) : key.substr(5);
            REQUIRE(lavie_r3d_set_param(rh, key.c_str(), big.data(), numel) == 0);
        }
        const long packs = lavie_hostcheck_launches();
        REQUIRE(lavie_r3d_finalize(rh, nullptr) == 0 && lavie_hostcheck_launches() == packs + 20);
        REQUIRE(refused(lavie_r3d_finalize(rh, nullptr), "finalized already"));
        REQUIRE(refused(lavie_r3d_set_param(rh, "stem.1.bias", big.data(), 64), "finalized"));
        REQUIRE(lavie_r3d_workspace_bytes(nullptr, 1, 1, 1, 1) == -1);
        REQUIRE(lavie_r3d_workspace_bytes(rh, 0, T, Hh, Ww) == -1 && strstr(lavie_last_error(), "N=0"));
        REQUIRE(lavie_r3d_workspace_bytes(rh, N, T, 0, Ww) == -1 && strstr(lavie_last_error(), "H=0"));
        REQUIRE(lavie_r3d_workspace_bytes(rh, 1, 1, 1, 1) == 2 * 512 * 2 + 512 * 2);        // one row: the 512-channel level is the largest
        const long long need = lavie_r3d_workspace_bytes(rh, N, T, Hh, Ww);
        REQUIRE(need == 2 * (long long)N * T * 3 * 4 * 64 * 2 + (long long)N * 2 * 2 * 2 * 128 * 2);
        std::vector<char> ws((size_t)need);
        auto features = [&](const void* p, int dt, long long st, int n, int t, float* out, void* w, long long bytes) {
            return lavie_r3d_features(rh, p, dt, 3 * T * plane, st, T * plane, n, t, Hh, Ww, out, w, bytes, nullptr);
        };
        const long fwd = lavie_hostcheck_launches();
        REQUIRE(features(px.data(), 1, plane, N, T, feat.data(), ws.data(), need) == 0 && lavie_hostcheck_launches() == fwd + 21);
        REQUIRE(refused(features(px.data(), 1, plane, N, T, feat.data(), ws.data(), need - 1), "the workspace holds"));
        REQUIRE(refused(features(px.data(), 1, plane, N, T, feat.data(), nullptr, need), "the workspace holds 0 bytes"));
        REQUIRE(refused(features(nullptr, 1, plane, N, T, feat.data(), ws.data(), need), "pixels is null"));
        REQUIRE(refused(features(px.data(), 1, plane, N, T, nullptr, ws.data(), need), "out_f32 is null"));
        REQUIRE(refused(features(px.data(), 3, plane, N, T, feat.data(), ws.data(), need), "x_dtype=3"));
        REQUIRE(refused(features(px.data(), 1, plane, 0, T, feat.data(), ws.data(), need), "N=0"));
        REQUIRE(refused(features(px.data(), 1, plane, N, 0, feat.data(), ws.data(), need), "T=0"));
        REQUIRE(refused(features(px.data(), 1, plane - 1, N, T, feat.data(), ws.data(), need), "strides"));
        REQUIRE(refused(lavie_r3d_features(nullptr, px.data(), 1, 3 * T * plane, plane, T * plane, N, T, Hh, Ww, feat.data(), ws.data(), need, nullptr),
                        "null handle"));
        REQUIRE(lavie_hostcheck_launches() == fwd + 21);
        REQUIRE(lavie_r3d_destroy(rh) == 0 && lavie_r3d_destroy(nullptr) == 0);

        int xmin[28], cnt[28], coeff[28 * 5];
        REQUIRE(lavie_video_resample_table_host(34, 28, nullptr, nullptr, nullptr) == 5);
        REQUIRE(lavie_video_resample_table_host(34, 28, xmin, cnt, coeff) == 5 && xmin[0] == 0 && xmin[27] + cnt[27] == 34);
        REQUIRE(lavie_video_resample_table_host(34, 28, xmin, nullptr, coeff) == -1 && strstr(lavie_last_error(), "all given or all null"));
        REQUIRE(lavie_video_resample_table_host(0, 28, nullptr, nullptr, nullptr) == -1 && strstr(lavie_last_error(), "in=0"));
        const int VH = 40, VW = 64;
        const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f}, sd0[3] = {0.229f, 0.f, 0.225f};
        const long long vneed = lavie_video_preprocess_workspace_bytes(2, VH, VW, 34, 28);
        REQUIRE(vneed == (2 * 34 * 28 * 3 + 255) / 256 * 256);
        REQUIRE(lavie_video_preprocess_workspace_bytes(0, VH, VW, 34, 28) == -1 && strstr(lavie_last_error(), "B=0"));
        REQUIRE(lavie_video_preprocess_workspace_bytes(2, VH, VW, 41, 28) == -1 && strstr(lavie_last_error(), "crop=41 is greater than the frame"));
        std::vector<unsigned char> frames((size_t)2 * VH * VW * 3), mid((size_t)vneed);
        std::vector<float> vout((size_t)2 * 3 * 28 * 28);
        auto pre = [&](const void* in, int b, long long pitch, int dt, int crop, int size, const float* m, const float* s, long long bytes) {
            return lavie_video_preprocess_u8(in, b, VH, VW, pitch, (long long)VH * VW * 3, vout.data(), dt, crop, size, m, s, mid.data(), bytes, nullptr);
        };
        const long vbefore = lavie_hostcheck_launches();
        REQUIRE(pre(frames.data(), 2, 3 * VW, 1, 34, 28, mean, sd, vneed) == 0 && pre(frames.data(), 1, 3 * VW, 0, 34, 28, mean, sd, vneed) == 0);
        REQUIRE(lavie_hostcheck_launches() == vbefore + 4);
        REQUIRE(refused(pre(nullptr, 2, 3 * VW, 1, 34, 28, mean, sd, vneed), "null tensor"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 1, 34, 28, nullptr, sd, vneed), "null mean or std"));
        REQUIRE(refused(pre(frames.data(), 0, 3 * VW, 1, 34, 28, mean, sd, vneed), "B=0"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW - 1, 1, 34, 28, mean, sd, vneed), "row_pitch"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 2, 34, 28, mean, sd, vneed), "out_dtype=2"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 1, 41, 28, mean, sd, vneed), "crop=41 is greater than the frame"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 1, 34, 0, mean, sd, vneed), "size=0"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 1, 34, 1, mean, sd, vneed), "above 32"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 1, 34, 28, mean, sd0, vneed), "std[1]"));
        REQUIRE(refused(pre(frames.data(), 2, 3 * VW, 1, 34, 28, mean, sd, vneed - 1), "the workspace holds"));
        REQUIRE(lavie_hostcheck_launches() == vbefore + 4);
    }
    run_vae_optrace();
    REQUIRE(lavie_upsample_conv3x3_supported(320, 32, 20, 32) >= 0);
    int buckets[16 * 16];
    REQUIRE(lavie_relpos_buckets(16, 32, 32, buckets) == 0);
    REQUIRE(buckets[1] == 17 && buckets[16] == 1);                   // row q = 0 starts 0, 17; column k = 0 starts 0, 1
    printf("hostcheck: ok (%ld stubbed kernel launches)\n", lavie_hostcheck_launches());
    return 0;
}
