/* lavie_hip.h — C ABI of liblavie_hip.so: the MI355X (gfx950) implementation of the LaVie base
 * text-to-video denoising path.
 *
 * The reference (rigelshysaj/LaVie) is pure PyTorch and has no plugin/FFI seam; its seam is the
 * Python object protocol of `UNet3DConditionModel.forward` (base/models/unet.py:366-512) and the
 * sub-module forwards below it.  Each entry point cites the reference code it replaces.  The
 * Python facade in lavie_amd/ binds these symbols with ctypes (INTEGRATION.md shows the binding a
 * reference maintainer would add).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in `_host`; `stream` is a hipStream_t
 *    passed as void* (NULL = default stream); kernels are enqueued, never synchronised;
 *  - activations are fp16, CHANNELS-LAST: a video tensor [b, c, f, h, w] of the reference is stored
 *    as rows (b, f, y, x) of c contiguous halfs, which is also the reference's token layout
 *    "(b f) (h w) c" (attention.py:373) — the NCFHW <-> channels-last conversion happens only in
 *    lavie_unet_forward's first and last convolution;
 *  - norm scales/biases and linear biases are fp32 device arrays; weights are fp16;
 *  - the caller owns every buffer it passes; a lavie_unet_t owns its packed weights and workspace;
 *  - return value 0 = ok, negative = error, message from lavie_last_error() (thread local);
 *  - one host thread per process per GPU; no call may run concurrently on the same handle.
 */
#ifndef LAVIE_HIP_H
#define LAVIE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LAVIE_ABI_VERSION 8
#define LAVIE_MAX_LEVELS 8

const char* lavie_last_error(void);
int lavie_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Operators (the finer seam: SURVEY.md §8b "Sub-modules")
 * ---------------------------------------------------------------------------------------------- */

/* C[M,N] = A[M,K] W[N,K]^T (+ bias[N]) (+ bias2[m / rows_per_batch, N]) (+ R[M,N]).
 * Replaces nn.Linear / 1x1 Conv2d: to_q/to_k/to_v/to_out (attention.py:95-104,154,177-178,202),
 * proj_in/proj_out (attention.py:328,356,371,394), FeedForward.net.2 (attention.py:479).
 * geglu != 0: W/bias hold the GEGLU projection in lavie_pack_geglu order and
 * C[M, N/2] = h * gelu_erf(gate) (diffusers GEGLU; spec vsr/models/diffusers_attention.py:801-822).
 * K %% 64 == 0, N %% 64 == 0 (N %% 128 for geglu); R may alias C. */
int lavie_linear_f16(const void* A, int lda, const void* W, const float* bias, const float* bias2, int ldb2,
                     int rows_per_batch, const void* R, int ldr, void* C, int ldc, int M, int N, int K, int geglu,
                     void* stream);

/* Per-frame 3x3 convolution, pad 1, on channels-last images; implicit GEMM.
 * Replaces InflatedConv3d (resnet.py:13-21) as used by ResnetBlock3D.conv1/conv2 (resnet.py:183,200),
 * Downsample3D (stride 2, resnet.py:102-110), Upsample3D (nearest x2 folded into the gather: `ups`=1,
 * resnet.py:62-72), the skip concatenation torch.cat([h, skip]) (x2/C2 != 0, unet_blocks.py:538,630)
 * and the fused 1x1 conv_shortcut (sc1/sc2 appended to K, resnet.py:175,203).
 *   x1,x2 : [NI, Hi, Wi, C1|C2]          Wp : [Cout, 9*(C1+C2) + SC1 + SC2] (lavie_pack_conv3x3 order)
 *   y     : [NI, Ho, Wo, Cout],  Ho = ups ? 2*Hi : (Hi + 2 - 3)/stride + 1
 *   bias2 : per-video bias [NI/frames_per_video... ] see rows_per_batch; R: residual [M, Cout].
 * All channel counts are multiples of 64. */
int lavie_conv3x3_f16(const void* x1, int C1, const void* x2, int C2, const void* sc1, int SC1, const void* sc2, int SC2,
                      const void* Wp, const float* bias, const float* bias2, int ldb2, int rows_per_batch, const void* R,
                      void* y, int NI, int Hi, int Wi, int Cout, int stride, int ups, const void* zero_page,
                      void* stream);

/* The same convolution with a choice of leading pad (additive in ABI 8): one source, no shortcut, residual or per-video bias,
 * weights in lavie_pack_conv3x3_f16 order.  pad_lo = 1 is lavie_conv3x3_f16's geometry.  pad_lo = 0 (stride 2 only; with stride 1
 * the call is refused) is the AutoencoderKL encoder's downsampler, F.pad(x, (0, 1, 0, 1)) followed by a pad-0 stride-2 conv: tap
 * (ky, kx) of output (y, x) reads input (2y + ky, 2x + kx), zeros outside the image, Ho = (Hi - 2)/2 + 1 (odd Hi / Wi included).
 * x [NI, Hi, Wi, C] -> y [NI, Ho, Wo, Cout] channels-last rows; C and Cout multiples of 64.  The planner chooses by (M, N, K) as
 * for pad_lo = 1. */
int lavie_conv3x3_down_f16(const void* x, int C, const void* Wp, const float* bias, void* y, int NI, int Hi, int Wi, int Cout, int stride,
                           int pad_lo, const void* zero_page, void* stream);

/* Edge convolutions of a convolutional autoencoder (additive in ABI 8; csrc/conv_edge.hip): 3x3, pad 1, stride 1,
 * between an NCHW image of at most 8 channels and channels-last fp16 rows.  Both are deterministic (fixed accumulation order, no
 * atomics).
 *   lavie_conv_edge_in_f16 : x [N, Cin, H, W] NCHW, 1 <= Cin <= 8, read in place as fp16 (x_dtype 0) or fp32 (x_dtype 1; rounded to
 *       fp16 on the way in) -> y [N*H*W, Cout] fp16 rows, Cout %% 8 == 0.  bias fp32 [Cout] or NULL.  tap_bias fp32 [9][Cout] or
 *       NULL: entry [ky*3+kx][co] is added to y[pixel][co] exactly when tap (ky, kx) of that pixel lies inside the image, the form
 *       the bias of a 1x1 conv in FRONT of this conv takes when that conv is folded into the weights (the pair zero-pads between
 *       the two).  wp from lavie_pack_conv_edge_in_f16: w [Cout, Cin, 3, 3] fp16 -> 9 * (Cin rounded up to even) * Cout halfs.
 *   lavie_conv_edge_out_f16: x [N*H*W, Cin] fp16 rows, Cin %% 8 == 0 -> y [N, Cout, H, W] NCHW, 1 <= Cout <= 8, written as fp16
 *       (y_dtype 0) or fp32 (y_dtype 1) from fp32 accumulators; bias fp32 [Cout] or NULL.  wp from lavie_pack_conv_edge_out_f16:
 *       w [Cout, Cin, 3, 3] fp16 -> lavie_conv_edge_out_image_halfs(Cin) halfs (0: Cin is not served).
 * A channel count or dtype flag outside these ranges is refused with a message naming the argument; nothing is launched. */
int lavie_pack_conv_edge_in_f16(const void* w, void* out, int Cout, int Cin, void* stream);
int lavie_conv_edge_in_f16(const void* x, int x_dtype, const void* wp, const float* bias, const float* tap_bias, void* y, int N, int Cin,
                           int H, int W, int Cout, void* stream);
long long lavie_conv_edge_out_image_halfs(int Cin);
int lavie_pack_conv_edge_out_f16(const void* w, void* out, int Cout, int Cin, void* stream);
int lavie_conv_edge_out_f16(const void* x, const void* wp, const float* bias, void* y, int y_dtype, int N, int Cin, int H, int W, int Cout,
                            void* stream);

/* [Cout, Cin, 3, 3] (PyTorch) -> rows of `ld_out` halfs in the implicit GEMM's K order (64-channel slab, tap,
 * channel): out[co, col0 + ((ci/64)*9 + ky*3+kx)*64 + ci%64].  Cin %% 64 == 0. */
int lavie_pack_conv3x3_f16(const void* w, void* out, int Cout, int Cin, int ld_out, int col0, void* stream);
/* Temporal convolution over the frame axis on channels-last token rows (b, f, pixel): nn.Conv3d(C, Cout, kernel (T,1,1),
 * padding (T/2,0,0)), T = 3 or 5 — conv1 / conv2 of the VSR stage's ResnetBlock3DCNN (vsr/models/resnet.py:258-259, 274,
 * 285, 309).  Same implicit GEMM as the 3x3 conv with a frame-tap table: tap t of row m reads row
 * m + (t - T/2) * D, zeros outside the clip.  x [B*F*D, C], Wp [Cout, T*C] (lavie_pack_temporal_conv_f16 order),
 * y / R [B*F*D, Cout]; bias2 [B, ldb2] is the per-video time-embedding projection (rows_per_batch = F*D). */
int lavie_temporal_conv_f16(const void* x, int C, const void* Wp, const float* bias, const float* bias2, int ldb2,
                            int rows_per_batch, const void* R, void* y, int B, int F, int D, int Cout, int taps,
                            const void* zero_page, void* stream);
/* [Cout, Cin, T, 1, 1] (PyTorch Conv3d) -> [Cout][T*Cin] in the implicit GEMM's K order (64-channel slab, tap, channel). */
int lavie_pack_temporal_conv_f16(const void* w, void* out, int Cout, int Cin, int taps, void* stream);
/* A GEMM that consumes LayerNorm(A) without the normalised copy (how the engine runs every projection behind a LayerNorm,
 * BasicTransformerBlock attention.py:513-560): C[m, n] = rstd_m (sum_k A[m, k] Wf[n, k] - mean_m s[n]) + bias[n], with
 * Wf = W * gamma (fp16), s = row sums of Wf, bias = W beta (+ the layer's bias) prepared by the caller and ln_stats [M, 2] =
 * (mean, rstd) of the rows of A.  Never splits K. */
int lavie_linear_lnfold_f16(const void* A, const void* Wf, const float* bias, const float* ln_s, const float* ln_stats, void* C,
                            int M, int N, int K, void* stream);
/* The same with the GEGLU epilogue (the feed-forward's first projection behind a folded LayerNorm; additive in this ABI version):
 * C [M, N / 2] = h * gelu(gate) of the folded pre-activations.  Wf, bias and ln_s are in lavie_pack_geglu_f16's row order (pack Wf
 * with it; bias and ln_s take the same row permutation).  N % 128 == 0.  Never splits K. */
int lavie_linear_lnfold_geglu_f16(const void* A, const void* Wf, const float* bias, const float* ln_s, const float* ln_stats, void* C,
                                  int M, int N, int K, void* stream);
/* GEGLU projection [2*inner, K] (+ bias) -> 16-row value/gate interleave expected by lavie_linear_f16(geglu=1). */
int lavie_pack_geglu_f16(const void* w, const void* bias_f16, void* w_out, float* bias_out, int N, int K, void* stream);

/* The forward's end and glue kernels, one entry point per kernel (additive in ABI 8): what the engine launches around the
 * contraction core, callable on the caller's own operands.  Every one is deterministic; an argument outside the stated range is
 * refused and nothing is launched.
 *   lavie_timestep_sinusoid_f32 : Timesteps(dim, flip_sin_to_cos=True, freq_shift=0) (unet.py:153,428): t fp32 [B] -> out fp32
 *       [B, dim] = [cos(t w_k) | sin(t w_k)], w_k = 10000^(-k / (dim/2)); dim even.
 *   lavie_gemv_f16 : out[b, n] = act_out(sum_k act_in(in[b, k]) W[n, k] + bias[n]), in fp32 [B, K], W fp16 [N, K], bias fp32 [N] or
 *       NULL, out fp32 [B, N]; act 0 = none, 1 = SiLU.  TimestepEmbedding and the stacked time_emb_proj (unet.py:434,
 *       resnet.py:186).  1 <= B <= 8, K %% 8 == 0, B * K * 4 <= 65536.  A batch entry's result does not depend on its index.
 *   lavie_pack_conv_in_f16 : w [Cout, Cin, 3, 3] -> out[(k / 2) * Cout * 2 + co * 2 + k %% 2], k = (ky*3+kx) * Cin + ci.
 *   lavie_conv_in_f16 : x [B, Cin, F, H, W] (NCFHW) -> y [(B F) H W, Cout] channels-last rows, 3x3 pad 1 (unet.py:150,454); bias
 *       fp32 [Cout]; Cout %% 8 == 0, Cin even, 9 * Cin * Cout * 2 <= 65536.
 *   lavie_pack_conv_out_f16 : w [Cout, Cin, 3, 3] -> out[co, (ky*3+kx) * Cin + ci].
 *   lavie_conv_out_f16 : x [(B F) H W, Cin] rows -> y [B, Cout, F, H, W] (NCFHW), 3x3 pad 1 (unet.py:290,506); bias fp32 [Cout];
 *       Cout <= 8, Cin %% 8 == 0, 9 * Cin * Cout * 2 <= 65536.
 *   lavie_add_class_emb_silu_f32 : emb[b, :] = silu(emb[b, :] + table[label_b, :]) in place (vsr/models/unet.py:494-505); emb fp32
 *       [B, N], table fp16 [num_classes, N], labels on the host; 1 <= B <= 8, 0 <= label < num_classes.
 *   lavie_fill_relpos_bias_f32 : out[h, i, j] = emb[buckets[i, j], h] (attention.py:669-707); emb fp16 [num_buckets, heads],
 *       buckets int32 [F, F] on the device with every entry in [0, num_buckets) (lavie_relpos_buckets), out fp32 [heads, F, F].
 *   lavie_ln_fold_f16 : the LayerNorm fold lavie_linear_lnfold_f16 consumes: Wout[n, k] = fp16(W[n, k] gamma[k]), s_out[n] = sum_k
 *       Wout[n, k], b_out[n] = sum_k beta[k] W[n, k] (+ bias_f16[n]); W / Wout fp16 [N, K], s_out / b_out fp32 [N].
 *   lavie_pack_geglu_vec_f32 : out[n] = in[row(n)], lavie_pack_geglu_f16's row permutation on an fp32 vector; N %% 32 == 0.
 *   lavie_copy_rows_f16 : dst[r, col0 + c] = src[r, c] for r < rows, c < cols; ld_src >= cols, ld_dst >= col0 + cols.
 *   lavie_f16_to_f32 : dst[i] = float(a[i]) (+ float(b[i]) when b is not NULL), i < n. */
int lavie_timestep_sinusoid_f32(const float* t, float* out, int B, int dim, void* stream);
int lavie_gemv_f16(const float* in, const void* W, const float* bias, float* out, int B, int N, int K, int act_in, int act_out,
                   void* stream);
int lavie_pack_conv_in_f16(const void* w, void* out, int Cout, int Cin, void* stream);
int lavie_conv_in_f16(const void* x_ncfhw, const void* wp, const float* bias, void* y, int B, int Cin, int F, int H, int W, int Cout,
                      void* stream);
int lavie_pack_conv_out_f16(const void* w, void* out, int Cout, int Cin, void* stream);
int lavie_conv_out_f16(const void* x, const void* wp, const float* bias, void* y_ncfhw, int B, int Cin, int F, int H, int W, int Cout,
                       void* stream);
int lavie_add_class_emb_silu_f32(float* emb_inout, const void* table, const int* labels_host, int B, int N, int num_classes, void* stream);
int lavie_fill_relpos_bias_f32(const void* emb, const int* buckets_dev, float* out, int heads, int F, int num_buckets, void* stream);
int lavie_ln_fold_f16(const void* W, const float* gamma, const float* beta, const void* bias_f16, void* Wout, float* s_out, float* b_out, int N,
                      int K, void* stream);
int lavie_pack_geglu_vec_f32(const float* in, float* out, int N, void* stream);
int lavie_copy_rows_f16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, int col0, void* stream);
int lavie_f16_to_f32(const void* a, const void* b, float* dst, long long n, void* stream);

/* Low-rank adapter merge (LoRA on the attention projections; the fork's fine-tuning wraps to_q / to_k / to_v / to_out.0 with a
 * peft LoraConfig, base/pipelines/fine_tuning.py:296-307): out[n, k] = fp16_rne(float(W0[n, k]) + scale * sum_{j < r} B[n, j] A[j, k]).
 * W0 / out fp16 [N, K]; A fp32 [r, K] (lora_A / lora_down); B fp32 [N, r] (lora_B / lora_up).  fp32 accumulation with fmaf in
 * ascending j, one rounding, no atomics: deterministic.  1 <= r <= 128, K %% 8 == 0, W0 / out / A 16-byte aligned, finite scale. */
int lavie_lora_merge_f16(const void* W0, const float* A, const float* B, void* out, int N, int K, int r, float scale, void* stream);
/* Several adapters blended in one pass (additive in ABI 8).  A term with scale 0 is dropped from the list first.  With t_0 =
 * float(W0[n, k]) and, for the remaining terms i = 1 .. T in list order, t_i = fmaf(scale_i, acc_i[n, k], t_{i-1}), where acc_i is the
 * chain of the single merge (fmaf in ascending j over B_i, A_i): out[n, k] = fp16_rne(t_T), one conversion of the finished fp32 sum.
 * W0 is read and out written once per element however many terms there are; no atomics; out may alias W0.  T = 0: out = W0.
 * T = 1: the call is lavie_lora_merge_f16 with that term, so it gives that function's bits.  T >= 2: a further term with A = 0 or
 * B = 0 has acc = +0 and leaves every t_i as it was, so it changes no bit; two runs give the same bits.  (Such a term next to exactly ONE
 * other makes T = 2, and fp16_rne(t_1) may differ in the last bit, in about one element in 10^4, from what the single merge's own last
 * step gives when the compiler fuses its fmaf with the conversion; with scale 0 instead it is dropped and the bits are the single's.)
 * 1 <= n_terms <= LAVIE_LORA_MAX_TERMS; per term 1 <= r <= 128, A 16-byte aligned, finite scale; K %% 8 == 0, W0 / out 16-byte aligned.
 * `terms` is host memory, read before the call returns. */
#define LAVIE_LORA_MAX_TERMS 8
typedef struct lavie_lora_term {
    const float* A;     /* fp32 [r, K] device */
    const float* B;     /* fp32 [N, r] device */
    int r;
    float scale;
} lavie_lora_term;
int lavie_lora_merge_multi_f16(const void* W0, const lavie_lora_term* terms, int n_terms, void* out, int N, int K, void* stream);

/* FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; diffusers' apply_freeu / fourier_filter) on the two operands of a decoder
 * concat (additive in ABI 8).  h [(n y x), C_h] and skip [(n y x), C2] are fp16 channels-last row matrices of NI images of H x W.
 *   h_out    = h with channels [0, C_h / 2) scaled: fp16_rne(float(b) * h); the other channels keep their bits
 *   skip_out = skip with the 2 x 2 block around the centre of every (image, channel)'s shifted 2-D spectrum scaled by s, i.e. the mode
 *              set ky in {0, -1 mod H} x kx in {0, -1 mod W} (1 mode at 1 x 1, 2 at 1 x W or H x 1, else 4), without an FFT:
 *              out = in + (s - 1) / (H W) sum_k [cos phi_k A_k + sin phi_k B_k], A_k / B_k the fp32 cosine / sine sums of the image;
 *              formed in fp32, rounded once to fp16
 * s == 1 / b == 1: that tensor keeps its bits.  h_out may be h and skip_out may be skip (in place: the upper half of h is not touched).
 * Sums run slab by slab in a fixed order without atomics: two runs give the same bits, and an image's result does not depend on how
 * many images the call holds.  workspace: lavie_freeu_workspace_bytes(C2, NI, H, W) bytes (may be NULL when s == 1).  At most two
 * launches, no allocation, no synchronisation (capturable).  Any H, W >= 1; C_h %% 16 == 0, C2 %% 8 == 0, b and s finite and > 0, every
 * pointer 16-byte aligned: anything else is refused before anything is written. */
long long lavie_freeu_workspace_bytes(int C2, int NI, int H, int W);      /* 0 for a shape lavie_freeu_f16 refuses */
int lavie_freeu_f16(const void* h, int C_h, const void* skip, int C2, int NI, int H, int W, float b, float s, void* h_out,
                    void* skip_out, void* workspace, void* stream);

/* FreeInit's frequency mix (Wu et al., "FreeInit: Bridging Initialization Gap in Video Diffusion Models"; diffusers' FreeInitMixin;
 * additive in ABI 8; csrc/freq_mix.hip).  For each of `images` fp32 volumes [F, H, W] (the (video, channel) planes of
 * latents [P, C, F, H, W]):
 *   d           = fma(a, x0, fma(s, e0, -(r z)))                      the sampled latents re-noised to (a, s), minus the fresh noise
 *   out         = fma(Re IFFT3(filter .* FFT3(d)), 1 / (F H W), r z)   unnormalised forward and inverse transforms over (F, H, W)
 *   model_in[j] = fp16(out input_scale), j < dup                      rounded once, as lavie_latents_to_scaled_model_input1; copy j lies
 *                                                                     j dup_stride elements behind model_in
 * filter: fp32 [F, H, W] in FFT-native order (frequency 0 first), shared by all images.  It must be even in frequency,
 * filter[-k] = filter[k] (the caller takes the even part of a filter that is not, which is what the real part of the transform
 * keeps): the kernel computes the real part only.  A separable direct DFT in fp32, six launches; twiddles are tables rounded
 * from fp64, indexed by (k n) mod N.  Every sum runs in ascending order in one accumulator, without atomics: two calls give equal
 * bits and an image has the bits of its single-image call.  out may be x0; no other overlap is allowed.  No allocation, no
 * synchronisation (capturable).  workspace: lavie_freq_mix_workspace_bytes() bytes, 8-byte aligned.
 * Checked before anything is launched, each refusal names its argument: args != NULL and its struct_size; 1 <= images <= 65535,
 * 1 <= F <= 256, 1 <= H, W <= 128; non-null x0 / e0 / z / filter / out / workspace; workspace_bytes; finite a, s, r and input_scale;
 * with model_in: 1 <= dup <= 3 and dup_stride >= images F H W. */
#define LAVIE_FREQ_MIX_MAX_F 256
#define LAVIE_FREQ_MIX_MAX_HW 128
typedef struct lavie_freq_mix_args {
    int struct_size;                  /* sizeof this struct as the CALLER declared it; any other value is refused */
    int images, F, H, W;              /* volumes (videos x channels) and the three transformed axes */
    const float* x0;                  /* [images, F, H, W] fp32, device: the latents a sampling run returned */
    const float* e0;                  /* the same shape: the unit noise the first run started from */
    const float* z;                   /* the same shape: fresh unit noise */
    const float* filter;              /* [F, H, W] fp32, device, FFT-native order, even in frequency */
    float a, s, r;                    /* noise level (a, s) of the last training timestep; r = init_noise_sigma */
    float* out;                       /* [images, F, H, W] fp32, device; may be x0 */
    void* model_in;                   /* fp16, device, or NULL: dup copies of fp16(out input_scale) */
    int dup;                          /* 1..3 copies (read only with model_in) */
    long long dup_stride;             /* elements between two copies, >= images F H W */
    float input_scale;
    void* workspace;                  /* device */
    long long workspace_bytes;
} lavie_freq_mix_args;
long long lavie_freq_mix_workspace_bytes(int images, int F, int H, int W);   /* 0 for a shape the op refuses */
int lavie_freq_mix_f32(const lavie_freq_mix_args* args, void* stream);

/* Fused feed-forward sub-block (ABI 5): y = x + W2 (h * gelu(g)) + b2 with (h, g) = W1 LayerNorm(x) + b1 — the
 * `hidden_states = self.ff(self.norm3(hidden_states)) + hidden_states` line of BasicTransformerBlock
 * (/root/reference/base/models/attention.py:558; FeedForward / GEGLU spec /root/reference/vsr/models/diffusers_attention.py:
 * 734-822) as ONE kernel: the [M, 4C] GEGLU intermediate never exists in memory.  Rows stay in registers from load to store,
 * weights stream through LDS in a packed image (lavie_pack_geglu_mlp_f16).  y may alias x.  Built for C = 320:
 * lavie_geglu_mlp_image_bytes returns 0 for a width the kernel is not built for.
 *   w1 [8C, C] = ff.net.0.proj.weight (value rows, then gate rows), b1 [8C] fp16, w2 [C, 4C] = ff.net.2.weight (fp16 device);
 *   img: lavie_geglu_mlp_image_bytes(C) bytes, b1img: lavie_geglu_mlp_bias_floats(C) floats (device, written by the pack call);
 *   gamma / beta: norm3 weight / bias fp32 [C]; b2: ff.net.2.bias fp32 [C]. */
long long lavie_geglu_mlp_image_bytes(int C);
long long lavie_geglu_mlp_bias_floats(int C);
int lavie_pack_geglu_mlp_f16(const void* w1, const void* b1_f16, const void* w2, int C, void* img, float* b1img, void* stream);
int lavie_geglu_mlp_f16(const void* x, void* y, int M, int C, const void* img, const float* b1img, const float* gamma,
                        const float* beta, const float* b2, float eps, void* stream);

/* Fused temporal sub-block (ABI 5): y = x + to_out(attn_temp(norm_temp(x))) — lines 548-555 of BasicTransformerBlock.forward
 * with TemporalAttention.forward / _attention (/root/reference/base/models/attention.py:580-667) as ONE kernel on token rows in
 * (b f) d order: LayerNorm, the q / k / v projections, scale + rotary, relative-position bias, softmax over the frames of a
 * pixel, P V, to_out + bias + residual.  Neither q|k|v nor the attention output exists in memory; the two rearranges of the
 * reference are row addressing.  y may alias x.  Built for C = 320, 8 heads, exactly 16 frames, rotary over 32 channels:
 * lavie_temporal_block_image_bytes returns 0 otherwise.
 *   wq / wk / wv / wo: attn_temp.to_q / to_k / to_v / to_out.0 weights [C, C] fp16 (device); img: image bytes (device);
 *   gamma / beta: norm_temp fp32 [C]; bo: to_out.0.bias fp32 [C]; relbias fp32 [heads, F, F] (query, key);
 *   rot_cos / rot_sin fp32 [F, rot_dim / 2]; scale = dim_head^-0.5 (applied to q before the rotary embedding, :640). */
long long lavie_temporal_block_image_bytes(int C, int heads, int F, int rot_dim);
int lavie_pack_temporal_block_f16(const void* wq, const void* wk, const void* wv, const void* wo, int C, void* img, void* stream);
int lavie_temporal_block_f16(const void* x, void* y, int B, int F, int D, int C, int heads, const void* img, const float* gamma,
                             const float* beta, const float* bo, const float* relbias, const float* rot_cos,
                             const float* rot_sin, int rot_dim, float scale, float eps, void* stream);

/* Fused text cross-attention sub-block (ABI 6): with att = the output of attn1's attention core (before its to_out),
 *     x'  = x + attn1.to_out(att)                                   (attention.py:513-522, the projection and residual)
 *     y   = x' + attn2.to_out(attn2(norm2(x'), K, V))               (attention.py:524-534; CrossAttention :253-335)
 * as ONE kernel: q, the attention output, norm2(x') and x' never exist in memory.  K / V = attn2.to_k / to_v of the text
 * context are per-video constants; they travel inside the weight stream: lavie_pack_cross_block_f16 writes the weight part of
 * an image once per model, lavie_bind_cross_block_f16 completes one image per video from kv [B * ctx_len, 2C] (k | v rows,
 * fp16) once per context.  Rows [M, C] of video b are rows [b * rows_per_batch, (b + 1) * rows_per_batch) (rows_per_batch =
 * frames * pixels, a multiple of 16).  y may alias x.  Built for C = 320, 8 heads, ctx_len <= 80:
 * lavie_cross_block_image_bytes returns 0 otherwise.
 *   wo1 / wq2 / wo2: attn1.to_out.0 / attn2.to_q / attn2.to_out.0 weights [C, C] fp16 (device); tmpl: image bytes;
 *   img: B * image bytes (device); bo1 / bo2: the to_out biases fp32 [C]; gamma / beta: norm2 fp32 [C]; scale = dim_head^-0.5. */
long long lavie_cross_block_image_bytes(int C, int heads);
int lavie_pack_cross_block_f16(const void* wo1, const void* wq2, const void* wo2, int C, void* tmpl, void* stream);
int lavie_bind_cross_block_f16(const void* tmpl, const void* kv, int B, int ctx_len, int C, void* img, void* stream);
int lavie_cross_block_f16(const void* att, const void* x, void* y, int M, int rows_per_batch, int C, int heads, const void* img,
                          const float* bo1, const float* gamma, const float* beta, const float* bo2, int ctx_len, float scale,
                          float eps, void* stream);
/* The long variant (additive in ABI 8): the same sub-block for 81 <= ctx_len <= 160 (a text context widened with mapped image
 * tokens), with images of its own layout and size: a template from lavie_pack_cross_block_long_f16, per-video images from
 * lavie_bind_cross_block_long_f16, launched by lavie_cross_block_long_f16.  Arguments as above; C = 320, 8 heads;
 * lavie_cross_block_long_image_bytes returns 0 for any other width or head count.  Images of the two variants do not mix. */
long long lavie_cross_block_long_image_bytes(int C, int heads);
int lavie_pack_cross_block_long_f16(const void* wo1, const void* wq2, const void* wo2, int C, void* tmpl, void* stream);
int lavie_bind_cross_block_long_f16(const void* tmpl, const void* kv, int B, int ctx_len, int C, void* img, void* stream);
int lavie_cross_block_long_f16(const void* att, const void* x, void* y, int M, int rows_per_batch, int C, int heads, const void* img,
                               const float* bo1, const float* gamma, const float* beta, const float* bo2, int ctx_len, float scale,
                               float eps, void* stream);

/* Upsample3D (ABI 6, /root/reference/base/models/resnet.py:44-79: F.interpolate(scale_factor=2, mode="nearest") then the 3x3
 * conv): y = conv3x3(nearest_x2(x)) + bias as FOUR 2x2 convs on x, one per output parity — the nine taps of an output pixel
 * fall on 2 x 2 source pixels, so the weights of coinciding taps are summed once at pack time (fp32 sum, one rounding) and the
 * product needs 4 C instead of 9 C multiply-adds per output element.  Same result as lavie_conv3x3_f16(..., ups = 1) up to that
 * rounding.  x [NI * Hi * Wi, C] rows, y [NI * 2Hi * 2Wi, C] rows.
 *   lavie_pack_conv3x3_parity_f16: w [C, C, 3, 3] fp16 (PyTorch layout) -> out [4][C][4 C] fp16 (device);
 *   lavie_upsample_conv3x3_supported: 1 when the geometry fits the kernel (C % 160 == 0, whole source rows per 320-pixel tile);
 *   otherwise use lavie_conv3x3_f16 with ups = 1. */
int lavie_pack_conv3x3_parity_f16(const void* w, void* out, int Cout, int Cin, void* stream);
int lavie_upsample_conv3x3_supported(int NI, int Hi, int Wi, int C);
int lavie_upsample_conv3x3_f16(const void* x, const void* wpar, const float* bias, void* y, int NI, int Hi, int Wi, int C,
                               const void* zero_page, void* stream);

/* GroupNorm (+ optional SiLU) over channels-last rows; the "batch" is whatever shares statistics:
 *   video domain  (resnet.py:180,191; unet.py:504): NB = b,   P = f*h*w   rows per batch
 *   frame domain  (attention.py:324,369)          : NB = b*f, P = h*w
 * Input may be the virtual concat [x1 | x2].  stats_ws: lavie_group_norm_ws_floats(NB, groups) floats of
 * scratch (slab partials + mean/rstd; no atomics: results are bit-reproducible). */
long long lavie_group_norm_ws_floats(int NB, int groups);
int lavie_group_norm_f16(const void* x1, int C1, const void* x2, int C2, int NB, int P, int groups, const float* gamma,
                         const float* beta, float eps, int silu, float* stats_ws, void* y, void* stream);

/* Fused head of the transformer block (ABI 7, round 4): with GN = the per-frame GroupNorm of Transformer3DModel (attention.py:369),
 *     tx  = proj_in(GN(x))                               (attention.py:371-373: 1x1 conv, then tokens)
 *     qkv = [to_q | to_k | to_v](norm1(tx))              (attention.py:513-516 with CrossAttention :154, 177-178)
 * as ONE kernel: the normalised copy of x, norm1's statistics and the re-read of tx never exist in memory.  The GroupNorm is handed
 * over as per-(frame, channel) pairs (a, b), y = a x + b: lavie_group_norm_affine_f16 computes the statistics (as
 * lavie_group_norm_f16 does) and writes ab_out [NB][C][2] instead of a normalised tensor.  rows_per_domain = rows per frame (a
 * multiple of 16 that divides M).  Built for C = 320: lavie_proj_qkv_image_bytes returns 0 otherwise.
 *   wpin [C, C] = proj_in.weight (1x1 conv or Linear), wqkv [3C, C] = attn1.to_q / to_k / to_v rows stacked (fp16, device);
 *   bpin: proj_in.bias fp32 [C]; ln_gamma / ln_beta: norm1 fp32 [C]; tx [M, C], qkv [M, 3C] fp16 out. */
long long lavie_proj_qkv_image_bytes(int C);
int lavie_pack_proj_qkv_f16(const void* wpin, const void* wqkv, int C, void* img, void* stream);
int lavie_group_norm_affine_f16(const void* x, int C, int NB, int P, int groups, const float* gamma, const float* beta, float eps,
                                float* stats_ws, float* ab_out, void* stream);
int lavie_proj_qkv_f16(const void* x, const float* gn_ab, int rows_per_domain, const void* img, const float* bpin, const float* ln_gamma,
                       const float* ln_beta, float ln_eps, void* tx, void* qkv, int M, int C, void* stream);

/* nn.LayerNorm(C) over rows (attention.py:442,459,474,480). */
int lavie_layer_norm_f16(const void* x, const float* gamma, const float* beta, void* y, int rows, int C, float eps,
                         void* stream);

/* softmax(scale q k^T) v with heads packed along channels; replaces CrossAttention._attention
 * (attention.py:209-239) and reshape_heads_to_batch_dim / reshape_batch_dim_to_heads (112-124).
 * q: [NB*Lq, ldq], k/v: [(NB/kv_batch_div)*Lk, ld], o: [NB*Lq, ldo]; head h at columns h*dh.
 * Head dims: every multiple of 8 up to 160 (the UNets), and 256 / 512 (attention_wide.hip: the single head of the
 * AutoencoderKL mid block, e.g. NB 1, Lq = Lk = 163,840, dh 512); any other head dim is refused with a message that
 * names this set. */
int lavie_attention_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int NB,
                        int Lq, int Lk, int heads, int dh, int kv_batch_div, float scale, void* stream);

/* SparseCausalAttention (interpolation/models/attention.py:609-665): spatial self-attention whose keys/values for
 * frame f of a video are the D tokens of the video's FIRST frame followed by the D tokens of frame max(f-1, 0)
 * (:630-639), i.e. 2 D keys per query; the concatenation is never materialised — the kernel stages both segments
 * straight from the per-frame K/V rows.  q/k/v/o: [NB*D, ld] rows, NB = videos * frames, NB %% frames == 0. */
int lavie_sparse_causal_attention_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o,
                                      int ldo, int NB, int frames, int D, int heads, int dh, float scale, void* stream);

/* TemporalAttention._attention (attention.py:634-667) on tokens ordered (b, f, pixel):
 * qkv [B*F*D, ld] = q | k | v, o [B*F*D, ldo]; bias [heads, F, F] fp32 (query, key);
 * rot_cos/rot_sin [F, rot_dim/2] fp32.  rot_dim = 0 (tables may be NULL) and an all-zero bias give the plain
 * softmax(scale q k^T) v over frames of the interpolation model's attn_temp (interpolation/models/attention.py:
 * 268-289, 596-603). */
int lavie_temporal_attention_f16(const void* qkv, int ld, void* o, int ldo, int B, int F, int D, int heads, int dh,
                                 const float* bias, const float* rot_cos, const float* rot_sin, int rot_dim, float scale,
                                 void* stream);

/* T5-style relative position buckets of RelativePositionBias (attention.py:681-699), HOST function:
 * out_host[i*F + j] = bucket(query i, key j). */
int lavie_relpos_buckets(int F, int num_buckets, int max_distance, int* out_host);

/* Classifier-free guidance + DDPM ancestral step, fused (pipeline_videogen.py:679-683 and
 * diffusers DDPMScheduler.step): eps2 = [uncond | cond] fp16 (n each), x fp32 (updated in place),
 * noise fp32 (may be NULL iff sigma == 0), model_in2 = fp16 [x' | x'] for the next UNet call. */
int lavie_cfg_ddpm_step(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float guidance,
                        float k_x, float k_eps, float c_x0, float c_xt, float sigma, void* stream);
int lavie_latents_to_model_input(const float* x, void* model_in2, long long n, void* stream);
/* Same two kernels for schedulers whose `scale_model_input` is not the identity (EulerDiscreteScheduler, sample_method
 * 'eulerdiscrete', base/pipelines/sample.py:50-55; pipeline_videogen.py:667): the fp16 model input written for the NEXT
 * UNet call is x' * next_input_scale (Euler: 1 / sqrt(sigma_next^2 + 1)); x itself stays unscaled in fp32. */
int lavie_cfg_sampler_step(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float guidance,
                           float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, void* stream);
int lavie_latents_to_scaled_model_input(const float* x, void* model_in2, long long n, float input_scale, void* stream);
/* The loop body without classifier-free guidance (`guidance_scale <= 1`: do_classifier_free_guidance is False,
 * pipeline_videogen.py:626, 666, 678): eps fp16 [n] is used as it is, model_in fp16 [n] is the single copy x' * scale. */
int lavie_sampler_step(const void* eps, float* x, const float* noise, void* model_in, long long n, float k_x, float k_eps,
                       float c_x0, float c_xt, float sigma, float next_input_scale, void* stream);
int lavie_latents_to_scaled_model_input1(const float* x, void* model_in, long long n, float input_scale, void* stream);
/* Guidance + multistep step (DPM-Solver++ 2M, lavie_amd/scheduling_dpmsolver_multistep.py), one launch per denoising step.
 * The five-coefficient form above cannot express a second-order multistep update: it needs the previous step's x0 prediction.
 * Per element, fp32, in this order:
 *   eps = eps_u + guidance (eps_c - eps_u)        (cfg variant only)
 *   x0  = k_x x - k_eps eps
 *   D   = c_prev != 0 ? x0 + c_prev (x0 - x0_prev) : x0
 *   x'  = c_xt x + c_x0 D;   x0_prev <- x0;  x <- x';  model_in <- fp16(x' next_input_scale)   ([x' | x'] for the cfg variant)
 * x0_prev: fp32 device buffer of the caller, n elements, updated in place.  With c_prev == 0 (first step, final step, order 1) it
 * is written and NEVER read: it may be uninitialised.  No noise operand (the solver is deterministic), no atomics: bit-reproducible.
 * No host synchronisation and no allocation: safe inside a stream capture.  Checked on the host before any HIP call: non-null
 * tensors, n >= 1, finite scalars, eps / x / x0_prev / model_in 16-byte aligned (the kernel uses 16-byte accesses; under guidance
 * with n % 8 != 0 the cond halves are not aligned and the launch takes a one-element-per-lane form, same arithmetic). */
int lavie_cfg_multistep_step(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, float guidance, float k_x,
                             float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale, void* stream);
int lavie_multistep_step(const void* eps, float* x, float* x0_prev, void* model_in, long long n, float k_x, float k_eps,
                         float c_x0, float c_xt, float c_prev, float next_input_scale, void* stream);

/* Sampling around known latents (additive in ABI 8): the four steps above with the known-region replacement of the legacy
 * inpaint / img2img loop inside the step kernel, still one launch per denoising step.  The caller pins part of the latents
 * [P, channels, inner] (inner = frames * height * width) with a mask; after the step the pinned part holds the known clean
 * latents at the noise level (a_next, s_next) of the timestep the step lands on, the rest keeps the step's own result.
 * Per element, fp32, contraction off, every fused multiply-add spelled out in the source:
 *   xm = the x' of the plain entry point of the same name, with that kernel's rounding points
 *   xk = s_next != 0 ? fma(s_next, noise_known, a_next known) : a_next known
 *   m  = mask[(i / (channels inner)) inner + i % inner]
 *   x' = m == 0 ? xm : m == 1 ? xk : fma(m, xk - xm, xm);   x <- x'
 *   model_in <- fp16(x' next_input_scale), rounded as the plain entry point rounds it (five-coefficient family: the exact
 *               product rounded once; multistep family: fp16 of the fp32 product), one value for both guidance halves
 *   multistep family: x0_prev <- m == 0 ? x0 : m == 1 ? known : fma(m, known - x0, x0); never read when c_prev == 0
 * So m == 0 everywhere gives the plain entry point's bits whatever known / noise_known hold, and m == 1 gives xk whatever
 * the model predicted: with a_next = 1, s_next = 0 (after the last step) that is `known` itself.  0 < m < 1 is a linear blend.
 * known / mask / noise_known are read-only and must not overlap x, x0_prev or model_in; the other aliasing rules are those
 * of the plain entry points.  No atomics, no host synchronisation, no allocation: bit-reproducible and safe in a capture.
 * Checked on the host before any HIP call, a refused call launches nothing and names the argument: region != NULL and its
 * struct_size; non-null eps / x / x0_prev / model_in / known / mask; noise_known != NULL unless s_next == 0; noise != NULL
 * unless sigma == 0; channels, inner >= 1 and n == P channels inner for a whole P >= 1; finite scalars; with inner % 8 == 0
 * (eight elements per lane, 16-byte accesses; otherwise one element per lane) every tensor read or written 16-byte aligned. */
typedef struct lavie_known_region {
    int struct_size;              /* sizeof this struct as the CALLER declared it; any other value is refused */
    int channels;                 /* C of the latents: the mask is broadcast over it */
    long long inner;              /* frames * height * width */
    const float* known;           /* [P, channels, inner] fp32, device */
    const float* mask;            /* [P, 1, inner] fp32 in [0, 1], device; NULL (= 1 everywhere) only for lavie_known_blend_f32 */
    const float* noise_known;     /* [P, channels, inner] fp32, device; may be NULL iff s_next == 0 */
    float a_next, s_next;         /* noise level the step lands on: x_t = a known + s noise */
} lavie_known_region;
int lavie_cfg_sampler_step_known(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float guidance,
                                 float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, void* stream,
                                 const lavie_known_region* region);
int lavie_sampler_step_known(const void* eps, float* x, const float* noise, void* model_in, long long n, float k_x, float k_eps,
                             float c_x0, float c_xt, float sigma, float next_input_scale, void* stream,
                             const lavie_known_region* region);
int lavie_cfg_multistep_step_known(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, float guidance,
                                   float k_x, float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale,
                                   void* stream, const lavie_known_region* region);
int lavie_multistep_step_known(const void* eps, float* x, float* x0_prev, void* model_in, long long n, float k_x, float k_eps,
                               float c_x0, float c_xt, float c_prev, float next_input_scale, void* stream,
                               const lavie_known_region* region);
/* The start of such a run, no eps operand: x <- m == 0 ? x : m == 1 ? xk : fma(m, xk - x, x) with xk as above at the noise
 * level of the FIRST timestep, and model_in <- fp16(x' input_scale) rounded once, as lavie_latents_to_scaled_model_input
 * does: n values, or [x' | x'] (2 n) with dup != 0.  With a mask it prepares x_T of a pinned run; with region->mask == NULL
 * (m = 1 everywhere) it is the scheduler's add_noise and starts a run at reduced strength.  Same checks as above. */
int lavie_known_blend_f32(float* x, void* model_in, int dup, long long n, float input_scale, void* stream,
                          const lavie_known_region* region);

/* Sampling a clip longer than the model's window as overlapping frame windows (additive in ABI 8; csrc/sampler_window.hip,
 * DESIGN.md 7.9): ONE fp32 latent tensor x [P, C, F, hw] holds the whole clip, the UNet ran on W windows of L frames each
 * (window w = frames [starts[w], starts[w] + L)), and this call fuses the windows' noise predictions where they overlap, advances
 * the whole clip by one scheduler step and writes every window's next fp16 model input, in one launch.
 * Per element (p, c, f, j), fp32, contraction off, over the windows that cover frame f in ascending window order:
 *   e_w = fma(guidance, ec_w - eu_w, eu_w)              (cfg == 0: e_w = eu_w)   from eps[w][half, c, f - starts[w], j]
 *   n_w = profile[f - starts[w]] / S                    S = the covering windows' profile values added in window order
 *   eps = fma(n_w, e_w, eps)                            starting from 0
 *   x', x0 = the plain step of the family from eps      family 0: lavie_cfg_sampler_step / lavie_sampler_step, aux = the step's noise
 *                                                       (read when c4 = sigma != 0); family 1: lavie_cfg_multistep_step /
 *                                                       lavie_multistep_step, aux = x0_prev (read when c4 = c_prev != 0, always written)
 *   model_in[w][half, c, f - starts[w], j] = fp16(x' next_input_scale) for every covering window and both guidance halves, rounded
 *                                            as the family's plain entry point rounds it
 * So a frame covered by one window has n_w = 1 and eps = e_w exactly: the bits of the plain entry point; all windows that share a
 * frame receive one fp16 value; both guidance halves of every model_in[w] are bit-equal.  No atomics, no host synchronisation,
 * no allocation: bit-reproducible and safe in a capture.
 * eps[w] / model_in[w]: fp16 device tensors [nb, C, L, hw], nb = 2 P with cfg ([negative | prompt]) else P.  starts_host,
 * profile_host, eps_host and model_in_host are HOST arrays (W, L, W, W entries), read before the call returns; they travel to the
 * kernel as launch arguments.
 * Checked on the host before anything is dereferenced or launched, each refusal names its argument: args != NULL and its
 * struct_size; family 0 / 1; P, C, F, hw >= 1 and P C F <= 65535; 1 <= W <= 32, 1 <= L <= 64; non-null host arrays; starts
 * strictly ascending with starts[0] >= 0 and starts[W-1] + L <= F; every frame covered by at least 1 and at most 4 windows; every
 * profile value finite and > 0; no null pointer in either table; x != NULL, aux != NULL unless family 0 with c4 == 0; no overlap
 * between x, aux, any model_in[w] and any other buffer of the call (two eps tensors may overlap: they are only read); finite
 * scalars; with hw %% 8 == 0 (eight elements per lane, 16-byte accesses; otherwise one element per lane) every tensor 16-byte
 * aligned. */
#define LAVIE_WINDOW_MAX_WINDOWS 32
#define LAVIE_WINDOW_MAX_LENGTH 64
#define LAVIE_WINDOW_MAX_COVER 4
typedef struct lavie_window_step_args {
    int struct_size;                  /* sizeof this struct as the CALLER declared it; any other value is refused */
    int family;                       /* 0 five-coefficient (aux = noise), 1 multistep (aux = x0_prev) */
    int cfg;                          /* != 0: classifier-free guidance, nb = 2 P */
    int P, C, F;                      /* videos, latent channels, frames of the WHOLE clip */
    long long hw;                     /* height * width of a latent frame */
    int W, L;                         /* windows, frames per window */
    const int* starts_host;           /* [W] first frame of each window */
    const float* profile_host;        /* [L] weight of a window's i-th frame */
    const void* const* eps_host;      /* [W] device pointers: the UNet's output for each window */
    void* const* model_in_host;       /* [W] device pointers: the next model input of each window */
    float* x;                         /* [P, C, F, hw] fp32, device, updated in place */
    float* aux;                       /* [P, C, F, hw] fp32, device: the step's noise (family 0) or x0_prev (family 1) */
    float guidance, k_x, k_eps, c_x0, c_xt, c4, next_input_scale;
} lavie_window_step_args;
int lavie_window_step(const lavie_window_step_args* args, void* stream);

/* Guidance from a per-latent table (additive in ABI 8; csrc/sampler_guidance.hip): a guidance scale of its own
 * for every latent of a batched call, and guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are
 * Flawed"; diffusers' rescale_noise_cfg) inside the fused step.  eps = [negative | prompt], fp16 [2 P, per]; for latent p:
 *   e_i   = fma(g_p, ec_i - eu_i, eu_i)                     fp32, the value the step kernels themselves form
 *   s_t   = std(ec), s_e = std(e) over the latent's per elements, unbiased (per - 1)
 *   f_p   = rescale s_t / s_e + (1 - rescale)               in double, stored as fp32
 *   eps_i = f_p e_i                                         one fp32 multiply, then the plain step of the family from eps
 * s_e == 0 gives f_p = 1 (diffusers gives NaN there); a NaN or infinity among a latent's predictions makes that latent's f_p NaN and
 * no other's.  lavie_guidance_table writes table[W][P] = (fp32 g_p, fp32 f_p) in two launches: per-chunk fp32 sums of ec, ec^2,
 * e, e^2 (a chunk = 2048 elements whatever P or the grid; partials[W P][chunks][4]), then one workgroup per latent that adds the
 * chunks in ascending order with a fixed tree in double.  rescale == 0 writes f_p = 1 in one launch and touches no partials.
 * g_p = guidance_dev[p] (P floats on the device) or, with guidance_dev == NULL, `guidance`.  moments != NULL also receives the
 * four double sums per latent.  W > 1: one eps tensor per frame window, each with statistics of its own.  No floating-point
 * atomics, fixed order of additions, no host synchronisation, no allocation: bit-reproducible and safe in a capture; partials,
 * table and moments are the caller's, lavie_guidance_partials_floats gives the partials' size (-1 for arguments out of range).
 * Checked on the host before anything is dereferenced or launched, each refusal names its argument: args != NULL and its
 * struct_size; 1 <= W <= 32, P >= 1, W P <= 65535; per >= 2; non-null eps_host and entries, 16-byte aligned when per %% 8 == 0
 * (16-byte loads; otherwise one element per lane, same arithmetic); finite guidance; rescale in [0, 1]; table != NULL; with
 * rescale != 0 partials != NULL, 16-byte aligned and partials_floats large enough. */
typedef struct lavie_guidance_table_args {
    int struct_size;                  /* sizeof this struct as the CALLER declared it; any other value is refused */
    int W, P;                         /* eps tensors (1 without windows), latents in each */
    long long per;                    /* elements of one latent */
    const void* const* eps_host;      /* [W] HOST array of device pointers, fp16 [2 P, per] each */
    const float* guidance_dev;        /* [P] fp32, device, or NULL: every latent takes `guidance` */
    float guidance, rescale;
    float* partials;                  /* device workspace, see above; may be NULL iff rescale == 0 */
    long long partials_floats;
    float* table;                     /* [W][P][2] fp32, device, written */
    double* moments;                  /* [W][P][4] fp64, device, written; may be NULL */
} lavie_guidance_table_args;
long long lavie_guidance_partials_floats(int latents, long long per);
int lavie_guidance_table(const lavie_guidance_table_args* args, void* stream);
/* The guided steps above with (g, f) = table[i / per] in place of the `guidance` argument and eps = f e; everything else, the
 * rounding points included, is the entry point of the same name without `_scaled`, so a table of (g, 1) gives that entry point's
 * bits in x, x0_prev and model_in.  table: fp32 [P][2] on the device ([W][P][2] for the windowed step, which then needs cfg != 0),
 * as lavie_guidance_table writes it.  Checked on the host like their plain forms, and: table != NULL; per >= 2 and n == P per for a
 * whole P in 1..65535 (the known-region forms take per = channels inner from the region); 16-byte alignment of every tensor when
 * per %% 8 == 0 (eight elements per lane; otherwise one). */
int lavie_cfg_sampler_step_scaled(const void* eps2, float* x, const float* noise, void* model_in2, long long n, const float* table,
                                  long long per, float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale,
                                  void* stream);
int lavie_cfg_multistep_step_scaled(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, const float* table,
                                    long long per, float k_x, float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale,
                                    void* stream);
int lavie_cfg_sampler_step_known_scaled(const void* eps2, float* x, const float* noise, void* model_in2, long long n, const float* table,
                                        float k_x, float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, void* stream,
                                        const lavie_known_region* region);
int lavie_cfg_multistep_step_known_scaled(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, const float* table,
                                          float k_x, float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale,
                                          void* stream, const lavie_known_region* region);
int lavie_window_step_scaled(const lavie_window_step_args* args, const float* table, void* stream);

/* UniPC (Zhao et al., arXiv:2302.04867; lavie_amd/scheduling_unipc_multistep.py; csrc/sampler_unipc.hip), additive in
 * ABI 8: one launch per denoising step runs guidance, the x0 prediction, the corrector that recomputes the sample the model was
 * just evaluated at, the predictor to the next timestep, the history writes and the next fp16 model input.  The corrector reuses
 * the model output the predictor needs anyway, so it costs no UNet forward.  Per element, fp32, contraction off, in this order:
 *   eps = eps_u + guidance (eps_c - eps_u)          (cfg entries; _scaled: (g, f) = table[i / per] and eps = f eps, as above)
 *   m   = k_x x - k_eps eps                         one fma on the rounded product k_x x
 *   xc  = corr != 0 ? c_l x_last + c_0 m + c_1 m1 + c_2 m2 : x        the rounded product c_l x_last, then one fma per term in
 *                                                                     this order; a term whose coefficient is 0 is skipped
 *   x'  = p_x xc + p_0 m + p_1 m1                   the sum of the two rounded products, then one fma for p_1 m1 unless p_1 == 0
 *   x_last <- xc;  m2 <- m1;  m1 <- m;  x <- x';  model_in <- fp16(fp32(x' next_input_scale))    ([x' | x'] for the cfg entries)
 * x_last (the previous corrected sample), m1, m2 (the two previous x0 predictions): fp32 device buffers of the caller, n elements
 * each, updated in place.  A buffer is read only when a coefficient that multiplies it is in force and non-zero (x_last: corr and
 * c_l; m1: corr and c_1, or p_1; m2: corr and c_2); otherwise it is written and NEVER read, so all three may be uninitialised at
 * the first step (corr = 0, p_1 = 0).  When m1 is not read, m2 receives m (no later step can need that value).
 * With corr = 0 and p_1 = 0, x and model_in have the bits of lavie_multistep_step(k_x, k_eps, c_x0 = p_0, c_xt = p_x, c_prev = 0).
 * No noise operand, no atomics, no host synchronisation, no allocation: bit-reproducible and safe inside a stream capture.
 * Checked on the host before any HIP call, a refused call launches nothing and names its argument: coeffs.struct_size; non-null
 * eps / x / x_last / m1 / m2 / model_in (and table); n >= 1; finite scalars; x, x_last, m1, m2 pairwise disjoint; _scaled: per >=
 * 2 and n == P per for a whole P in 1..65535; with n % 8 == 0 (_scaled: per % 8 == 0; eight elements per lane, 16-byte accesses;
 * otherwise one element per lane, same arithmetic) every tensor 16-byte aligned. */
typedef struct lavie_unipc_coeffs {
    int struct_size;                  /* sizeof this struct as the CALLER declared it; any other value is refused */
    int corr;                         /* != 0: the corrector runs (every step but a run's first) */
    float guidance;                   /* lavie_cfg_unipc_step only; finite everywhere */
    float k_x, k_eps;
    float c_l, c_0, c_1, c_2;         /* corrector: x_last, m, m1, m2 */
    float p_x, p_0, p_1;              /* predictor: xc, m, m1 */
    float next_input_scale;
} lavie_unipc_coeffs;
int lavie_unipc_step(const void* eps, float* x, float* x_last, float* m1, float* m2, void* model_in, long long n,
                     lavie_unipc_coeffs coeffs, void* stream);
int lavie_cfg_unipc_step(const void* eps2, float* x, float* x_last, float* m1, float* m2, void* model_in2, long long n,
                         lavie_unipc_coeffs coeffs, void* stream);
int lavie_cfg_unipc_step_scaled(const void* eps2, float* x, float* x_last, float* m1, float* m2, void* model_in2, long long n,
                                const float* table, long long per, lavie_unipc_coeffs coeffs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Perturbed-attention guidance (PAG: Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance"; diffusers'
 * AnimateDiffPAGPipeline) inside the fused step (sampler_pag.hip; additive in ABI 8).  The four steps carry the arguments of their
 * plain namesakes plus `pag_scale`, and eps / model_in hold one part more, the perturbed prediction last: fp16 [3, n] = [negative |
 * prompt | perturbed] for the cfg_ entries, [2, n] = [prompt | perturbed] for the others (the output of ONE forward whose trailing
 * batch entries ran under lavie_unet_set_pag).  Per element, fp32, every fused multiply-add spelled out:
 *   e   = cfg ? fma(guidance, ec - eu, eu) : ec
 *   eps = pag_scale != 0 ? fma(pag_scale, ec - ep, e) : e        (pag_scale == 0: the perturbed part is not read)
 *   then the family's plain step unchanged: x <- x' in place (multistep: x0_prev <- x0), and the family's rounding of
 *   x' * next_input_scale as ONE fp16 value written to all three (two) parts of model_in.
 * pag_scale == 0 gives the bits of the plain namesake; ep == ec gives its values.  Eight elements per lane with 16-byte accesses
 * when n % 8 == 0 (eps, x, the noise that is read / x0_prev, model_in must then be 16-byte aligned: every part is), else one element
 * per lane with the same arithmetic.  No atomics, no host synchronisation, no allocation: safe inside a stream capture.
 * Refused with a message naming the argument, nothing launched: a null tensor, n < 1, a non-finite scalar, pag_scale < 0, a
 * misaligned tensor in the eight-element form.
 * PAG is not combined with the known-region (_known), frame-window (lavie_window_step) or table (_scaled) forms. */
int lavie_cfg_pag_sampler_step(const void* eps3, float* x, const float* noise, void* model_in3, long long n, float guidance, float k_x,
                               float k_eps, float c_x0, float c_xt, float sigma, float next_input_scale, float pag_scale, void* stream);
int lavie_pag_sampler_step(const void* eps2, float* x, const float* noise, void* model_in2, long long n, float k_x, float k_eps, float c_x0,
                           float c_xt, float sigma, float next_input_scale, float pag_scale, void* stream);
int lavie_cfg_pag_multistep_step(const void* eps3, float* x, float* x0_prev, void* model_in3, long long n, float guidance, float k_x,
                                 float k_eps, float c_x0, float c_xt, float c_prev, float next_input_scale, float pag_scale,
                                 void* stream);
int lavie_pag_multistep_step(const void* eps2, float* x, float* x0_prev, void* model_in2, long long n, float k_x, float k_eps, float c_x0,
                             float c_xt, float c_prev, float next_input_scale, float pag_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hook: HIP-event timing per kernel class on the launch stream (bench.py's roofline leg).
 * Classes: 0 conv3x3 (implicit GEMM, gathered), 1 linear/1x1/GEGLU GEMM, 2 spatial+text attention core,
 * 3 temporal attention core, 4 GroupNorm, 5 LayerNorm, 6 other, 7 the halo-patch conv kernel alone (a subset of
 * class 0: the events bracket exactly that kernel's launches), 8 the fused temporal sub-block kernel, 9 the fused feed-forward
 * kernel (both with events attached to the kernel launch itself).  lavie_profile_end synchronises the
 * stream and fills four host arrays of LAVIE_PROFILE_CLASSES entries (launches, milliseconds,
 * algorithmic flops, algorithmic bytes — the per-launch figures are defined in DESIGN.md).
 * ---------------------------------------------------------------------------------------------- */
#define LAVIE_PROFILE_CLASSES 11
/* Which optional engine paths lavie_unet_forward takes (A/B timing, parity cross-checks).  Bits: 0 = fused feed-forward kernel
 * (lavie_geglu_mlp_f16), 1 = fused temporal-attention sub-block (lavie_temporal_block_f16), 2 = fused text cross-attention
 * sub-block (lavie_cross_block_f16), 4 = parity form of the Upsample3D convs (lavie_upsample_conv3x3_f16), 5 = GroupNorm statistics
 * taken from the producing kernel's epilogue instead of a statistics pass (round 4).  Bit 6 (debug, off): every GroupNorm that takes
 * producer statistics ALSO runs the statistics pass and compares the two on the host.  Bit 8: the fused block head
 * (lavie_proj_qkv_f16: GroupNorm -> proj_in -> norm1 -> q|k|v in one kernel).  Default 0x137 (bits 0, 1, 2, 4, 5, 8); 0 = the
 * one-GEMM-per-launch path of round 2.  Any other bit (3, 7, 9 and up) is an error and leaves the mask unchanged. */
int lavie_debug_fused_mask(int mask);
/* Test hook: GroupNorm launches so far (process-wide) that took their statistics from the producers' epilogues.  Bit 6 of the mask
 * above makes every such launch ALSO run the statistics pass and compare the two on the host (synchronises; an error names the
 * first (batch, group) that differs). */
long long lavie_debug_gn_producer_count(void);
/* Producer-side norm statistics at operator level (additive, ABI unchanged; test hooks).  The kernels that store a tensor can leave
 * sums and sums of squares of the rounded fp16 values they stored: per (row block, channel) for a consuming GroupNorm ("column
 * statistics": per block and channel quad four sums, then four sums of squares), per (row, 16 NT-column wave tile) for a consuming
 * LayerNorm ("row statistics": [M][slots][2]).  In a forward the engine asks for them; the sink below asks for them on behalf of the
 * operator-level GEMM entry points (lavie_linear_f16, lavie_linear_lnfold_f16, lavie_conv3x3_f16, lavie_conv3x3_down_f16,
 * lavie_upsample_conv3x3_f16, lavie_temporal_conv_f16).
 *   colstat / rowstat: device buffers of colstat_floats / rowstat_floats floats; null or 0 disarms that kind.  While armed, every such
 *   launch whose plan writes column statistics writes them to `colstat` (a GEGLU epilogue writes none), and a plain EPI_LINEAR
 *   launch without a LayerNorm fold writes row statistics to `rowstat` (and is therefore planned unsplit, as in the engine).  A
 *   buffer too small for what the planned launch stores is refused before the launch; the message names the float count.
 * lavie_debug_op_statistics_plan(colstat, rowstat): while either is non-zero, the same entry points plan as if that kind were armed,
 *   record the plan for the query and launch NOTHING (their outputs stay untouched): how a caller sizes the sink's buffers.
 * lavie_debug_op_statistics_last: the plan of the last such launch.  colstat_rows / colstat_span / nsets / set_blocks are what the
 *   engine hands a consuming GroupNorm; colstat_blocks_stored >= nsets * set_blocks counts the tile padding the 128-row and
 *   ping-pong kernels store too (a block whose rows all lie past M holds zeros); colstat_floats = colstat_blocks_stored * 2 N. */
typedef struct lavie_op_statistics_info {
    int struct_size;                  /* sizeof this struct as the CALLER declared it; any other value is refused */
    int M, N, splits;                 /* of the launch */
    int colstat_written;              /* 0 / 1 */
    int colstat_rows, colstat_span, nsets, set_blocks;
    int colstat_contiguous;           /* 1: block b of a set holds the set's rows [b colstat_rows, (b + 1) colstat_rows) in ascending order (the
                                         128-row, ping-pong and persistent kernels, the split-K reduce, the halo-patch kernel's whole-row tiles and
                                         its parity form, whose set j = the outputs of parity j); 0: only the span holds (2-D and temporal tiles) */
    int rowstat_written;              /* 0 / 1 */
    int rowstat_cols, rowstat_slots;  /* columns per slot; slots per row = N / rowstat_cols */
    long long colstat_blocks_stored, colstat_floats, rowstat_floats;
} lavie_op_statistics_info;
int lavie_debug_op_statistics(float* colstat, long long colstat_floats, float* rowstat, long long rowstat_floats);
int lavie_debug_op_statistics_plan(int colstat, int rowstat);
int lavie_debug_op_statistics_last(lavie_op_statistics_info* out);
/* lavie_group_norm_f16 with the producers' column statistics of x1 / x2 (either may be null: none).  When every given descriptor can
 * serve the GroupNorm (C equal to the tensor's, C % 4 == 0, P a whole number of spans and of rows * nsets), one fold of the partials
 * replaces the statistics pass and lavie_debug_gn_producer_count() grows by one; otherwise the two-pass path runs.  A descriptor
 * whose partials_floats cannot hold nsets * set_blocks blocks, or whose set_blocks is fewer than the NB domains need, is refused. */
typedef struct lavie_gn_producer_stats {
    int struct_size;                  /* sizeof this struct as the CALLER declared it; any other value is refused */
    int C;                            /* channels of the tensor */
    const float* partials;            /* device: [nsets][set_blocks][C / 4][2][4] */
    long long partials_floats;
    int rows, nsets, set_blocks, span;
} lavie_gn_producer_stats;
int lavie_group_norm_stats_f16(const void* x1, int C1, const void* x2, int C2, int NB, int P, int groups, const float* gamma,
                               const float* beta, float eps, int silu, float* stats_ws, void* y, const lavie_gn_producer_stats* cs1,
                               const lavie_gn_producer_stats* cs2, void* stream);
/* Row statistics -> (mean, rstd): partials [M][slots][2] (sum, sum of squares over row_len values per row) -> out [M][2], the
 * ln_stats operand of lavie_linear_lnfold_f16.  Fixed summation order. */
int lavie_rowstat_finalize_f32(const float* partials, int slots, int M, int row_len, float eps, float* out, void* stream);
/* Test/tuning knob for the implicit-GEMM kernel choice: 0 automatic, 1 128-row kernel with the widest tile,
 * 3 160x320 ping-pong kernel wherever N % 320 == 0, 4 automatic without the ping-pong
 * kernel, 5 halo-patch conv kernel wherever the conv is eligible, 6 automatic without the halo-patch kernel,
 * 7 persistent ping-pong kernel for every eligible plain GEMM, 8 automatic without it, 9 automatic without the GEGLU GEMMs on it.
 * Any other value is an error and leaves the mode unchanged. */
int lavie_debug_force_tile(int mode);
/* Test/tuning knob: force the split-K factor of the implicit GEMM (0 = automatic). */
int lavie_debug_force_splits(int s);
/* Tuning knob: LDS bytes one temporal-attention workgroup may stage (smaller = more workgroups per CU). */
int lavie_debug_temporal_budget(int bytes);
/* Test hook (additive, ABI unchanged): the most workgroups the launchers of the row-resident kernels start — lavie_geglu_mlp_f16,
 * lavie_temporal_block_f16, lavie_cross_block_f16 / lavie_cross_block_long_f16 and lavie_proj_qkv_f16, and nothing else.  0 =
 * automatic: min(tiles, 256).  1..256 = min(tiles, max_workgroups): the kernels deal their 16-row tiles to gridDim.x workgroups in
 * near-equal runs, 8 per pass, so a small cap walks a small input through second and later passes, which 256 workgroups reach only
 * past 2048 tiles (32784 rows).  Results do not depend on it.  Any other value is an error and leaves the setting unchanged. */
int lavie_debug_rowfuse_grid(int max_workgroups);
int lavie_profile_begin(unsigned mask, int max_events);
int lavie_profile_end(void* stream, long long* launches_host, double* ms_host, double* flops_host, double* bytes_host);

/* ------------------------------------------------------------------------------------------------
 * Whole denoiser: UNet3DConditionModel.forward (unet.py:366-512)
 * ---------------------------------------------------------------------------------------------- */
typedef struct lavie_unet_s* lavie_unet_t;

typedef struct lavie_unet_config {
    /* sizeof(lavie_unet_config) as the CALLER compiled / declared it.  lavie_unet_create rejects any other value, so a
     * binding written against an older (shorter) layout fails with a message instead of being read past its end. */
    int struct_size;
    int in_channels, out_channels;
    int num_levels;
    int block_out_channels[LAVIE_MAX_LEVELS];
    int attn_levels[LAVIE_MAX_LEVELS];      /* 1: CrossAttn{Down,Up}Block3D, 0: {Down,Up}Block3D */
    int layers_per_block;
    int heads;
    int cross_attention_dim;
    int norm_groups;
    float norm_eps;
    int rotary_dim;
    int rel_buckets, rel_max_distance;
    /* Block variant of the frame-interpolation model (interpolation/models/attention.py:456-606; all 0 = base model):
     *   sparse_causal_attn1 : attn1 is SparseCausalAttention (use_first_frame, :493-504, 609-665)
     *   temporal_plain      : attn_temp is the plain CrossAttention over frames — no rotary embedding, no
     *                         relative-position bias, and no such tensors in the state dict (:525-533)
     *   ff_before_temporal  : block order spatial -> text -> feed-forward -> temporal (:566-606) */
    int sparse_causal_attn1, temporal_plain, ff_before_temporal;
    /* Block variant of the VSR stage's UNet3DVSRModel (vsr/models/attention.py:314-594; 0 = base model):
     *   vsr_blocks              : Transformer3DModel starts with a ResnetBlock3DCNN (3,1,1) without time embedding
     *                             (`resblock_temporal`, :350, 395-398), the temporal attention tensors are named
     *                             attn_temporal / norm_temporal, proj_in / proj_out are nn.Linear (:353, 383)
     *   only_cross_attention[l] : attn1 of level l attends to the text context instead of the frame (:465-490, 558-561) */
    int vsr_blocks;
    int only_cross_attention[LAVIE_MAX_LEVELS];
    /* UNet3DVSRModel (vsr/models/unet.py:100-600):
     *   vsr_temporal_modules : a TemporalModule3D (ResnetBlock3DCNN (5,1,1) -> ResnetBlock3D -> zero-initialised 1x1 shift
     *                          conv, residual; temporal_module.py:65-178) after every down block, the mid block and every
     *                          up block (down_temporal_idx / mid_temporal / up_temporal_idx = all levels)
     *   num_class_embeds     : > 0: emb = time_embedding + class_embedding[noise level] (:176-177, 494-505); the forward
     *                          entry is then lavie_unet_forward_labels */
    int vsr_temporal_modules;
    int num_class_embeds;
} lavie_unet_config;

/* sizeof(lavie_unet_config) in this build of the library: what cfg->struct_size must hold. */
int lavie_unet_config_size(void);
int lavie_unet_create(const lavie_unet_config* cfg, lavie_unet_t* out);
int lavie_unet_destroy(lavie_unet_t h);
/* Number of state-dict entries the model expects and the i-th name/numel (reference key names,
 * unet.py:142-295): lets a binder enumerate the checkpoint contract without Python. */
int lavie_unet_num_params(lavie_unet_t h);
int lavie_unet_param_info(lavie_unet_t h, int i, const char** name, long long* numel);
/* Hand over one fp16 state-dict tensor (borrowed until lavie_unet_finalize returns and the stream drains). */
int lavie_unet_set_param(lavie_unet_t h, const char* name, const void* data_f16, long long numel);
/* Repack all weights into the engine's own arena (fused QKV, [Cout][tap][Cin] convs, GEGLU order, fp32 biases). */
int lavie_unet_finalize(lavie_unet_t h, void* stream);
/* Size the activation workspace for inputs up to [B, *, F, H, W] (allocates; not stream-ordered). */
int lavie_unet_prepare(lavie_unet_t h, int B, int F, int H, int W, int ctx_len);
/* Optional: the text keys / values of every transformer block (attention.py:177-178 on encoder_hidden_states, which the
 * reference recomputes in every block of every denoising step, and once per frame: :364) computed ONCE for the context
 * tensor `ctx` [B, ctx_len, cross_attention_dim] and kept in the handle.  Forwards called afterwards with the same `ctx`
 * pointer, B and ctx_len read them instead of recomputing them; any other context is computed as usual.  The caller
 * promises not to change the tensor's contents while it is cached; ctx = NULL drops the cache.  Needs lavie_unet_prepare. */
int lavie_unet_cache_context(lavie_unet_t h, const void* ctx, int B, int ctx_len, void* stream);
/* A/B switch (default on): fold every LayerNorm of the transformer blocks into the epilogues of the GEMM that
 * produces its input (row statistics) and the GEMM that consumes its output (gamma folded into the weights). */
int lavie_unet_set_ln_fold(lavie_unet_t h, int on);
/* FreeU inside the forward (diffusers' enable_freeu(s1, s2, b1, b2), same argument order; additive in ABI 8): in up block i in {0, 1},
 * in front of EVERY resnet of the block, the running activation and the popped skip go through lavie_freeu_f16 with (b_{i+1}, s_{i+1}),
 * in place; the resnet (norm1 and the shortcut included) sees the modified pair.  A stage with b == 1 and s == 1 launches nothing, so
 * (1, 1, 1, 1), the default, is the plain forward, bit for bit.  Every value must be finite and > 0: otherwise an error and no change.
 * Holds for every forward that follows, eager or captured (a change re-captures); it needs no new workspace after lavie_unet_prepare. */
int lavie_unet_set_freeu(lavie_unet_t h, float s1, float s2, float b1, float b2);
/* Perturbed-attention guidance inside the forward (additive in ABI 8; the handle must be finalized).  `layers_host`: n_layers
 * prefixes of transformer names as the state dict spells them ("mid_block", "down_blocks.2", "up_blocks.1.attentions.0", ...): a
 * transformer is selected when its prefix (mid_block.attentions.0, ...) starts with an entry followed by '.' or the end of the name.
 * `perturbed`: the number of TRAILING batch entries whose attn1 is perturbed in the selected blocks, in every forward that follows:
 * there attn1(x) = to_out(to_v(norm1(x))), the identity map on values, no softmax (the q|k|v projection runs on all rows, the
 * attention kernel on the leading (B - perturbed) F frames, the perturbed rows receive the V columns through a strided row copy;
 * to_out and everything behind it are unchanged).  n_layers == 0 or perturbed == 0 switches it off (the default): off is the plain
 * forward, launch for launch and bit for bit.  Refused with a message naming the argument, nothing changed: an entry that selects no
 * transformer; a selected transformer whose attn1 is not the plain spatial self-attention (the interpolation model's sparse-causal
 * blocks, the VSR model's only_cross_attention levels); perturbed < 0.  A forward (or lavie_unet_transformer_forward) with
 * B <= perturbed is refused.  While it is on, lavie_unet_set_cfg_shared_input(1) is ignored (plain forward: this is where the shared
 * input does not apply; letting the perturbed entries share the down path with their prompt twins is not implemented).  Holds on
 * every kernel route, eager or captured (a change re-captures); it needs no new workspace after lavie_unet_prepare.  With B <= 8 a
 * forward serves at most 2 prompts as [negative | prompt | perturbed], 4 as [prompt | perturbed]. */
int lavie_unet_set_pag(lavie_unet_t h, const char* const* layers_host, int n_layers, int perturbed);
/* Classifier-free guidance (pipeline_videogen.py:666: `torch.cat([latents] * 2)`) runs the UNet on the SAME latents twice with
 * different text.  on = 1: the caller vouches that sample[b] == sample[b + B/2] for every b < B/2 (B even) in the forwards that
 * follow; the layers in front of the first text cross-attention (conv_in, down_blocks.0.resnets.0, and the GroupNorm / proj_in /
 * self-attention of down_blocks.0.attentions.0: unet.py:437-452, attention.py:369-373, 513-522) are then computed for the first
 * half of the batch only and copied.  Outputs equal the plain forward's to rounding (a half-batch launch may pick another tile).
 * Base UNet configuration only; ignored (plain forward) where it does not apply.  Default off. */
int lavie_unet_set_cfg_shared_input(lavie_unet_t h, int on);
/* Low-rank adapters (LoRA) on the attention projections: the to_q / to_k / to_v / to_out.0 weight of attn1, attn2 and attn_temp
 * (attn_temporal in the VSR model) of every transformer block — the target_modules of the fork's LoraConfig
 * (base/pipelines/fine_tuning.py:296-307).  Served merged: W = W0 + global_scale * scale * B A (lavie_lora_merge_f16), written into
 * the packed weights and every image derived from them (fused q|k|v, LayerNorm folds, the row-resident kernels' images and a cached
 * context's text K / V) IN PLACE, so device addresses never change and a captured forward graph stays valid.
 * All four need a finalized handle; every argument is checked before any HIP call.
 *   lora_set: registers (or replaces) the adapter of one target.  `name` is the state-dict key of the weight; base_f16 [N, K] is the
 *     base weight (copied now: the handle never reads it again), A fp32 [r, K], B fp32 [N, r] (copied now), 1 <= r <= 128,
 *     `scale` (finite) the per-target factor, peft's lora_alpha / r.  Stream-ordered on `stream`; takes effect at the next apply.
 *   lora_clear: drops the adapter of `name`, or of every target for name = NULL; the next apply restores the base weights.
 *     Synchronises `stream` before freeing the adapter's buffers.
 *   lora_set_scale: the global factor (diffusers' cross_attention_kwargs={"scale": s}), default 1; 0 gives the base weights exactly.
 *   lora_apply: merges every target of the blocks touched since the last apply, re-derives those blocks and, if a context is cached
 *     (lavie_unet_cache_context), recomputes its K / V from the same ctx tensor.  Nothing to do = no launch.
 * Several adapters at once: the registry has LAVIE_LORA_MAX_TERMS slots, each holding one adapter (its targets' A / B / r / scale)
 * and one blend weight (default 1).  A target is served as
 *     W = W0 + sum over slots (global_scale * weight_slot * scale_slot,target) * B A
 * over the slots that hold an entry for the target, in ascending slot order, in ONE pass (lavie_lora_merge_multi_f16: fp32 sum, one
 * rounding).  The factor of a term is computed in fp32, left to right, as (global_scale * weight) * scale; a slot whose factor is 0
 * is not a term; with no terms the base copy goes back.  So the served weights depend on the registry's state only, never on the
 * order of the calls that led to it.  lora_set / lora_clear above act on slot 0; the global scale multiplies every slot.
 *   lora_set_slot / lora_clear_slot: lora_set / lora_clear for one slot, 0 <= slot < LAVIE_LORA_MAX_TERMS.  A target keeps one base
 *     copy for all of its slots; it goes away, after the next apply has written the base back, when its last slot is cleared.
 *   lora_set_slot_weight: the slot's blend weight (finite); 0 switches the adapter off and keeps it resident.  Marks the blocks in
 *     which the slot has an entry; takes effect at the next apply. */
int lavie_unet_lora_set(lavie_unet_t h, const char* name, const void* base_f16, const float* A, const float* B, int r, float scale,
                        void* stream);
int lavie_unet_lora_clear(lavie_unet_t h, const char* name, void* stream);
int lavie_unet_lora_set_scale(lavie_unet_t h, float scale);
int lavie_unet_lora_apply(lavie_unet_t h, void* stream);
int lavie_unet_lora_set_slot(lavie_unet_t h, int slot, const char* name, const void* base_f16, const float* A, const float* B, int r,
                             float scale, void* stream);
int lavie_unet_lora_clear_slot(lavie_unet_t h, int slot, const char* name, void* stream);
int lavie_unet_lora_set_slot_weight(lavie_unet_t h, int slot, float weight);
long long lavie_unet_weight_bytes(lavie_unet_t h);
long long lavie_unet_workspace_bytes(lavie_unet_t h);
/* sample [B, Cin, F, H, W] fp16 (NCFHW, as the reference passes it), timesteps [B] fp32,
 * ctx [B, ctx_len, cross_attention_dim] fp16  ->  out [B, Cout, F, H, W] fp16. */
int lavie_unet_forward(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx, void* out, int B,
                       int F, int H, int W, int ctx_len, void* stream);
/* The same forward replayed from a hipGraph (the reference has no counterpart: it is the launch path of unet.py:366-512).
 * First call with a new (pointers, shape, stream) tuple: eager.  Second: the enqueue of one forward is captured on `stream`,
 * instantiated and launched.  Later calls with the same tuple: hipGraphLaunch.  Tensor contents may change between calls,
 * addresses may not (a changed address simply starts over).  Runs eagerly while lavie_profile_begin is active. */
int lavie_unet_forward_graph(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx, void* out, int B,
                             int F, int H, int W, int ctx_len, void* stream);

/* Same for a model with num_class_embeds > 0: class_labels_host[B] (host ints, the VSR noise level per video). */
int lavie_unet_forward_labels(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx,
                              const int* class_labels_host, void* out, int B, int F, int H, int W, int ctx_len, void* stream);

/* Layer cache (feature caching as in DeepCache, Ma et al., CVPR 2024; additive in ABI 8).  The hidden state that enters the last,
 * full-resolution layers of the decoder changes slowly from one denoising step to the next, so a sampler may run the whole network
 * only every N-th step.  For a depth d in 1..layers_per_block the forward's list of steps has two cuts: A behind layer d - 1 of down
 * level 0 (its resnet, its transformer, the push of its skip) and B in front of layer layers_per_block - d of the last up block
 * (behind the upsampler into level 0 and, in the VSR model, the temporal module that follows it).  The cache holds the running
 * activation at B, rows(0) x C fp16 (C = block_out_channels[0]; [1] for d = layers_per_block) and its GroupNorm column statistics,
 * in one allocation outside the workspace that lavie_unet_prepare sizes for its shape.
 *   set_layer_cache: depth 0 switches it off and frees the allocation, 1..layers_per_block selects the cuts.  Refused for a model
 *     with fewer than three levels.  Every call marks a held cache invalid, and so does lavie_unet_prepare with another shape.
 *   layer_cache_bytes: the size of the allocation now (0: off, or no prepare yet); -1 for a null handle.
 *   forward_cached: lavie_unet_forward / _labels (class_labels_host NULL for a model without class embedding) with a mode:
 *     LAVIE_LAYER_CACHE_OFF      the plain forward, launch for launch; the cache is neither read nor written.
 *     LAVIE_LAYER_CACHE_REFRESH  the full walk, launch for launch and bit for bit the plain forward, except that the producer of the
 *                                tensor at B stores it into the cache; records (B, F, H, W, ctx_len, depth).
 *     LAVIE_LAYER_CACHE_REUSE    the shallow walk: the time embedding, conv_in, d down layers, the cached tensor, d + 1 up layers (with
 *                                the d + 1 skips of this call, in the order the full walk pops them), the trailing VSR temporal module,
 *                                conv_norm_out and conv_out.  Refused, nothing launched: depth 0, no valid cache, a recorded tuple
 *                                that differs from this call's, a capturing stream (a refresh is refused there too).
 *   The shared CFG prefix lies in front of A and works in every mode; FreeU and perturbed-attention guidance act in layers a reuse call
 *   does not run.  Weights, adapters, the context's contents, FreeU or PAG changed between a refresh and a reuse are the caller's
 *   business: the cached tensor is whatever the refresh computed.  Refresh and reuse calls of one handle belong on one stream.
 *   lavie_unet_forward_graph has no cached form. */
#define LAVIE_LAYER_CACHE_OFF 0
#define LAVIE_LAYER_CACHE_REFRESH 1
#define LAVIE_LAYER_CACHE_REUSE 2
int lavie_unet_set_layer_cache(lavie_unet_t h, int depth);
long long lavie_unet_layer_cache_bytes(lavie_unet_t h);
int lavie_unet_forward_cached(lavie_unet_t h, const void* sample, const float* timesteps, const void* ctx,
                              const int* class_labels_host /* NULL for models without class embedding */, void* out, int B, int F,
                              int H, int W, int ctx_len, int mode, void* stream);

/* Finer engine seams for parity tests (same packed weights as the whole model):
 * ResnetBlock3D.forward (resnet.py:177-207) and Transformer3DModel.forward (attention.py:358-407)
 * of the block whose state-dict prefix is `prefix` (e.g. "down_blocks.0.resnets.0").
 * x1/x2/y channels-last; temb [B, time_embed_dim] fp32 (the output of time_embedding, pre-SiLU). */
int lavie_unet_resnet_forward(lavie_unet_t h, const char* prefix, const void* x1, int C1, const void* x2, int C2,
                              const float* temb, void* y, int B, int F, int H, int W, void* stream);
int lavie_unet_transformer_forward(lavie_unet_t h, const char* prefix, void* x_inout, const void* ctx, int B, int F, int H,
                                   int W, int ctx_len, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Text encoder: transformers' CLIPTextModel (additive in ABI 8)
 * ---------------------------------------------------------------------------------------------- */
/* Causal self-attention over packed rows: qkv [NB L, ld] holds q | k | v of a token side by side (each heads * dh wide, head h at
 * columns h dh of its part); row b L + i attends to rows b L + j, j <= i:  o [NB L, ldo] = softmax_j(scale q_i k_j) v_j.
 * (CLIPAttention under the causal mask of CLIPTextTransformer.)  1 <= L <= 128, dh 32 or 64, NB >= 1, ld >= 3 heads dh, ldo >=
 * heads dh, both multiples of 8, both tensors 16-byte aligned: anything else is refused with a message naming the argument and
 * nothing is launched.  Fixed summation order, no atomics; a batch entry has the bits of its single-entry call. */
int lavie_causal_attention_f16(const void* qkv, int ld, void* o, int ldo, int NB, int L, int heads, int dh, float scale, void* stream);
/* out [B L, C] = fp16(float(tok_table[ids[r]]) + float(pos_table[r % L])), one rounding (CLIPTextEmbeddings).  ids_dev int32 [B L];
 * tok_table fp16 [V, C]; pos_table fp16 [P, C] with P >= L, which the caller vouches for; C % 8 == 0; tables and out 16-byte
 * aligned.  The kernel clamps an id into [0, V): no id reads outside the table.  A caller that holds the ids on the host should
 * validate them there (the Python wrapper raises). */
int lavie_token_embed_f16(const int* ids_dev, const void* tok_table, const void* pos_table, void* out, int B, int L, int C, int V,
                          void* stream);
/* x[0, n) <- act(x) in place, computed in fp32 with one rounding.  kind 0: x sigmoid(1.702 x) (CLIP's quick_gelu); kind 1: erf-GELU. */
#define LAVIE_TEXT_ACT_QUICK_GELU 0
#define LAVIE_TEXT_ACT_GELU 1
int lavie_act_f16(void* x, long long n, int kind, void* stream);

typedef struct lavie_text_s* lavie_text_t;
typedef struct lavie_text_config {
    int struct_size;       /* sizeof(lavie_text_config) as the caller declared it; any other value is refused (as lavie_unet_create) */
    int vocab_size;
    int hidden;            /* a multiple of 128, <= 2048 */
    int intermediate;      /* a multiple of 128 */
    int layers;
    int heads;             /* hidden / heads must be 32 or 64 */
    int max_positions;     /* rows of the position table, <= 128 */
    int act;               /* LAVIE_TEXT_ACT_* */
    float eps;             /* layer_norm_eps */
} lavie_text_config;
int lavie_text_config_size(void);
int lavie_text_create(const lavie_text_config* cfg, lavie_text_t* out);
int lavie_text_destroy(lavie_text_t h);
/* The state-dict contract: names are the keys of transformers' CLIPTextModel.state_dict()
 * (text_model.embeddings.token_embedding.weight, text_model.encoder.layers.0.self_attn.q_proj.weight, ...). */
int lavie_text_num_params(lavie_text_t h);
int lavie_text_param_info(lavie_text_t h, int i, const char** name, long long* numel);
/* One fp16 tensor, borrowed until lavie_text_finalize returns and the stream drains. */
int lavie_text_set_param(lavie_text_t h, const char* name, const void* data_f16, long long numel);
/* Copies the weights into the handle's own allocation (q | k | v fused, biases and norm vectors fp32) and allocates the workspace of
 * the largest call (B = 16, L = max_positions).  Allocates; not stream-ordered. */
int lavie_text_finalize(lavie_text_t h, void* stream);
/* Bytes of the handle's workspace that lavie_text_encode(h, ., B, L, ...) uses; -1 for a shape it refuses. */
long long lavie_text_workspace_bytes(lavie_text_t h, int B, int L);
/* ids_dev int32 [B, L] -> out_f16 [B, L, hidden] = last_hidden_state (the final LayerNorm applied).  1 <= B <= 16, 1 <= L <=
 * max_positions.  Enqueues 2 + 8 layers launches on `stream`; no allocation, no synchronisation (capturable).  Two calls on the
 * same ids agree bit for bit; the [L, hidden] block of a prompt has the same bits at every B and every position in the batch (the
 * GEMMs run one fixed tile geometry without split-K whatever B is); rows <= i do not depend on the ids behind position i.  Ids are
 * clamped into [0, vocab_size) by the embedding kernel. */
int lavie_text_encode(lavie_text_t h, const int* ids_dev, int B, int L, void* out_f16, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image conditioning: transformers' CLIPVisionModel and the fork's MappingNetwork (additive in ABI 8)
 * ---------------------------------------------------------------------------------------------- */
/* Bidirectional attention over short sequences with separate query and key lengths: o [NB Lq, ldo] = softmax_j(scale q_i k_j) v_j over
 * j < Lk; q [NB Lq, ldq], k [NB Lk, ldk], v [NB Lk, ldv], head h at columns h dh of each.  Three pointers with their own pitches: columns
 * of one fused q | k | v tensor (the vision tower, the mapper's self-attention) or q from one tensor and k | v from another (its
 * cross-attention).  1 <= Lq <= 320, 1 <= Lk <= 320, dh 32 or 64, NB >= 1, every pitch a multiple of 8 and >= heads dh, every tensor
 * 16-byte aligned: anything else is refused with a message naming the argument and nothing is launched.  Fixed summation order, no
 * atomics; an entry has the bits of its single-entry call. */
int lavie_short_attention_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int NB, int Lq,
                              int Lk, int heads, int dh, float scale, void* stream);
/* CLIPVisionEmbeddings.  pixel_values [B, 3, S, S] NCHW, x_dtype 0 = fp16, 1 = fp32 (as lavie_conv_edge_in_f16), S = G P;
 * out [B, 1 + G^2, C] fp16: row 0 = class_embedding + position 0, row 1 + g = patch g (row-major over the grid) through the P x P
 * stride-P convolution (no bias) + position 1 + g.  wp: the conv weight packed by lavie_pack_patch_embed_f16 ([C, 3, P, P] ->
 * [C, lavie_patch_embed_k(P)], K = 3 P^2 zero-padded to a multiple of 64); workspace: lavie_patch_embed_workspace_bytes(B, S, P)
 * bytes, 16-byte aligned.  C a multiple of 128 up to 2048.  Rounding points: a pixel to fp16 (fp32 input only), the store.  No read
 * outside pixel_values; an image's rows do not depend on B. */
int lavie_patch_embed_k(int P);
long long lavie_patch_embed_workspace_bytes(int B, int S, int P);
int lavie_pack_patch_embed_f16(const void* w, void* out, int C, int P, void* stream);
int lavie_patch_embed_f16(const void* pixel_values, int x_dtype, const void* wp, const void* class_embedding, const void* pos_table,
                          void* out, void* workspace, int B, int S, int P, int C, void* stream);
/* x[0, n) <- max(x, 0) in place, exact: negative values become +0, -0 and +0 keep their bits (torch.relu).  The activation of
 * nn.TransformerDecoderLayer.  (A kind of its own entry: lavie_act_f16 keeps refusing every kind but 0 and 1.) */
#define LAVIE_TEXT_ACT_RELU 2
int lavie_relu_f16(void* x, long long n, void* stream);

typedef struct lavie_vision_s* lavie_vision_t;
typedef struct lavie_vision_config {
    int struct_size;       /* sizeof(lavie_vision_config) as the caller declared it; any other value is refused */
    int hidden;            /* a multiple of 128, <= 2048 */
    int intermediate;      /* a multiple of 128 */
    int layers;
    int heads;             /* hidden / heads must be 32 or 64 */
    int image_size;        /* a multiple of patch_size; 1 + (image_size / patch_size)^2 tokens, <= 320 */
    int patch_size;
    int act;               /* LAVIE_TEXT_ACT_QUICK_GELU or LAVIE_TEXT_ACT_GELU */
    float eps;             /* layer_norm_eps */
} lavie_vision_config;
int lavie_vision_config_size(void);
int lavie_vision_create(const lavie_vision_config* cfg, lavie_vision_t* out);
int lavie_vision_destroy(lavie_vision_t h);
/* The state-dict contract: names are the keys of transformers' CLIPVisionModel.state_dict(), listed with the classic vision_model.
 * prefix (vision_model.embeddings.class_embedding, vision_model.pre_layrnorm.weight, ...); lavie_vision_set_param takes them with or
 * without the prefix.  post_layernorm.weight / .bias are accepted and ignored (they belong to the pooled output, which is not built)
 * and are not listed. */
int lavie_vision_num_params(lavie_vision_t h);
int lavie_vision_param_info(lavie_vision_t h, int i, const char** name, long long* numel);
/* One fp16 tensor, borrowed until lavie_vision_finalize returns and the stream drains. */
int lavie_vision_set_param(lavie_vision_t h, const char* name, const void* data_f16, long long numel);
/* Copies the weights into the handle's own allocation (q | k | v fused, the patch weight packed, biases and norm vectors fp32) and
 * allocates the workspace of the largest call (B = 16).  Allocates; not stream-ordered. */
int lavie_vision_finalize(lavie_vision_t h, void* stream);
/* Bytes of the handle's workspace that lavie_vision_encode(h, ., ., B, ...) uses; -1 for a batch it refuses. */
long long lavie_vision_workspace_bytes(lavie_vision_t h, int B);
/* pixel_values [B, 3, image_size, image_size] (x_dtype 0 = fp16, 1 = fp32) -> out_f16 [B, tokens, hidden] = last_hidden_state of
 * CLIPVisionTransformer: embeddings, pre_layrnorm, the layers; post_layernorm is NOT applied (as in transformers).  1 <= B <= 16.
 * Enqueues 2 + B + 8 layers launches on `stream`; no allocation, no synchronisation (capturable).  Two calls agree bit for bit; an
 * image's [tokens, hidden] block has the same bits at every B and every position in the batch. */
int lavie_vision_encode(lavie_vision_t h, const void* pixel_values, int x_dtype, int B, void* out_f16, void* stream);

typedef struct lavie_mapper_s* lavie_mapper_t;
typedef struct lavie_mapper_config {
    int struct_size;       /* sizeof(lavie_mapper_config) as the caller declared it; any other value is refused */
    int input_dim;         /* width of the vision features, a multiple of 64 */
    int output_dim;        /* width of the text embeddings, a multiple of 128, <= 2048 */
    int layers;
    int heads;             /* output_dim / heads must be 32 or 64 */
    int dim_feedforward;   /* a multiple of 128 */
    int seq_in;            /* vision tokens, <= 320 */
    int seq_out;           /* text tokens, <= 320 */
    float eps;             /* of the three LayerNorms of a layer */
} lavie_mapper_config;
int lavie_mapper_config_size(void);
int lavie_mapper_create(const lavie_mapper_config* cfg, lavie_mapper_t* out);
int lavie_mapper_destroy(lavie_mapper_t h);
/* Names are the keys of MappingNetwork.state_dict() (image_proj.weight, image_pos_embedding, text_pos_embedding,
 * transformer_decoder.layers.0.self_attn.in_proj_weight, ...).  text_proj.weight / .bias are accepted and ignored (the reference's
 * forward never uses them) and are not listed. */
int lavie_mapper_num_params(lavie_mapper_t h);
int lavie_mapper_param_info(lavie_mapper_t h, int i, const char** name, long long* numel);
int lavie_mapper_set_param(lavie_mapper_t h, const char* name, const void* data_f16, long long numel);
int lavie_mapper_finalize(lavie_mapper_t h, void* stream);
/* Bytes of the handle's workspace that an encode of B prompts (and up to B images) uses; -1 for a batch it refuses. */
long long lavie_mapper_workspace_bytes(lavie_mapper_t h, int B);
/* MappingNetwork.forward: image_feats fp16 [Bi, seq_in, input_dim], text fp16 [B, seq_out, output_dim] -> rows row0 .. row0 + seq_out - 1
 * of out fp16 [B, ld_out_rows, output_dim]; the other rows of out are not touched.  ld_out_rows = 154, row0 = 77 puts the result
 * behind the text tokens of a context buffer the caller has filled (ready for lavie_unet_cache_context); the plain form is
 * ld_out_rows = seq_out, row0 = 0.  Bi is 1 (one image for every prompt) or B; 1 <= B <= 16.  Enqueues Bi + B + 13 layers launches; no
 * allocation, no synchronisation (capturable).  Two calls agree bit for bit; a prompt's block has the same bits at every B and
 * position, and with Bi = 1 the bits of Bi = B with the image repeated. */
int lavie_mapper_encode(lavie_mapper_t h, const void* image_feats, int Bi, const void* text, int B, void* out, int ld_out_rows, int row0,
                        void* stream);

/* ---- The encoders' own launches at operator level (additive in ABI 8): what lavie_text_*, lavie_vision_* and
 * lavie_mapper_* launch without the planner of lavie_linear_f16, for per-element checks.
 * C [M, N] (ldc) = A [M, K] (lda) W [N, K]^T + bias [N] (+ R [M, N] (ldr), which may alias C) on the one pinned plan of the encoders:
 * the 128-row kernel at 128 columns, no split-K, whatever M, N and K are; fp32 sum over K in an order that depends on K alone, bias and
 * residual in fp32, one fp16 rounding.  A row's bits do not depend on M or on where the row lies.  lavie_debug_force_tile / _splits do
 * not reach it and lavie_debug_op_statistics_last does not record it.  Refused by name, nothing launched: a null A, W, bias or C,
 * M < 1, N not a multiple of 128, K not a multiple of 64, lda < K or not a multiple of 8, ldc (ldr) < N or not a multiple of 4, a
 * tensor that is not 16-byte aligned.  One launch, capturable. */
int lavie_pinned_linear_f16(const void* A, int lda, const void* W, const float* bias, const void* R, int ldr, void* C, int ldc, int M, int N,
                            int K, void* stream);
/* out fp16 [B, L, C] = fp16(float(x [B, L, C]) + float(pos [L, C])), one rounding: the mapper's target rows plus their positions.
 * C a multiple of 8, 16-byte aligned tensors; a null tensor, B < 1 or L < 1 is refused by name. */
int lavie_add_rows_f16(const void* x, const void* pos, void* out, int B, int L, int C, void* stream);

/* ---- Seeded engine noise (csrc/philox.h, csrc/sampler_noise.hip).  A standard normal as a pure function of (a latent's 64-bit seed,
 * a 64-bit draw number, the element's flat index e inside ONE latent [C, F, h, w]): no generator state exists anywhere, and a latent
 * has the same noise alone, in any batch, on any rank and under any window split.
 *   words = Philox4x32-10(key = (lo, hi of seed), counter = (lo, hi of e >> 2, lo, hi of draw)), multipliers 0xD2511F53 / 0xCD9E8D57,
 *   key increments 0x9E3779B9 / 0xBB67AE85; (w0, w1) give elements 4 (e >> 2) + 0, 1 and (w2, w3) give + 2, 3; for a pair (a, b)
 *   u1 = ((a >> 8) + 1) 2^-24, u2 = (b >> 8) 2^-24, r = sqrt(-2 ln u1), first = r cos(2 pi u2), second = r sin(2 pi u2), in fp32.
 * The stream is this library's own: no equality with torch's or any other library's generator is claimed. */
#define LAVIE_NOISE_MAX_SEEDS 16
/* The integer part on the host: out[4] = Philox4x32-10(key[2], counter[4]).  Needs no device. */
int lavie_philox4x32_host(const unsigned int* key, const unsigned int* counter, unsigned int* out);
/* out fp32 [P, per] (device): row p = elements first_element .. first_element + per - 1 of latent seeds_host[p] at `draw`.  1 <= P <=
 * LAVIE_NOISE_MAX_SEEDS, per >= 1, first_element >= 0, first_element + per <= 2^62.  Sixteen-byte stores, eight elements per lane,
 * when first_element % 4 == 0, per % 8 == 0 and out is 16-byte aligned; otherwise one element per lane: the same bits.  One launch,
 * no allocation, no synchronisation (capturable); seeds_host is read before the call returns. */
int lavie_philox_normal_f32(float* out, const unsigned long long* seeds_host, int P, long long per, long long first_element,
                            unsigned long long draw, void* stream);
/* The key of a step whose noise is made inside the step kernel. */
typedef struct lavie_noise_key {
    int struct_size;                         /* sizeof(lavie_noise_key) as the caller declared it; any other value is refused */
    int count;                               /* latents P, 1..LAVIE_NOISE_MAX_SEEDS */
    const unsigned long long* seeds_host;    /* [count], read before the call returns: the seeds travel as kernel arguments */
    long long per;                           /* elements of one latent */
    unsigned long long draw;
} lavie_noise_key;
/* lavie_sampler_step / lavie_cfg_sampler_step with noise[i] = the normal of (seeds[i / per], draw, i % per), read when sigma != 0: x and
 * model_in have the bits of lavie_philox_normal_f32 (first_element 0) followed by the plain entry.  There is no noise operand; n = count
 * per.  Like the plain entries these have no alignment rule and take their scalars as they come: eight elements per lane when per % 8
 * == 0 and eps, x and model_in are 16-byte aligned, otherwise one, the same bits.  The known-region, table and PAG steps have no seeded
 * form: they take the materialised tensor. */
int lavie_sampler_step_seeded(const void* eps, float* x, void* model_in, long long n, float k_x, float k_eps, float c_x0, float c_xt,
                              float sigma, float next_input_scale, void* stream, const lavie_noise_key* key);
int lavie_cfg_sampler_step_seeded(const void* eps2, float* x, void* model_in2, long long n, float guidance, float k_x, float k_eps,
                                  float c_x0, float c_xt, float sigma, float next_input_scale, void* stream, const lavie_noise_key* key);
/* lavie_window_step for the five-coefficient family (family = 0) with the step's noise made in the kernel: the element's index is its
 * index in the WHOLE clip [C, F, hw] (key->per = C F hw, key->count = P), so the windows do not enter it.  args->aux is not read. */
int lavie_window_step_seeded(const lavie_window_step_args* args, const lavie_noise_key* key, void* stream);
/* Test hook (additive, ABI unchanged): what the step launchers answer to a noise key beside an operand that has no seeded form, which
 * no entry above can pass them.  combine 1: a known region, 2: a guidance table, 3: a perturbed part, 4: the multistep family (plain
 * steps); 5: a guidance table, 6: the multistep family (window step).  Always non-zero with the launcher's refusal in
 * lavie_last_error(); touches no device and launches nothing. */
int lavie_debug_noise_key_refusal(int combine);

/* ---- The denoising objective evaluated forward (additive in ABI 8; csrc/denoise_loss.hip): the noised model input
 * in front of the UNet and the mean squared error against the regenerated target behind it, with the noise of `key` made in
 * registers on both sides.  For latent p of key->count, element e of key->per, in fp32 with every rounding point fixed:
 *   n = the normal of (seeds[p], draw, e); with offset_hw != 0: n = fma(offset_coef, m, n), m = the normal of element e / offset_hw
 *   of (seeds[p], offset_draw), one value per plane of offset_hw elements (a [B, C, F, 1, 1] term);
 *   a = a_host[p] = sqrt(abar_t), s = s_host[p] = sqrt(1 - abar_t) of the latent's timestep, computed by the caller. */
typedef struct lavie_denoise_args {
    int struct_size;                 /* sizeof(lavie_denoise_args) as the caller declared it; any other value is refused */
    int x0_dtype;                    /* 0 = fp16, 1 = fp32 */
    const void* x0;                  /* [count, per] (device): the clean latents, already scaled by the VAE factor */
    const float* a_host;             /* [count], read before the call returns */
    const float* s_host;             /* [count], read before the call returns */
    float offset_coef;               /* read when offset_hw != 0 */
    unsigned long long offset_draw;
    long long offset_hw;             /* 0: no offset noise; otherwise it must divide key->per */
} lavie_denoise_args;
#define LAVIE_LOSS_EPSILON 0
#define LAVIE_LOSS_V_PREDICTION 1
#define LAVIE_LOSS_SAMPLE 2
/* model_in fp16 [count, per] = fp16 of fma(s, n, a x0), rounded once; with s == 0 fp16 of a x0 and no noise is made.  Eight elements per
 * lane when per % 8 == 0 and x0 and model_in are 16-byte aligned, otherwise one: the same bits.  Refused by name, nothing launched: a
 * null args, key, x0, a_host, s_host or model_in, a struct of another size, x0_dtype outside 0..1, count outside
 * 1..LAVIE_NOISE_MAX_SEEDS, per < 1, offset_hw < 0 or not dividing per, a level that is not finite, a tensor that is not aligned to its
 * element.  One launch, no allocation, capturable.  A latent's bits do not depend on count or on its position. */
int lavie_noisy_latents_seeded(const lavie_denoise_args* args, const lavie_noise_key* key, void* model_in, void* stream);
/* fp32 elements of the workspace of the entry below for P latents of `per` elements; -1 for P < 1 or per outside 1..2^40. */
long long lavie_denoising_loss_workspace_floats(int P, long long per);
/* out fp32 [count] (device) = the mean over the latent of the squared difference of pred fp16 [count, per] and the target: n
 * (LAVIE_LOSS_EPSILON), fma(a, n, -(s x0)) (LAVIE_LOSS_V_PREDICTION) or x0 (LAVIE_LOSS_SAMPLE), n having the bits the entry above
 * used.  Fixed order of additions: fp32 sums of depth 17 over chunks of 2048 elements into `workspace`, then a second launch adds a
 * latent's chunks in index order in double and divides by per.  No atomics: two calls agree bit for bit, and a latent's value does not
 * depend on count or on its position.  Refusals as above, and: a null pred, out or workspace, workspace_floats below the query's
 * answer, kind outside 0..2.  Two launches, capturable. */
int lavie_denoising_loss_f32(const lavie_denoise_args* args, const lavie_noise_key* key, const void* pred, int kind, float* out,
                             float* workspace, long long workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CLIP image processor, feature heads and CLIPSIM (additive in ABI 8): pixels and token ids in, context or score out
 * ---------------------------------------------------------------------------------------------- */
/* One axis of Pillow's 8-bit bicubic resampling from `in` samples to `out`, on the host (needs no device): first tap xmin_out[out],
 * tap count count_out[out] and int32 coefficients coeff_out[out, ksize] (scaled by 2^22, zero behind the taps) of every output.
 * Returns ksize = 2 ceil(2 max(in / out, 1)) + 1 (> 0), also when all three pointers are null (the size query); -1 with a message for
 * in or out outside 1..65535 or in / out > 32.  Output x of a row u is clip(0, 255, (2^21 + sum_t u[xmin + t] coeff[x, t]) >> 22). */
int lavie_clip_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out);
typedef struct lavie_clip_preprocess_config {
    int struct_size;       /* sizeof(lavie_clip_preprocess_config) as the caller declared it; any other value is refused */
    int size;              /* the short edge after the resize (CLIPImageProcessor.size["shortest_edge"]); CLIP: 224 */
    int crop;              /* the centre crop's edge (crop_size); CLIP: 224 */
    float mean[3];         /* image_mean; CLIP: 0.48145466, 0.4578275, 0.40821073 */
    float std[3];          /* image_std;  CLIP: 0.26862954, 0.26130258, 0.27577711 */
} lavie_clip_preprocess_config;
/* Bytes of the workspace lavie_clip_preprocess_u8 needs for B images [H, W, 3] (the uint8 image between the two passes, only the
 * source rows and the columns the crop keeps); -1 with a message for a shape that entry refuses. */
long long lavie_clip_preprocess_workspace_bytes(int B, int H, int W, int size, int crop);
/* CLIPImageProcessor (resize the short edge to `size` with Pillow's bicubic filter, centre crop, rescale by 1 / 255, normalise):
 * in_u8 uint8 [B, H, W, 3] on the device, rows row_pitch >= 3 W bytes apart, images image_pitch bytes apart (not read when B = 1)
 * -> out [B, 3, crop, crop], out_dtype 1 = fp32 with the bits of the stock processor's pixel_values, 0 = fp16, one rounding of that
 * value.  cfg null: CLIP's defaults.  The long edge goes to int(size long / short); the crop starts at (resized - crop) / 2.
 * Refused by name, nothing launched: B < 1, a short edge below 8, a scale (source / resized) above 32, crop greater than a resized
 * edge (the stock processor pads there), row_pitch below 3 W, image_pitch below one image, a workspace too small, std of 0.
 * Every refusal comes before the device is touched.  Two launches on `stream`.  The coefficient tables of a (device, H, W, size,
 * crop, mean, std) are made on the host and uploaded the first time that key is seen on the current device (an allocation and a
 * blocking copy: not capturable), then cached.  Only the rows and columns the crop keeps
 * are computed, and no byte outside an image's [H, 3 W] is read.  An image's output does not depend on B or on its position. */
int lavie_clip_preprocess_u8(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype,
                             const lavie_clip_preprocess_config* cfg, void* workspace, long long workspace_bytes, void* stream);
/* out fp32 [B, D] = normalise?(w LN?(x[b, row_b, :])): CLIPModel.get_image_features / get_text_features on a tower's hidden states,
 * L2-normalised when normalize != 0.  x fp16 [B, L, C]; w fp16 [D, C] (visual_projection / text_projection, no bias).  Row: with
 * ids_dev (int32 [B, L], device) the row CLIPTextTransformer pools -- eos_token_id == 2: the first maximum of the ids, otherwise the
 * first position equal to eos_token_id, row 0 when there is none -- else `row`.  ln_gamma / ln_beta fp32 [C] (post_layernorm) or
 * both null.  LayerNorm, projection and norm accumulate in fp32 in a fixed order; nothing is rounded to fp16.  C and D multiples of
 * 128 up to 2048.  One workgroup per item: an item's bits do not depend on B or on its position.  One launch, capturable. */
int lavie_clip_embed_f16(const void* x, int B, int L, int C, const int* ids_dev, int eos_token_id, int row, const float* ln_gamma,
                         const float* ln_beta, float eps, const void* w, int D, int normalize, float* out, void* stream);
/* frames == 0: out fp32 [N, P] = scale <img_n, txt_p> (logits_per_image with scale = exp(logit_scale)).  frames >= 1, N = P frames:
 * out [P] = (100 / frames) sum_f <img_{p frames + f}, txt_p>, the dot products those of the matrix form, added in frame order
 * (CLIPSIM on normalised features).  img fp32 [N, D], txt fp32 [P, D].  Fixed order, no atomics.  One launch, capturable. */
int lavie_clip_similarity_f32(const float* img, const float* txt, float* out, int N, int P, int D, int frames, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FVD on the engine (additive in ABI 8): 3-D convolutions, the R3D-18 feature extractor, the video processor
 * ---------------------------------------------------------------------------------------------- */
/* Halfs of the packed weights of a Conv3d [Cout, Cin, kt, kh, kw]: Cout rows of kt kh kw Cin halfs rounded up to a multiple of 64;
 * -1 for an extent outside 1..7 or a width outside 1..4096. */
long long lavie_conv3d_packed_halfs(int Cout, int Cin, int kt, int kh, int kw);
/* w fp16 [Cout, Cin, kt, kh, kw] -> out fp16 [Cout][kt][kh][kw][Cin], each row zero-padded to a multiple of 64 halfs. */
int lavie_conv3d_pack(const void* w_f16, void* out_f16, int Cout, int Cin, int kt, int kh, int kw, void* stream);
/* The same pack from fp32 weights with the BatchNorm3d behind the conv folded in, as lavie_r3d_finalize runs it: scale = gamma /
 * sqrt(var + eps) in double, out_f16 = fp16(w scale), rounded once from the double product, in lavie_conv3d_pack's layout;
 * shift_f32 [Cout] = fp32(beta - mean scale), the bias of the folded conv.  w fp32 [Cout, Cin, kt, kh, kw]; gamma, beta, mean, var
 * fp32 [Cout].  A null tensor and a shape lavie_conv3d_packed_halfs refuses are refused by name. */
int lavie_conv3d_fold_pack_f32(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, double eps,
                               void* out_f16, float* shift_f32, int Cout, int Cin, int kt, int kh, int kw, void* stream);
/* y = relu?(conv3d(x) + bias + residual) on channels-last fp16 rows: x [N, T, H, W, Cin] -> y [N, To, Ho, Wo, Cout], extents
 * floor((n - 1) / stride) + 1.  Built: ksize 3 (kernel (3,3,3), padding 1) with stride 1 or 2 on all three axes, and ksize 1 (kernel
 * (1,1,1), no padding) with stride 2; Cin and Cout each 64, 128, 256 or 512; everything else is refused by name.  wp: lavie_conv3d_pack's
 * image; bias fp32 [Cout] (required); residual fp16 [N To Ho Wo, Cout] or null, may be y itself.  fp32 accumulation over the taps in
 * (t, h, w) order, channels inside a tap, taps outside the volume contributing zeros; bias, residual and ReLU in fp32; one fp16
 * rounding.  One tile geometry, no split-K, no atomics: an output row's bits depend on its own inputs only.  One launch, capturable. */
int lavie_conv3d_f16(const void* x, const void* wp, const float* bias, const void* residual, int relu, void* y, int N, int T, int H, int W,
                     int Cin, int Cout, int ksize, int stride, void* stream);
/* The stem of a video ResNet: Conv3d(3, 64, kernel (3,7,7), stride (1,2,2), padding (1,3,3)) + bias (+ ReLU) from pixels to
 * channels-last fp16 rows y [N, T, Ho, Wo, 64].  Pixel (n, t, c, h, w) is read at element n stride_n + t stride_t + c stride_c + h W + w
 * of `pixels` (x_dtype 0 = fp16, 1 = fp32, rounded to fp16 on the way in): frames-major planar [N T, 3, H, W] is (3 T H W, 3 H W, H W),
 * channels-first [N, 3, T, H, W] is (3 T H W, H W, T H W); each stride at least H W.  wp: lavie_conv3d_pack(w, ., 64, 3, 3, 7, 7): 448
 * halfs per row, 441 of them weights. */
int lavie_conv3d_stem_f16(const void* pixels, int x_dtype, long long stride_n, long long stride_t, long long stride_c, const void* wp,
                          const float* bias, int relu, void* y, int N, int T, int H, int W, void* stream);
/* out fp32 [N, C] = the mean over the rows of x fp16 [N, rows, C] (AdaptiveAvgPool3d(1) of channels-last rows): per (n, c) four
 * sequential fp32 partials (rows r = g, g + 4, ...) summed (p0 + p1) + (p2 + p3), then one division.  No atomics.  N up to 65535. */
int lavie_mean_rows_f32(const void* x, float* out, int N, int rows, int C, void* stream);

/* R3D-18 without its classifier (torchvision's r3d_18 layout: stem, layer1 .. layer4 of two basic blocks, mean over positions).
 * Lifecycle as lavie_vision_*: create, set_param for every tensor, finalize, then features.  Parameters are fp32 DEVICE tensors,
 * borrowed until finalize's work on `stream` has drained.  Names: stem.0.weight, stem.1.{weight, bias, running_mean, running_var},
 * layerL.B.conv{1,2}.0.weight, layerL.B.conv{1,2}.1.*, layerL.0.downsample.{0.weight, 1.*} (L = 2..4); also with the numeric prefixes
 * of nn.Sequential(*children[:-1]) ("0." = stem, "1." .. "4." = layer1 .. layer4).  fc.* and *.num_batches_tracked are accepted and
 * ignored; any other name, and a wrong element count, is refused by name.  finalize folds every BatchNorm (eps 1e-5) into its conv:
 * scale = weight / sqrt(running_var + eps) in double, conv weight times scale rounded once to fp16, shift = bias - running_mean scale
 * kept in fp32; a tensor never set is refused by name. */
typedef struct lavie_r3d_s* lavie_r3d_t;
int lavie_r3d_create(lavie_r3d_t* out);
int lavie_r3d_destroy(lavie_r3d_t h);
int lavie_r3d_num_params(lavie_r3d_t h);
int lavie_r3d_param_info(lavie_r3d_t h, int i, const char** name, long long* numel);
int lavie_r3d_set_param(lavie_r3d_t h, const char* name, const void* data_f32, long long numel);
int lavie_r3d_finalize(lavie_r3d_t h, void* stream);
/* Bytes of the workspace lavie_r3d_features(h, ..., N, T, H, W, ...) uses; -1 with a message for a shape it refuses. */
long long lavie_r3d_workspace_bytes(lavie_r3d_t h, int N, int T, int H, int W);
/* out_f32 [N, 512] = the features of N clips of T frames H x W, any extents >= 1 (the model's own: 16 x 224 x 224).  pixels, x_dtype
 * and the three strides as lavie_conv3d_stem_f16.  Refused by name, nothing launched: a null handle or tensor, a handle that is not
 * finalized, an extent below 1, N above 65535, strides below H W, a workspace below lavie_r3d_workspace_bytes.  21 launches on
 * `stream`, capturable.  A clip's features have the same bits at every N and at every position in the batch. */
int lavie_r3d_features(lavie_r3d_t h, const void* pixels, int x_dtype, long long stride_n, long long stride_t, long long stride_c, int N,
                       int T, int H, int W, float* out_f32, void* workspace, long long workspace_bytes, void* stream);

/* One axis of Pillow's 8-bit BILINEAR resampling (support max(in / out, 1)); everything else as lavie_clip_resample_table_host.
 * Returns ksize = 2 ceil(max(in / out, 1)) + 1. */
int lavie_video_resample_table_host(int in, int out, int* xmin_out, int* count_out, int* coeff_out);
long long lavie_video_preprocess_workspace_bytes(int B, int H, int W, int crop, int size);
/* The per-frame transform of the FVD evaluation: centre crop of `crop` x `crop` pixels (offsets round-half-even((n - crop) / 2), as
 * torchvision's CenterCrop), Pillow's bilinear resize of that square to size x size, rescale by 1 / 255, normalise.  in_u8 uint8
 * [B, H, W, 3] -> out [B, 3, size, size]; pitches, out_dtype, workspace, the table cache and the refusals as lavie_clip_preprocess_u8,
 * with these differences: a crop greater than H or W is refused (the stock transform pads there), the scale is crop / size.  mean and
 * std point at three floats each (host).  fp32 output has the bits of Pillow followed by (v / 255 - mean) / std in fp32. */
int lavie_video_preprocess_u8(const void* in_u8, int B, int H, int W, long long row_pitch, long long image_pitch, void* out, int out_dtype,
                              int crop, int size, const float* mean3, const float* std3, void* workspace, long long workspace_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LAVIE_HIP_H */
