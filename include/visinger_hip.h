/*
 * visinger_hip.h -- C ABI of the MI355X-native (gfx950) VISinger variational-inference hot path.
 *
 * The reference (jisang93/VISinger) has no FFI: its boundary for this path is the Python nn.Module API of
 * modules/visinger/{encoder,flow,decoder,predictor}.py and modules/rel_transformer.py.  This header
 * is the C ABI that sits directly under that API: every entry point below is what one reference
 * ``nn.Module.forward`` (cited file:line, paths under the reference tree) binds to.  The Python mirror of the
 * module API that calls it through ctypes lives in visinger_amd/modules/ (see INTEGRATION.md).
 *
 * Conventions
 *   - all tensors are fp32, contiguous, device (HBM) pointers unless stated; layout [B, C, T] (T fastest);
 *   - frame masks are fp32 [B, T] (the reference's [B, 1, T] nonpadding mask);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); nothing here synchronises the device;
 *   - handles own their packed weights and workspaces in HBM (hipMalloc at create / first use of a shape, never
 *     on the steady-state path);  weights are handed over in the reference's own state_dict layout
 *     (``weight_v`` / ``weight_g`` / ``bias``) and are folded (g * v / ||v||) and re-packed into MFMA fragment
 *     order on the device by the *_set_weights call;
 *   - every function returns VS_OK (0) or an error code; vs_last_error() returns a thread-local message.
 *     Nothing aborts, nothing falls back to a CPU path.
 */
#ifndef VISINGER_HIP_H
#define VISINGER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_API __attribute__((visibility("default")))

enum vs_status { VS_OK = 0, VS_EINVAL = 1, VS_EHIP = 2, VS_EUNSUPPORTED = 3, VS_ENOMEM = 4 };

VS_API const char *vs_last_error(void);
/* Name of the kernel instance the calling thread's last vs_conv_forward / vs_respair_forward / vs_relattn_fwd launched, spelled as
 * rocprofv3 prints it without the namespace and argument list ("conv_split_kernel<1, 8, 4, 1, 6>"): the dispatch is decided in
 * this library, so a caller that attributes per-launch timings to kernel instances (bench.py's roofline line) reads it back
 * here instead of restating the selection.  Thread-local; "" before the first launch.  (No reference counterpart.)          */
VS_API const char *vs_last_kernel_name(void);
VS_API int vs_abi_version(void);          /* 7: vs_retime_tokens, vs_retime_frames, vs_f0_norm_interp, vs_pitch_condition, vs_normal_fill, vs_prior_sample (appended to 7: new exports only, no layout or signature changed),vs_conv_set_weights_batch, vs_weight_norm_multi_fwd / _bwd, vs_conv_wgrad_bias, vs_wn_step_fwd / _bwd, vs_l1_mean_fwd / _bwd; 6: vs_source_hash, vs_bias_grad, vs_conv_set_weights_pair; 5: vs_relattn_fwd_work / vs_relattn_kv_work_bytes; 4: vs_set_option / vs_get_option / vs_reset_option; 3: vs_dtype in vs_conv_io_t; 2: vs_relattn_fwd(math) */
/* sha256 (hex) over the sources this library was compiled from (kernels, headers, textual includes, the build recipe), embedded by
 * visinger_amd/csrc/build.py.  The loader recomputes it over the tree it sits in and refuses a library built from other sources (a
 * stale object that an mtime check would pass after a checkout).  (No reference counterpart: the reference has no native code.)  */
VS_API const char *vs_source_hash(void);
/* Dispatch switches (A/B comparisons and debugging; never needed for correct results).  The library reads the environment
 * variables of the same names ONCE, when it is loaded; afterwards only these calls change a switch, and no launch path touches
 * the environment.  Names and meanings: INTEGRATION.md "Switches".  Unknown name -> VS_EINVAL.  (No reference counterpart: the
 * reference steers nothing on this path but `hparams`.)                                                                       */
VS_API int vs_set_option(const char *name, long long value);
VS_API int vs_get_option(const char *name, long long *value);
VS_API int vs_reset_option(const char *name);
/* number of HIP devices visible / name of device 0 written into buf (diagnostics for the loader) */
VS_API int vs_device_info(char *buf, size_t buf_bytes);

/* ------------------------------------------------------------------------------------------------------------
 * a12  weight-norm fold: w[r, :] = g[r] * v[r, :] / ||v[r, :]||_2
 *      (torch.nn.utils.weight_norm at modules/visinger/encoder.py:147,154,164; decoder.py:24,72-87)          */
VS_API int vs_weightnorm_fold(const float *v, const float *g, float *w, int64_t rows, int64_t cols, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Conv1d / ConvTranspose1d operator handle -- every nn.Conv1d / nn.ConvTranspose1d site of the path
 * (encoder.py:88,90,152,163; flow.py:60,62; decoder.py:19,24-26,34,72-87; rel_transformer.py:120-128,332-333).
 * Implicit GEMM on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32).                                */
typedef struct vs_conv vs_conv_t;

enum vs_conv_kind {
    VS_CONV1D = 0,           /* y[b,co,t] = bias[co] + sum w[co,ci,k] x[b,ci,t + k*dil - pad]                  */
    VS_CONV_TRANSPOSE1D = 1, /* nn.ConvTranspose1d, w is [c_in, c_out, k]; `dilation` carries the stride        */
    VS_CONV1D_PAIRED = 2     /* Conv1d whose c_out = 2*H rows are consumed as (row c, row H+c) pairs by a fused
                                epilogue: WaveNet gate (encoder.py:206-213) or affine coupling (flow.py:71-85) */
};
enum vs_in_act {
    VS_IN_NONE = 0,
    VS_IN_LRELU = 1,      /* leaky_relu(x, 0.1)                 */
    VS_IN_MASK = 2,       /* x * mask[b,t]                      */
    VS_IN_LRELU_MASK = 3  /* leaky_relu(x, 0.1) * mask[b,t]     (decoder.py:93-95) */
};
enum vs_out_act { VS_OUT_NONE = 0, VS_OUT_TANH = 1, VS_OUT_RELU = 2 };
enum vs_pair_mode { VS_PAIR_GATE = 0, VS_PAIR_COUPLING_FWD = 1, VS_PAIR_COUPLING_INV = 2 };
enum vs_out_mode {
    VS_OUT_LINEAR = 0,            /* y = act((v + res + acc) * scale) [* mask]                                  */
    VS_OUT_COUPLING_MEAN_FWD = 1, /* y = v*mask + res*mask                 (flow.py:74,78 with mean_only)        */
    VS_OUT_COUPLING_MEAN_INV = 2  /* y = (res - v*mask) * mask             (flow.py:74,83 with mean_only)        */
};

/* flags for vs_conv_create */
#define VS_CONV_FLIP_IN 1u  /* read input channels in reversed order  (folds flow.py:88-95 Flip into the weights) */
#define VS_CONV_FLIP_OUT 2u /* write output rows in reversed order (within each half for PAIRED)                 */
#define VS_CONV_ADJOINT 4u  /* VS_CONV1D only: vs_conv_set_weights is handed the weight of the FORWARD conv this handle is the grad-input
                               of, [c_in, c_out, k] of THIS handle, and packs its adjoint w'[co, ci, t] = w[ci, co, k - 1 - t] (channel
                               transpose + tap reversal by index arithmetic: no flipped copy per training step); g must be NULL      */

VS_API int vs_conv_create(vs_conv_t **out, int kind, int c_in, int c_out, int k, int dilation_or_stride, int padding,
                          unsigned flags);
VS_API void vs_conv_destroy(vs_conv_t *h);
/* w: [c_out, c_in, k] ([c_in, c_out, k] for transpose).  g == NULL: w is the effective weight;
 * g != NULL: w is weight_v and g is weight_g ([dim0,1,1]) -> folded on the device.  bias may be NULL.          */
VS_API int vs_conv_set_weights(vs_conv_t *h, const float *w, const float *g, const float *bias, void *stream);
/* The same for TWO handles fed from one plain (already folded) weight `w` -- a conv and the VS_CONV_ADJOINT handle of its grad-input -- in
 * one pair of launches instead of two: the training step packs every weight version for both (autograd.HipConvFn).  bias0: h0's bias or
 * NULL; h1 gets none.  Falls back to two vs_conv_set_weights calls outside the split-f16 arithmetic.  (No reference counterpart.)       */
VS_API int vs_conv_set_weights_pair(vs_conv_t *h0, vs_conv_t *h1, const float *w, const float *bias0, void *stream);
/* The same for n handles, each from its own plain (already folded) weight w[i] and bias[i] (bias, or bias[i], may be NULL) -- every conv of a
 * network at the top of a training pass -- in TWO launches for the whole batch (fp32 fragments + largest |w| of every handle; then the f16
 * planes): the reference re-derives each module's weight inside its forward (torch.nn.utils.weight_norm's hook, modules/commons/... conv
 * modules); a training step packed ~340 handles with four launches a pair.  No handle may appear twice.  Handles outside VS_MATH_SPLIT3 (and
 * the <= 4-row VALU convs) take vs_conv_set_weights inside the call.  Stages a table through pinned host memory: not capturable into a graph.  */
VS_API int vs_conv_set_weights_batch(vs_conv_t *const *handles, const float *const *w, const float *const *bias, int n, void *stream);

/* Arithmetic of the matrix contraction of one conv handle (inputs, outputs and accumulation are fp32 in every mode):
 *   VS_MATH_F32    exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), Winograd F(2,3) instances where they measured faster
 *   VS_MATH_SPLIT6 operands split exactly into three bf16 planes, the six leading cross products on v_mfma_f32_32x32x16_bf16:
 *                  fp32-class result (dropped terms <= 2^-23 relative per product) at 16/6 of the fp32 matrix rate (default)
 *   VS_MATH_SPLIT3 operands split into two f16 planes, x * s = xh + xl (22 significant bits; s = a power of two per staged tile /
 *                  per conv weight that puts the largest magnitude below 2^15, found on the device, taken out again in fp32), the
 *                  three leading cross products on v_mfma_f32_32x32x16_f16: representation + dropped term <= 2^-22 relative per
 *                  product, below the rounding of the fp32 accumulation itself; 16/3 of the fp32 matrix rate
 *   VS_MATH_BF16   operands rounded to bf16 (RNE), fp32 accumulate: BASELINE.json's long-form bf16 configuration
 * May be called before or after vs_conv_set_weights (the bf16 planes are re-packed from the fp32 fragments).
 * No reference counterpart: its arithmetic is whatever torch picks (config/models/base_config.yaml:5 `amp: false` = fp32).   */
enum vs_conv_math { VS_MATH_F32 = 0, VS_MATH_BF16 = 1, VS_MATH_SPLIT3 = 3, VS_MATH_SPLIT6 = 6 };
VS_API int vs_conv_set_math(vs_conv_t *h, int math, void *stream);
VS_API int vs_conv_get_math(const vs_conv_t *h);

/* Element type of a conv launch's activation tensors.  VS_DTYPE_BF16 = bf16-RESIDENT activations (BASELINE.json config 5: "bf16
 * activations"): with VS_MATH_BF16 every product rounds its operands to bf16 anyway, and on the bf16 matrix pipe the 128- / 256-channel
 * convs are HBM-bound with fp32 tensors (x + residual + y at 4.3-4.6 TB/s).  Plain VS_CONV1D / VS_CONV_TRANSPOSE1D launches in
 * VS_MATH_BF16 with VS_OUT_LINEAR outputs and no split_row; all strides stay in ELEMENTS; mask and bias_b stay fp32; y is rounded to
 * nearest even once, after residual / accumulate / scale / activation in fp32.                                                  */
enum vs_dtype { VS_DTYPE_F32 = 0, VS_DTYPE_BF16 = 1 };

/* One output destination of a conv launch.  Strides are in floats; row stride is always the time length. */
typedef struct vs_conv_out {
    float *y;            /* [B, rows, T_out] with batch stride y_bs                                              */
    const float *res;    /* optional residual input, same indexing as y (batch stride res_bs); may alias y       */
    const float *acc;    /* optional accumulate input, same indexing as y (batch stride acc_bs); may alias y     */
    int64_t y_bs, res_bs, acc_bs;
    float scale;         /* applied after the adds; 0.0f means unset (= 1.0f)                                    */
    int out_act;         /* enum vs_out_act                                                                      */
    int out_mask;        /* != 0: multiply by mask[b, t]                                                         */
    int mode;            /* enum vs_out_mode                                                                     */
} vs_conv_out_t;

typedef struct vs_conv_io {
    const float *x;      /* [B, c_in, T] with batch stride x_bs (0 -> c_in*T)                                    */
    int64_t x_bs;
    int64_t B, T;
    int in_act;          /* enum vs_in_act, applied while staging x into LDS                                     */
    int x_dtype;         /* enum vs_dtype of x (ABI 3; occupies what was padding: 0 = fp32 as before)            */
    const float *mask;   /* [B, T] frame mask for VS_IN_MASK / out_mask / coupling modes (NULL if unused)        */
    const float *bias_b; /* optional per-item bias [B, c_out] (conditioning), row stride bias_b_bs               */
    int64_t bias_b_bs;
    int split_row;       /* rows [0, split_row) go to out[0], rows [split_row, c_out) to out[1] (row - split_row);
                            0 or >= c_out: everything goes to out[0]                                             */
    int y_dtype;         /* enum vs_dtype of out[0].y / res / acc (ABI 3; was padding)                           */
    vs_conv_out_t out[2];
    int pair_mode;       /* PAIRED only: enum vs_pair_mode; result rows = c_out/2, written through out[0]
                            (res = x1 for the coupling modes)                                                    */
    float *logdet;       /* PAIRED + COUPLING_FWD: [B] accumulated (+=) with sum(logs * mask); may be NULL       */
} vs_conv_io_t;

VS_API int vs_conv_forward(vs_conv_t *h, const vs_conv_io_t *io, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * a11  A whole MRF residual block (or any even-length prefix / suffix of its conv chain) in ONE launch on the split-f16 arithmetic:
 *      for each pair (conv1, conv2):  x = conv2(lrelu(conv1(lrelu(x)))) + x;   y = (x [+ io->out[0].acc]) * io->out[0].scale
 *      (modules/visinger/decoder.py:91-104; the accumulate input and the scale carry the MRF sum of decoder.py:52-56).
 *      convs = {convs1[0], convs2[0], convs1[1], convs2[1], ...}: 2, 4 or 6 handles of 32, 64 or 128 channels, one odd kernel size <= 11,
 *      "same" padding, all in VS_MATH_SPLIT3 (x / acc / y fp32 tensors) or all in VS_MATH_BF16 (x / acc / y bf16-RESIDENT, x_dtype =
 *      y_dtype = VS_DTYPE_BF16: BASELINE.json configs[4]); the other combinations are refused.  The residual stream stays in registers (fp32) between the pairs; each tile recomputes
 *      its receptive halo instead of exchanging it.  io: x, B, T, in_act = VS_IN_LRELU, out[0].y / acc / scale; nothing else.        */
VS_API int vs_resblock_supported(vs_conv_t *const *convs, int nconv);
VS_API int vs_resblock_forward(vs_conv_t *const *convs, int nconv, const vs_conv_io_t *io, void *stream);

/* One launch for a residual pair of the MRF blocks on the 32- / 64-channel stages (decoder.py:92-101):
 *     y = conv2(lrelu(conv1(lrelu(x)) + b1)) + b2 + res [+ acc] [* scale]
 * conv1 / conv2 are existing handles (weights set): same channel count C in {32, 64}, same odd k <= 13, "same" padding, conv2
 * undilated.  io: x, B, T, in_act = VS_IN_LRELU, out[0] = {y, res, acc, strides, scale}; no mask / bias_b / split / activation.
 * vs_respair_supported() tells whether a pair qualifies (callers fall back to two vs_conv_forward launches otherwise).       */
VS_API int vs_respair_supported(const vs_conv_t *conv1, const vs_conv_t *conv2);
VS_API int vs_respair_forward(vs_conv_t *conv1, vs_conv_t *conv2, const vs_conv_io_t *io, void *stream);

/* Weight gradient of a stride-1 (dilated) conv, the backward of nn.Conv1d under the training step (trainer.py:306-384 ->
 * autograd of encoder.py / flow.py / decoder.py convs):  gw[co, ci, k] = sum_{b,t} gy[b, co, t] * x[b, ci, t + k*dil - pad],
 * x read as 0 outside [0, T_in).  gy: [B, c_out, T_out], x: [B, c_in, T_in].  The reduction over (b, t) is cut into slices
 * that each write one partial plane: gw_planes is [vs_conv_wgrad_planes(...)][c_out, c_in, k], every plane fully written, and
 * gw = sum of the planes (deterministic; the caller reduces).  k <= 16, (k-1)*dil <= 64.
 * (The grad-input is vs_conv_forward with the reversed / transposed weight.)                                            */
VS_API int vs_conv_wgrad_planes(int64_t B, int64_t c_out, int64_t c_in, int64_t T_out, int k);
VS_API int vs_conv_wgrad(const float *gy, const float *x, float *gw_planes, int64_t B, int64_t c_out, int64_t c_in,
                         int64_t T_out, int64_t T_in, int k, int dil, int pad, void *stream);
/* The same with the reduction of the planes done here and, with_bias != 0, the conv's bias gradient gb[co] = sum_{b,t} gy[b, co, t] from the
 * same pass over gy (the workgroups of the first c_in tile sum their gy rows): what autograd computes for the `weight` and `bias` arguments of
 * torch.nn.functional.conv1d, in two launches.  work: vs_conv_wgrad_planes(...) * (c_out * c_in * k + (with_bias ? c_out : 0)) floats of
 * scratch; out: c_out * c_in * k floats of gw followed, with_bias, by c_out floats of gb.  Deterministic (fixed plane order).              */
VS_API int vs_conv_wgrad_bias(const float *gy, const float *x, float *work, float *out, int with_bias, int64_t B, int64_t c_out,
                              int64_t c_in, int64_t T_out, int64_t T_in, int k, int dil, int pad, void *stream);
/* length of the time axis produced for an input of length T */
VS_API int64_t vs_conv_out_len(const vs_conv_t *h, int64_t T);

/* ------------------------------------------------------------------------------------------------------------
 * a6  windowed relative-position self-attention core: MultiHeadAttention.attention
 *     (modules/rel_transformer.py:148-179 with the relative helpers 181-243).
 *     q, k, v: [B, n_heads*k_channels, T] (the outputs of conv_q/k/v; they may live in one [B, 3C, T] buffer, hence
 *     the shared batch stride).  rel_k / rel_v: [n_heads_rel, 2*window+1, k_channels] (emb_rel_k / emb_rel_v);
 *     window_size < 0 disables the relative terms.  mask: [B, T] frame mask m, attention mask = m[i]*m[j]; masked
 *     scores are SET to -1e4 (fully masked rows come out uniform, never NaN).  out: [B, n_heads*k_channels, T].
 *     Streaming softmax: no [T, T] tensor is materialised (the reference's `self.attn` is not produced).
 *     math (enum vs_conv_math, declared below): VS_MATH_BF16 rounds q / sqrt(dk), k, v and the probabilities to bf16 and runs both
 *     GEMMs on the bf16 matrix instruction with fp32 accumulation (softmax statistics and relative terms stay fp32) -- BASELINE.json's
 *     long-form bf16 configuration; VS_MATH_SPLIT3 (the default arithmetic of the path) / VS_MATH_SPLIT6: the same operands as two f16
 *     planes under power-of-two scales (per query, per K tile, running per V tile) with three cross products / as three bf16 planes with
 *     six -- fp32-class results on the f16 / bf16 matrix instruction, heads of up to 128 channels; VS_MATH_F32, and every shape those
 *     kernels do not take (T % 4 != 0, unaligned rows, wider heads in the split arithmetics): the exact-fp32 matrix instruction.        */
VS_API int vs_relattn_fwd(const float *q, const float *k, const float *v, int64_t qkv_batch_stride, const float *rel_k,
                          const float *rel_v, const float *mask, float *out, int64_t out_batch_stride, int64_t B,
                          int n_heads, int k_channels, int64_t T, int window_size, int n_heads_rel, int math, void *stream);

/* The same with the KEYS of every (batch, head) cut into `ksplit` ranges (1..16) that run as separate workgroups and are merged by a
 * second kernel: for launches too small to fill the chip (a single utterance is 16 workgroups of 32 serial key tiles).  `work`:
 * B * n_heads * ksplit * (k_channels + 2 + 2 * window + 1) * T floats of scratch.  Only the f16- / bf16-pipe kernels (VS_MATH_SPLIT3 /
 * VS_MATH_SPLIT6 / VS_MATH_BF16 on shapes they take) split; any other case runs exactly as vs_relattn_fwd.                           */
VS_API int vs_relattn_fwd_ksplit(const float *q, const float *k, const float *v, int64_t qkv_batch_stride, const float *rel_k,
                                 const float *rel_v, const float *mask, float *out, int64_t out_batch_stride, int64_t B, int n_heads,
                                 int k_channels, int64_t T, int window_size, int n_heads_rel, int math, float *work, int ksplit,
                                 void *stream);

/* The same with caller-provided scratch for PRE-PACKED keys / values (VS_MATH_BF16, long sequences): every 32- / 64-key tile of K and V
 * is converted to bf16 and laid out as the attention kernel's LDS image ONCE per launch (attn_pack_kv_kernel) instead of once per
 * 128-query block inside it (T / 128 times).  vs_relattn_kv_work_bytes() tells how many bytes `kv_work` (16-byte aligned) must hold for
 * a launch, 0 where pre-packing does not apply (other arithmetics, T < 1024, VS_NO_ATTN_KVPACK); with kv_work NULL or too small the
 * call behaves exactly as vs_relattn_fwd_ksplit.  Outputs are bit-identical either way (the same bf16 operands in the same order).   */
VS_API size_t vs_relattn_kv_work_bytes(int64_t B, int n_heads, int k_channels, int64_t T, int math);
VS_API int vs_relattn_fwd_work(const float *q, const float *k, const float *v, int64_t qkv_batch_stride, const float *rel_k,
                               const float *rel_v, const float *mask, float *out, int64_t out_batch_stride, int64_t B, int n_heads,
                               int k_channels, int64_t T, int window_size, int n_heads_rel, int math, float *work, int ksplit,
                               void *kv_work, size_t kv_work_bytes, void *stream);

/* a7  channel LayerNorm with its neighbours fused (rel_transformer.py:24-42; call sites 297-299, 305-307, 314-316):
 *     y = ((LayerNorm_C(a + r) * gamma + beta) + g) * mask      r, g, mask optional.
 *     g is the conditioning added at the top of the NEXT encoder layer: [B, C, T] (g_time_stride = 1,
 *     g_batch_stride = C*T) or [B, C, 1] broadcast over time (g_time_stride = 0, g_batch_stride = C).            */
VS_API int vs_layernorm_c_fwd(const float *a, const float *r, const float *gamma, const float *beta, const float *g,
                              int64_t g_batch_stride, int g_time_stride, const float *mask, float *y, int64_t B,
                              int64_t C, int64_t T, float eps, void *stream);

/* Training path: the elementwise neighbours of the convs as one forward and one backward launch each, where autograd
 * through PyTorch-ROCm ops took 10-25 small kernels.
 *   vs_gate_fwd / vs_gate_bwd: the WaveNet gate (modules/visinger/encoder.py:206-213 fused_add_tanh_sigmoid_multiply + the conditioning
 *     add of :177-180): acts[b, c, t] = tanh(x_in[b, c, t] + g[b, c]) * sigmoid(x_in[b, H + c, t] + g[b, H + c]).  x_in: [B, 2H, T];
 *     g: optional per-item bias, row b at g + b * g_bs (the layer's 2H-slice of the cond_layer output); acts / dacts: [B, H, T];
 *     dx_in: [B, 2H, T] = d loss / d x_in (= d / d g before the sum over t); dg (optional): += sum_t dx_in[b, :, t], row stride dg_bs.
 *   vs_layernorm_c_bwd: backward of y = LayerNorm_C(a + r) * gamma + beta (rel_transformer.py:33-42; r optional): dx [B, C, T] is the
 *     gradient w.r.t. a (and r); dgamma / dbeta are PER-ITEM partial sums: row b of a zero-initialised [B, 2, C] buffer holds
 *     (dgamma_b, dbeta_b) -- pass dgamma = buf, dbeta = buf + C -- accumulated with float atomics over the item's 64-frame blocks
 *     only (one [C] row for the whole batch serialised 128 workgroups on every address); the caller sums over b.                */
VS_API int vs_gate_fwd(const float *x_in, const float *g, int64_t g_bs, float *acts, int64_t B, int64_t H, int64_t T, void *stream);
VS_API int vs_gate_bwd(const float *x_in, const float *g, int64_t g_bs, const float *dacts, float *dx_in, float *dg, int64_t dg_bs,
                       int64_t B, int64_t H, int64_t T, void *stream);
/*   vs_wn_step_fwd / vs_wn_step_bwd: the residual / skip update behind a WaveNet layer's res_skip conv (modules/visinger/encoder.py:186-193):
 *     x_new = (x + rs[:, :H]) * mask, out_new = out_acc + rs[:, H:] with rs [B, 2H, T], x / out_acc / x_new / out_new [B, H, T], mask [B, T];
 *     out_acc NULL: the first layer (out_new = rs[:, H:]).  Backward: d_rs[:, :H] = dx = dx_new * mask, d_rs[:, H:] = dout_new (NULL inputs: zeros);
 *     the gradient of out_acc is dout_new itself.                                                                                              */
VS_API int vs_wn_step_fwd(const float *x, const float *rs, const float *out_acc, const float *mask, float *x_new, float *out_new, int64_t B,
                          int64_t H, int64_t T, void *stream);
/*   vs_l1_mean_fwd / vs_l1_mean_bwd: out[0] = mean |a - b| over n elements and d/da = sign(a - b) * gout[0] / n (the feature-matching loss terms,
 *     tasks/visinger.py:162-169), one launch each, deterministic.  work: 257 floats the caller keeps (work[256] starts as 0 and returns to 0);
 *     calls that share `work` must be ordered on one stream.                                                                                       */
VS_API int vs_l1_mean_fwd(const float *a, const float *b, float *work, float *out, int64_t n, void *stream);
VS_API int vs_l1_mean_bwd(const float *a, const float *b, const float *gout, float *da, int64_t n, void *stream);
VS_API int vs_wn_step_bwd(const float *dx_new, const float *dout_new, const float *mask, float *d_rs, float *dx, int64_t B, int64_t H,
                          int64_t T, void *stream);
/* gb[c] = sum over (b, t) of gy[b, c, t]: the bias gradient of every conv of the training path (what autograd computes for the `bias`
 * argument of torch.nn.functional.conv1d for the convs of modules/visinger under tasks/visinger.py:53-89), deterministic, one launch.     */
VS_API int vs_bias_grad(const float *gy, float *gb, int64_t B, int64_t C, int64_t T, void *stream);
/* torch.nn.utils.weight_norm (dim 0) of n tensors in one launch each way: w_i[r, :] = g_i[r] * v_i[r, :] / ||v_i[r, :]||, the row norms kept
 * for the backward (what torch._weight_norm / its backward compute per tensor; the reference applies weight_norm to every conv of
 * modules/visinger and the discriminators).  table: DEVICE memory, n rows of 8 x int64 {v, g, w, norm, rows, cols, first row, 0} with
 * first row = the running sum of `rows`; total_rows = the sum.  grads: DEVICE memory, n rows of 4 x int64 {gw, gv, gg, 0}: gw = dL/dw_i
 * (0: the tensor takes no gradient and its outputs are left untouched), gv / gg receive dL/dv_i and dL/dg_i.                                  */
VS_API int vs_weight_norm_multi_fwd(const void *table, int64_t n, int64_t total_rows, void *stream);
VS_API int vs_weight_norm_multi_bwd(const void *table, const void *grads, int64_t n, int64_t total_rows, void *stream);
VS_API int vs_layernorm_c_bwd(const float *a, const float *r, const float *gamma, const float *dy, float *dx, float *dgamma,
                              float *dbeta, int64_t B, int64_t C, int64_t T, float eps, void *stream);

/* Layout kernels of a strided dense conv run as the stride-1 conv of its input phases (the period / scale discriminators' stride-3 / stride-1
 * convs on vs_conv_forward, modules/discriminator.py:20-24, 55-60):
 *   vs_phase_stack:   x [N, C, T] (element strides sn, sc, st: any view) -> xf [stride * C][cols], cols >= N * Hq:
 *                     xf[r * C + c][n * Hq + j] = x[n][c][j * stride + r - pad], zero outside [0, T) and in the columns past the last
 *                     item -- N items end to end as ONE sequence;
 *   vs_phase_items:   to_sequence = 1: items src [N, C, Tv] -> dst [C][ld] at column n * Hq + j (zeros for Tv <= j < Hq);
 *                     to_sequence = 0: the inverse, sequence src [C][ld] -> items dst [N, C, Tv];
 *   vs_phase_unstack: the adjoint of vs_phase_stack, gxf [stride * C][ld] -> gx [N, C, T].                                              */
VS_API int vs_phase_stack(const float *x, int64_t sn, int64_t sc, int64_t st, float *xf, int64_t N, int64_t C, int64_t T, int stride, int pad,
                          int64_t Hq, int64_t cols, void *stream);
VS_API int vs_phase_items(const float *src, float *dst, int64_t N, int64_t C, int64_t Tv, int64_t Hq, int64_t ld, int to_sequence, void *stream);
VS_API int vs_phase_unstack(const float *gxf, int64_t ld, float *gx, int64_t N, int64_t C, int64_t T, int stride, int pad, int64_t Hq,
                            void *stream);

/* Training-mode attention core (rel_transformer.py:148-179 incl. the relative terms of :181-243 and the dropout of :173), streaming:
 * no [T, T] tensor in either direction.  q / k / v / out / dout / dq / dk / dv: [B, n_heads * k_channels, T] (batch strides given, 0 =
 * dense); rel_k / rel_v: [n_heads_rel, 2 * window + 1, k_channels] (window_size < 0: none); mask: [B, T] or NULL (scores of masked
 * (query, key) pairs are filled with -1e4 as the reference does; their gradient is zero).  Exact-fp32 MFMA; heads of <= 128 channels.
 *   forward:  out, and lse [2][B, n_heads, T] = per query the maximum score m and log sum_k exp(score - m) (saved for the backward; kept
 *             apart because a fully masked row has m = -1e4, where fp32 m + log(sum) would round the log away);
 *   dropout:  p_drop on the probabilities, mask = a counter-based hash of (seed, batch * head, query, key): pass the same seed to the
 *             backward.  Not torch's random stream (the reference's own masks are not reproducible across devices either);
 *   backward: dq, dk, dv; d rel_k / d rel_v as PARTIAL sums drel_*_part [B * n_heads * ceil(T / 32)][2 * window + 1][k_channels] that the
 *             caller reduces over the leading axis (per head, or over all heads when the tables are shared) -- deterministic, no atomics;
 *             work: B * n_heads * T * (3 + 4 * window) floats of scratch (row sums D, per-query relative dots).                       */
VS_API int vs_relattn_train_fwd(const float *q, const float *k, const float *v, int64_t qkv_batch_stride, const float *rel_k,
                                const float *rel_v, const float *mask, float *out, int64_t out_batch_stride, float *lse, int64_t B,
                                int n_heads, int k_channels, int64_t T, int window_size, int n_heads_rel, float p_drop, uint64_t seed,
                                void *stream);
VS_API int vs_relattn_train_bwd(const float *q, const float *k, const float *v, int64_t qkv_batch_stride, const float *rel_k,
                                const float *rel_v, const float *mask, const float *out, const float *dout, int64_t out_batch_stride,
                                const float *lse, float *dq, float *dk, float *dv, int64_t grad_batch_stride, float *work,
                                float *drel_k_part, float *drel_v_part, int64_t B, int n_heads, int k_channels, int64_t T, int window_size,
                                int n_heads_rel, float p_drop, uint64_t seed, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f2  on-device linear / mel spectrograms (utils/audio/mel_processing.py:15-38: torchaudio Spectrogram / MelSpectrogram, power 2).
 *     The framed windowed DFT is a strided conv of the reflect-padded waveform with the (cos | -sin) * hann basis and the mel
 *     projection a 1x1 conv with the HTK filterbank: both run on vs_conv_forward (visinger_amd/audio.py builds the two bases).
 *     Between them:  p[b, f, t] = y[b, f, t]^2 + y[b, F + f, t]^2   on the transform output y [B, 2F, T] (rows f real, F + f imaginary),
 *     and for the mel loss on generated audio (tasks/base.py:232-238) its backward  dy[b, f] = 2 y[b, f] dp[b, f],
 *     dy[b, F + f] = 2 y[b, F + f] dp[b, f].                                                                                      */
VS_API int vs_spec_power_fwd(const float *y, float *p, int64_t B, int64_t F, int64_t T, void *stream);
VS_API int vs_spec_power_bwd(const float *y, const float *dp, float *dy, int64_t B, int64_t F, int64_t T, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f3  seeded per-item sampling of the synthesis path.  No reference counterpart for the stream (the reference draws torch.randn_like, whose
 *     values depend on the batch they are drawn in); vs_prior_sample replaces that draw plus the arithmetic of models/visinger.py:107,
 *     z_p = (mu_p + randn_like(mu_p) * exp(logs_p)) * frame_mask, in one launch.
 *     Stream: n(seed, take, c, t) from Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (t, c >> 2, take, 0): the four
 *     outputs give channels 4q .. 4q + 3 of frame t as two Box-Muller pairs (DESIGN.md "Seeded sampling").  A value depends on nothing else:
 *     not on B, the row, the padded T, H or K.  seeds: DEVICE int64 [B], 0 <= seed < 2^63, read by the kernel (a captured graph is replayed
 *     with other seeds by overwriting that buffer).
 *     vs_normal_fill:  out [B * K, H, T], row b * K + k = take take0 + k of item b.
 *     vs_prior_sample: z[b * K + k, c, t] = (mu[b, c, t] + noise_scale * n * exp(logs[b, c, t])) * mask[b, t]; mu / logs: rows of one
 *                      [B, 2H, T] projection output (FramePriorNetwork.proj), batch stride stat_batch_stride in elements, row stride T;
 *                      mask [B, T] or NULL (all ones), a masked frame is exactly 0; eps_out [B * K, H, T] or NULL: receives n, bit-identical
 *                      to vs_normal_fill.
 *     VS_EINVAL before anything is launched: NULL seeds / out / z / mu / logs, B, H, T <= 0, K < 1, take0 < 0, take0 + K > 2^32, T > 2^32,
 *     stat_batch_stride < H * T.  One launch, no allocation, no host synchronisation.                                              */
VS_API int vs_normal_fill(const int64_t *seeds, int64_t take0, int64_t K, float *out, int64_t B, int64_t H, int64_t T, void *stream);
VS_API int vs_prior_sample(const float *mu, const float *logs, int64_t stat_batch_stride, const float *mask, const int64_t *seeds,
                           int64_t take0, int64_t K, float noise_scale, float *z, float *eps_out, int64_t B, int64_t H, int64_t T,
                           void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f4  the pitch curve of synthesis (csrc/pitch_ops.hip): a guide curve in Hz, a transposition in cents, the sung curve back in Hz.
 *     vs_f0_norm_interp: utils/audio/pitch/utils.py:42-57 (norm_interp_f0, one item at a time through numpy there) per row of f0_hz [B, T], on
 *       the first lengths[b] frames (lengths: DEVICE int64 [B], clamped to [0, T]; NULL = T):  uv = 1 where f0_hz == 0, else 0;  f0_norm =
 *       log2f(f0_hz + 1) on voiced frames, the straight line between the two voiced neighbours on an unvoiced frame between them, the first /
 *       last voiced value before / after them (np.interp's edge rule), 0 on a row without a voiced frame.  Frames at or beyond lengths[b]:
 *       f0_norm = 0, uv = 0 (the collate padding) -- they take no part in the interpolation.  A negative, NaN or infinite value counts as
 *       unvoiced (uv = 1; the reference produces NaN there).  A row's result depends on its own frames only (not on B, the row, T).
 *       One workgroup per row, a two-pass chunked scan; f0_norm doubles as the scan's scratch, so the three buffers must be distinct.
 *     vs_pitch_condition: the frame prior's condition, models/visinger.py:129-135, plus the edits, per (b, t):
 *       x = f0_norm[b, t] if given, else pred[b, t, 0];  voiced = (uv[b, t] == 0) if uv is given, else (pred[b, t, 1] <= 0);
 *       if cents != NULL and cents[b] != 0:  x = log2f((exp2f(x) - 1) * exp2f(cents[b] / 1200) + 1)   (a zero shift leaves x's bits alone);
 *       m = mask[b, t] (NULL: 1);  cond = (voiced && m != 0) ? x * m : 0;  f0_hz_out (optional) = clamp(exp2f(x) - 1, 50, 1250) on those
 *       frames (denorm_f0's default range), 0 elsewhere.  pred: dense [B, T, 2], 8-byte aligned.  cents: DEVICE fp32 [B].
 *     VS_EINVAL before anything is launched: NULL f0_hz / f0_norm / uv resp. cond, aliased buffers, B, T <= 0, T >= 2^24 (vs_f0_norm_interp:
 *     frame distances are exact in fp32 below it), pred and f0_norm both NULL, uv and pred both NULL.  One launch each, no allocation, no atomics,
 *     no host synchronisation: a captured graph replays with another curve / other shifts by overwriting the buffers.                  */
VS_API int vs_f0_norm_interp(const float *f0_hz, const int64_t *lengths, float *f0_norm, float *uv, int64_t B, int64_t T, void *stream);
VS_API int vs_pitch_condition(const float *pred, const float *f0_norm, const float *uv, const float *mask, const float *cents, float *cond,
                              float *f0_hz_out, int64_t B, int64_t T, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f5  tempo and duration control of synthesis (csrc/timing_ops.hip): the frame alignment, and a curve on its timeline, retimed on
 *     the device.  Not in the reference (no length regulator; its inference replays the score's timing).  Per item b, tokens i = 1 .. T_tokens:
 *     vs_retime_tokens: d_i = frames of mel2ph[b] equal to i (0 and indices above T_tokens are ignored, as in vs_mel2token_to_dur), or dur[b, i-1]
 *       clamped to [0, 2^24) -- exactly one of mel2ph [B, T_frames] / dur [B, T_tokens] is given;  c_i = d_1 + .. + d_i.
 *       f = stretch[b, i-1] / tempo[b] (one fp32 division; NULL stretch / tempo = 1), a non-finite f becomes 1, then f is clamped to [2^-6, 2^6];
 *       s_i = (int64) rintf(f * 65536);  P_i = sum_{j<=i} d_j s_j;  R_i = (P_i + 32768) >> 16;  m_i = d_i > 0 ? min_frames : 0;
 *       e_0 = 0, e_i = max(e_{i-1} + m_i, R_i): cumulative rounding with a floor -- with min_frames = 1 a token that had frames keeps one, an
 *       empty token stays empty, all factors 1 give e = c.  cum_old = c, cum_new = e (int64 [B, T_tokens]), lengths[b] = e_T, or
 *       min(e_T, max_frames) with max_frames > 0 (0 = no capacity).  mel2ph must be monotonic over its valid prefix (not checked).
 *       One workgroup per item: integer LDS histogram, then a chunked int64 scan (the recurrence in its closed form M_i + max(0, max_{j<=i}(R_j - M_j)),
 *       M the prefix sum of m); bit-reproducible, independent of the launch shape.  stretch, tempo, lengths: DEVICE buffers, read by the kernel.
 *     vs_retime_frames: for t < min(lengths[b], T_out): mel2ph_out[b, t] = the smallest i with e_i > t (upper bound in the row of cum_new); 0 beyond.
 *       curve (optional, fp32 [B, curve_T] on the OLD timeline, <= 0 = unvoiced) -> curve_out [B, T_out]: for frame t of token i, u = t - e_{i-1},
 *       n = d_i, n' = e_i - e_{i-1}:  num = (2u + 1) n - n', den = 2 n';  num < 0: k = 0, w = 0, else k = num / den, w = float(num - k den) / float(den);
 *       k >= n - 1: k = n - 1, w = 0;  a = curve[c_{i-1} + k], b = curve[c_{i-1} + min(k + 1, n - 1)];  both > 0: a + w (b - a), else a if w < 0.5 else b
 *       (an unvoiced frame is never blended; w = 0 copies a's bits; no read across a token boundary; an index outside [0, curve_T) reads as 0).
 *       0 beyond lengths[b].  One lane per new frame.
 *     VS_EINVAL before anything is launched: both or neither of mel2ph / dur, NULL outputs, aliased dur / cum_old / cum_new, B, T_tokens, T_out <= 0,
 *     T_tokens > 8192 (the LDS histogram), T_frames outside [1, 2^24) with mel2ph, min_frames outside [0, 65536], max_frames < 0, curve without
 *     curve_out or the reverse, curve_T <= 0 with a curve, T_out >= 2^31.  No allocation, no host synchronisation: a captured graph replays under
 *     another tempo / stretch by overwriting those buffers, inside the capacity max_frames = T_out.                                      */
VS_API int vs_retime_tokens(const int64_t *mel2ph, const int64_t *dur, const float *stretch, const float *tempo, int64_t min_frames,
                            int64_t max_frames, int64_t *cum_old, int64_t *cum_new, int64_t *lengths, int64_t B, int64_t T_frames,
                            int64_t T_tokens, void *stream);
VS_API int vs_retime_frames(const int64_t *cum_old, const int64_t *cum_new, const int64_t *lengths, const float *curve, int64_t curve_T,
                            int64_t *mel2ph_out, float *curve_out, int64_t B, int64_t T_tokens, int64_t T_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f6  pitch tracking (csrc/pitch_track.hip): the per-frame f0 curve of a batch of recordings, in the convention of f4 / f5 (Hz, 0 = unvoiced,
 *     one value per hop).  Not in the reference (its extractors are parselmouth / pyworld on the host).  YIN (de Cheveigne & Kawahara 2002) with a LAG-CENTRED
 *     difference function.  wav: fp32 [B, L]; lengths: DEVICE int64 [B] (clamped to [0, L]) or NULL = L; f0_hz, periodicity (or NULL): fp32 [B, T], T the caller's.
 *       tau_max = ceil(sr / f0_min), tau_min = max(2, floor(sr / f0_max)) (in double), W = window, or 2 tau_max when window = 0;
 *       n_b = min(lengths[b] / hop, T); frames t >= n_b: f0 = periodicity = 0; a sample at or beyond lengths[b], or before 0, reads as 0.
 *     Frame t < n_b, c = t hop + hop / 2 (integer divisions throughout):
 *       1. d(tau) = sum_{j = 0 .. W-1} (x[s + j] - x[s + j + tau])^2,  s = c - W/2 - tau/2,  tau = 1 .. tau_max + 1  (the direct form, never energy - 2 acf);
 *       2. S(tau) = d(1) + .. + d(tau);  d'(tau) = d(tau) tau / S(tau) where 0 < S(tau) < inf, else 1 (a NaN or infinite sample in a lag's span: d' = 1 there);
 *       3. g = argmin of d' over [tau_min, tau_max], the lowest tau on a tie;  periodicity = clamp(1 - d'(g), 0, 1);
 *       4. e = sum_{j < W} x[c - W/2 + j]^2.  e not finite: f0 = 0 and periodicity = 0.  e <= silence * W (one fp32 product): f0 = 0.  Otherwise p = the first tau in
 *          [tau_min, tau_max] with d'(tau) < threshold, then p <- p + 1 while p + 1 <= tau_max and d'(p + 1) < d'(p); no such tau: f0 = 0;
 *       5. y0, y1, y2 = d'(p - 1), d'(p), d'(p + 1);  den = y0 - 2 y1 + y2;  off = den > 0 ? clamp(0.5 (y0 - y2) / den, -0.5, 0.5) : 0;  f0 = sr / (p + off).
 *     fp32 throughout, in an order fixed per frame and lag -- a frame's outputs depend on the samples of its own span only, not on B, the row, L, T, the padding
 *     or how many frames a workgroup takes:
 *       d(tau) = ((B_0 + B_1) + B_2) + ..., B_k = the chain acc = fmaf(v, v, acc) from 0 over j = 32k .. min(32k + 31, W - 1) ascending, v = the rounded difference;
 *       S(tau) = E_l + P, l = (tau - 1) / 17, P = d(17 l + 1) + .. + d(tau) ascending from 0, E_l = the sum of the chunk totals below l, formed over 64 chunks by
 *                the doubling scan v_l += v_{l - s}, s = 1, 2, 4, .. 32 (chunks beyond tau_max + 1 count 0) and taken from chunk l - 1 (E_0 = 0);
 *       e: partial l = the fmaf chain over j = l, l + 64, .. ascending, l < 64, then the butterfly e_l += e_{l ^ s}, s = 32, 16, .. 1;
 *       d' = (d * float(tau)) / S, off and f0 as written, IEEE fp32 operations.
 *     VS_EINVAL before anything is launched: NULL wav / f0_hz, aliased buffers, B, L, T <= 0, L >= 2^31 (or T), hop < 1, sr < 1, f0_min / f0_max / threshold not
 *     finite and > 0, f0_min >= f0_max, tau_max > 1024, tau_min >= tau_max, W outside [tau_max, 2048], silence < 0 (or NaN).  One launch, no allocation, no atomics,
 *     no host synchronisation; wav and lengths are read on the device: a captured graph replays on another recording by overwriting them.                    */
VS_API int vs_f0_yin(const float *wav, const int64_t *lengths, int64_t B, int64_t L, int sr, int hop, float f0_min, float f0_max, int window,
                     float threshold, float silence, float *f0_hz, float *periodicity, int64_t T, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f7  guide alignment (csrc/guide_align.hip): the score timed to a recording -- which frames of a guide curve (f6's output, on its OWN timeline)
 *     belong to which token, as new frames-per-token that vs_retime_tokens(dur =) turns into an alignment.  Not in the reference (its inference replays the score's
 *     timing; alignment is an offline host tool).  A monotonic Viterbi alignment; integer once the two inputs are quantised, so it is reproducible bit for bit.
 *     Per item b:  f0_hz fp32 [B, Tg];  g_len DEVICE int64 [B] or NULL (= Tg), clamped to [0, Tg]: G;  note_midi fp32 [B, T_ph]: the score pitch of each token as
 *     a MIDI number (fractions allowed), not finite or <= 0 = a rest (rests and padding);  dur int64 [B, T_ph]: score frames per token, read clamped to [0, 2^24);
 *     offset_cents DEVICE fp32 [B] or NULL (0): the guide's transposition against the score.  Outputs, every element written: dur_new int64 [B, T_ph],
 *     cost int32 [B], status int32 [B].
 *       Quantisation (unit: 1/16 semitone).  Frame t is voiced when f0 is finite and > 0; then q_t = (int) rintf(x) + 1104, x = 192 log2f(f0 / 440) (the accurate
 *       log2f, one fp32 division, one fp32 product) clamped to [-40000, 40000].  Pitched token: m_i = (int) rintf(min(16 note_midi, 2^20)).
 *       off = (int) rintf(clamp(offset_cents * 0.16f, -2^20, 2^20)), 0 for a non-finite offset.
 *       Active tokens: those with dur > 0, in order; S their count, d_s their durations, a_s the exclusive prefix sum of d, L = sum d.
 *       S == 0 or G < S:  status = 1, dur_new = max(dur, 0) (as given, not clamped above), cost = -1.  Otherwise status = 0 and:
 *       Local cost c(t, s) = pitch term + drift term.
 *         pitch: voiced frame, pitched token: delta = abs(q_t - m_s - off); with octave_fold: delta %= 192, delta = min(delta, 192 - delta); min(delta, cap);
 *                voiced, rest: w_voiced_rest;  unvoiced, pitched: w_unvoiced_note;  unvoiced, rest: 0.
 *         drift: u_t = floor(t L / G) (int64);  gap = max(0, a_s - u_t, u_t - (a_s + d_s - 1));  min((gap drift) >> 8, drift_cap).
 *       Recurrence, int32, INF = 2^30 - 1:  D(0, 0) = c(0, 0), D(0, s > 0) = INF;  for t >= 1: adv(t, s) = s > 0 && D(t-1, s-1) < D(t-1, s) (a tie stays),
 *         D(t, s) = min(INF, c(t, s) + (adv ? D(t-1, s-1) : D(t-1, s)));  cost = D(G-1, S-1).
 *       Backtrack: s = S-1; for t = G-1 .. 1: if adv(t, s): start[s] = t, s -= 1.  start[0] = 0, start[S] = G, n_s = start[s+1] - start[s] (>= 1).
 *       Runs (pitch cannot separate a consonant from the vowel of its note): a run is a maximal stretch of consecutive active tokens that are all rests, or all
 *         pitched with equal m.  In a run of k tokens with n = sum n_s, D_r = sum d_s and cumulative C_i (i = 1 .. k), int64, floor division:
 *         E_0 = 0;  R_i = min((2 C_i n + D_r) / (2 D_r), n - (k - i));  E_i = max(E_{i-1} + 1, R_i);  token i of the run gets E_i - E_{i-1} (E_k = n, each >= 1).
 *       Inactive tokens get 0: sum dur_new[b] = G.
 *     Weights: cap, w_voiced_rest, w_unvoiced_note, drift, drift_cap in [0, 4096] (defaults 64, 48, 24, 32, 64), octave_fold 0 / 1, reserved = 0.
 *     One workgroup per item, one launch: sequential over the frames, one column of D per lane, the neighbour by a lane shift and across waves through LDS (one
 *     barrier a frame, none when S <= 64).  Backpointers are one bit per (t, s), a wave's ballot per 64 columns: in LDS when G ceil(S / 64) <=
 *     VS_GUIDE_ALIGN_LDS_WORDS, else in `workspace`, laid out [B, Tg, ceil(T_ph / 64)] 64-bit words and written by plain stores.  The workspace (8-byte aligned,
 *     workspace_bytes >= B Tg ceil(T_ph / 64) 8) is REQUIRED when Tg ceil(T_ph / 64) > VS_GUIDE_ALIGN_LDS_WORDS and not looked at otherwise.
 *     An item's outputs depend on its own row's first G frames and T_ph tokens only.
 *     VS_EINVAL before anything is launched: NULL f0_hz / note_midi / dur / dur_new / cost / status, aliased buffers, B < 1, T_ph outside [1, 1024], Tg outside
 *     [1, 65536], a weight outside [0, 4096], octave_fold not 0 / 1, reserved != 0, a required workspace that is NULL, misaligned or too small.  No allocation,
 *     no atomics, no host synchronisation; f0_hz, g_len, note_midi, dur, offset_cents are read on the device: a captured graph replays on another guide by
 *     overwriting them.                                                                                                                                  */
#define VS_GUIDE_ALIGN_LDS_WORDS 5120
VS_API int vs_guide_align(const float *f0_hz, const int64_t *g_len, const float *note_midi, const int64_t *dur, const float *offset_cents, int cap,
                          int w_voiced_rest, int w_unvoiced_note, int drift, int drift_cap, int octave_fold, int reserved, int64_t *dur_new, int32_t *cost,
                          int32_t *status, void *workspace, size_t workspace_bytes, int64_t B, int64_t Tg, int64_t T_ph, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f8  guide pitch correction (csrc/guide_correct.hip): a tracked guide curve pulled onto the score it was sung to -- the slow part of its
 *     deviation from the note (a flat note, drift) is taken out, the fast part (vibrato, scoops, jitter) is kept or scaled.  Not in the reference (its pitch
 *     tools are offline host programs).  Integer once the inputs are quantised, so it is reproducible bit for bit.  The conventions are f7's.
 *     Per item b:  f0_hz fp32 [B, T], on the item's own frames;  mel2ph int64 [B, T]: 1-based token ids, 0 = padding;  note_midi fp32 [B, T_ph]: not finite or
 *     <= 0 = a rest;  lengths DEVICE int64 [B] or NULL (= T), clamped to [0, T]: n;  offset_cents DEVICE fp32 [B] or NULL (0): the guide's transposition against
 *     the score.  Host parameters: window W in [0, 1024] frames, strength_q a in [0, 256], vibrato_q in [0, 512] with b = 256 - vibrato_q, wild in [0, 2^18]
 *     units, octave_fold 0 / 1, reserved = 0.
 *       Quantisation (unit: 1/16 cent -- 19200 an octave, 1600 a semitone).  Frame t is voiced when f0 is finite and > 0; then
 *       q_t = (int) rintf(clamp(19200 log2f(f0 / 440), -2^22, 2^22)) (the accurate log2f, one fp32 division, one fp32 product).  Frame t has the token mel2ph[t]
 *       when that lies in [1, T_ph], else none.  Pitched token: m = (int) rintf(clamp(1600 (note_midi - 69), -2^22, 2^22)) (one fp32 difference, one fp32
 *       product).  off = (int) rintf(clamp(16 offset_cents, -2^22, 2^22)), 0 for a non-finite offset.
 *       Deviation.  d_t = q_t - m_t - off;  with octave_fold: d_t -= 19200 floor((d_t + 9600) / 19200).  Frame t < n is CORRECTABLE when it is voiced, its token
 *       is pitched and |d_t| <= wild.
 *       Segments.  A segment is a maximal stretch of consecutive frames t < n whose tokens are pitched with equal m (f7's run: consonant and vowel of a note,
 *       two equal notes in a row).  Unvoiced or wild frames inside a segment do not split it; they do not count.
 *       Slow part.  For a correctable t: S_t = the sum of d_u and N_t the count over the correctable u of t's segment with |u - t| <= W (N_t >= 1);
 *       s_t = floor((2 S_t + N_t) / (2 N_t));  v_t = d_t - s_t.
 *       Correction.  k_t = floor((a s_t + b v_t + 128) / 256);  f0_out = f0 exp2f((float)(-k_t) / 19200.0f) (one fp32 division, the accurate exp2f, one fp32
 *       product).  Where k_t == 0, and on every frame that is not correctable -- t >= n, NaNs and negative values included -- f0_out is the bits of f0_hz and
 *       k_out is 0.  (a = 256, b = 0: the windowed mean of every note moves onto the score and what is faster stays;  a = 0, b = 0: the identity, bit for bit;
 *       b = 256: flattened;  b = -256: the fast part doubled.)
 *       With wild <= 2^18 and W <= 1024 every intermediate fits int32: |d| <= 2^18, |S| <= 2049 2^18, |2 S + N| < 2^31, |a s| <= 2^26, |b v| <= 2^27.
 *     vs_guide_correct: f0_out fp32 [B, T], k_out int32 [B, T] or NULL; every element of both is written.  One launch: grid (tiles of VS_GUIDE_CORRECT_TILE
 *     frames, B); a workgroup stages its tile plus a halo of W frames on both sides (d, the flags, m -- note_midi gathered through mel2ph) into LDS, forms the
 *     prefix sums of d and of the flags, the prefix max of the segment starts and the suffix min of the segment ends in one workgroup scan, and takes S_t, N_t as
 *     differences at the clipped window's ends (a boundary farther than W away never matters: the halo is enough).  16-byte loads and stores when T % 4 == 0 and
 *     f0_hz, mel2ph, f0_out, k_out are 16-byte aligned.
 *     vs_guide_deviation: per item n_corr = the number of correctable frames and dev_med = the LOWER median of d_t over them -- the element at index
 *     (n_corr - 1) / 2 of the sorted values -- or 0 when there are none (int32 [B] each).  With offset_cents = NULL and a large wild, dev_med / 16 is the guide's
 *     transposition against the score in cents.  One workgroup per item: a bisection on the value over [-wild, wild], each step one count over the item's frames.
 *     A row's outputs depend on its own first n frames and its T_ph tokens only.
 *     VS_EINVAL before anything is launched, the outputs untouched: a NULL f0_hz / mel2ph / note_midi / f0_out (dev_med / n_corr), an output that overlaps an
 *     input or the other output, B < 1, T outside [1, 65536], T_ph outside [1, 1024], a parameter out of its range, reserved != 0.  No allocation, no atomics,
 *     no host synchronisation; f0_hz, lengths, mel2ph, note_midi, offset_cents are read on the device: a captured graph replays on another guide by overwriting
 *     them.                                                                                                                                               */
#define VS_GUIDE_CORRECT_TILE 1024
VS_API int vs_guide_correct(const float *f0_hz, const int64_t *lengths, const int64_t *mel2ph, const float *note_midi, const float *offset_cents, int window,
                            int strength_q, int vibrato_q, int wild, int octave_fold, int reserved, float *f0_out, int32_t *k_out, int64_t B, int64_t T,
                            int64_t T_ph, void *stream);
VS_API int vs_guide_deviation(const float *f0_hz, const int64_t *lengths, const int64_t *mel2ph, const float *note_midi, const float *offset_cents, int wild,
                              int octave_fold, int32_t *dev_med, int32_t *n_corr, int64_t B, int64_t T, int64_t T_ph, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f9  sample-rate conversion (csrc/resample.hip): a rational polyphase converter -- recordings at another rate in (f6 tracks them at the
 *     model's), waveforms at another rate out.  Not in the reference (it resamples on the host through librosa).
 *     Inputs: integers sr_in, sr_out >= 1, g = gcd(sr_in, sr_out); quality: zeros (integer >= 1, default 32), beta (> 0, default 10.0), rolloff (in (0, 1],
 *     default 0.90).  L = sr_out / g, M = sr_in / g, S = max(L, M), W = zeros S, fc = rolloff / (2 S).
 *       Prototype, for integer m with |m| <= W, zero elsewhere:  h(m) = L 2 fc sinc(2 fc m) I0(beta sqrt(1 - (m / W)^2)) / I0(beta),  sinc(x) = sin(pi x) / (pi x);
 *       evaluated in fp64 ON THE HOST and rounded once to fp32: the device only ever sees the fp32 table, which is part of the input, not of the arithmetic.
 *       Output: row b has len_b = lengths[b] clamped to [0, n_in] samples and out_len_b = ceil(len_b L / M).  For 0 <= n < min(out_len_b, n_out):
 *         y[b, n] = sum x[b, i] h(n M - i L) over every i with 0 <= i < len_b and |n M - i L| <= W;   y[b, n] = 0 for the other n < n_out.
 *       A sample at or beyond len_b is never read into a result.  out_lengths[b] (optional) = out_len_b, not cut at n_out.
 *     Table (the caller builds it; visinger_amd/resample.py design()): fp32 [L][P], 16-byte aligned, P = 2 C + 1, C = ceil(W / L).  Row rho holds the phase
 *       p = (rho M) mod L -- the phase of every output n with n mod L = rho, so consecutive outputs read consecutive rows -- and table[rho][j] = h((C - j) L + p).
 *       With n M = q L + p the output is the sum over j = 0 .. P - 1 of x[q - C + j] table[n mod L][j] (x = 0 outside [0, len_b)).
 *       Tile: 4 G outputs, G = L max(1, floor((256 + L / 2) / L)) (a whole number of table periods, about 256): vs_resample_tile(L).
 *       Budget: L P 4 <= VS_RESAMPLE_TABLE_BYTES, and the table plus one tile's input span -- (3 + floor((4 G - 1) M / L) + P + 4) & ~3 floats -- within
 *       VS_RESAMPLE_LDS_BYTES; M <= VS_RESAMPLE_MAX_M.  vs_resample_fits answers 1 / 0 for (L, M, P).  At the default quality 24000 <-> 48000,
 *       24000 <-> 44100, 16000 -> 24000, 22050 -> 24000 and 32000 -> 24000 fit (tables of at most 41600 bytes); 44100 -> 8000 does not.
 *     Device arithmetic: products and sums in fp32.  One output is ONE chain acc = fmaf(x[q - C + j], table[n mod L][j], acc) from acc = 0 over j = 0 .. P - 1
 *       ascending (ascending i); terms outside [0, len_b) or outside the prototype enter as products with an exact 0 (so a NaN or infinity at distance up to C
 *       samples reaches an output, not only one within W / L).  The order does not depend on B, the row, the padding, n_in, n_out or the launch shape: two
 *       calls that give an output the same samples give it the same bits.  All index arithmetic that involves n M is 64-bit.
 *     One launch: a workgroup loads the table into LDS once and walks tiles of its row, staging each tile's input span with 16-byte loads (when x is
 *     16-byte aligned and n_in % 4 == 0); a lane takes the four outputs n0 + c + r G of a tile, which share a table row.  Every element of y is written.
 *     VS_EINVAL before anything is launched: NULL x / table / y, aliased buffers, B, n_in, n_out <= 0 or n_in, n_out >= 2^40, L or M < 1, M > VS_RESAMPLE_MAX_M,
 *     P even or < 3, a table over its budget, table and span over the LDS budget, a misaligned table.  No allocation, no atomics, no host synchronisation;
 *     x and lengths are read on the device and out_lengths is written there: a captured graph replays on other samples and lengths by overwriting them.   */
#define VS_RESAMPLE_TABLE_BYTES 49152
#define VS_RESAMPLE_LDS_BYTES 65536
#define VS_RESAMPLE_MAX_M 1048576
VS_API int64_t vs_resample_tile(int L);
VS_API int vs_resample_fits(int L, int M, int P);
VS_API int vs_resample_poly(const float *x, const int64_t *lengths, int64_t B, int64_t n_in, const float *table, int L, int M, int P, float *y,
                            int64_t n_out, int64_t *out_lengths, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f10 guide dynamics (csrc/dynamics.hip): the loudness contour of a recording tracked per frame, compared with the synthesised waveform's own
 *     and applied to it as a smoothed, limited gain.  Not in the reference (the model has no energy condition).  The conventions are f7's / f8's.
 *     Level unit: 1/256 of a doubling of POWER (about 0.01176 dB): 256 units double the power, 512 the amplitude.  Host parameters in dB become units on the
 *     host as rint(dB 256 / (10 log10 2)), in double.  A level curve is fp32 mean-square power per frame; a value that is not finite or <= 0 means "no level
 *     there" -- the <= 0 convention of vs_retime_frames' curve, which therefore warps a level curve as it is.
 *     vs_level_track: wav fp32 [B, L];  lengths DEVICE int64 [B], clamped to [0, L], or NULL (= L);  level fp32 [B, T], every element written.
 *       n_b = min(len_b / hop, T).  Block u is the samples u hop .. u hop + hop - 1.  Block energy E_u, fp32, in a fixed order: partial l (l = 0 .. 63) is the
 *       chain acc = fmaf(v, v, acc) from 0 over the block's samples j with (j / 4) mod 64 == l, j ascending; then the butterfly e_l += e_{l ^ s}, s = 32, 16,
 *       .. 1 (the order a wave gets from one 16-byte load per lane and 256 samples; the 4-byte path, taken where the row is not 16-byte aligned or
 *       hop % 4 != 0, produces the same bits).  Frame level, t < n_b: s = the sum of E_u over u = max(0, t - half) .. min(n_b - 1, t + half), ascending from 0;
 *       cnt = the number of those blocks;  p = s / (float)(cnt hop), one IEEE division;  p = 0 where s is not finite, and for t >= n_b.  A sample at or
 *       beyond n_b hop is never read into a result.  A row's output depends on its own samples only: not on B, the row, L, T, the padding or the launch shape.
 *       One launch: grid (tiles of 64 frames, B); a workgroup computes the E_u of its tile plus `half` blocks on both sides into LDS, then the frame sums.
 *       VS_EINVAL: NULL wav / level, level overlapping an input, B, L, T <= 0, L or T >= 2^31, hop outside [1, 4096], half outside [0, 8].
 *     Quantisation (vs_level_offset, vs_level_gain).  A frame has a level when p is finite and > 0; then q = (int) rintf(clamp(256 log2f(p), -2^16, 2^16)) (the
 *       accurate log2f, one fp32 product).  lengths DEVICE int64 [B] or NULL (= T), clamped to [0, T]: n.  Frame t < n is ACTIVE when the guide and the own
 *       curve both have a level there and both q >= gate.  d_t = qg_t - qo_t.
 *     vs_level_offset: guide, own fp32 [B, T];  n_act = the item's number of active frames;  off = floor((2 sum d_t + n_act) / (2 n_act)) over them (int64
 *       sum), 0 when there are none;  both int32 [B].  One workgroup per item, as in vs_guide_deviation.
 *     vs_level_gain: offset DEVICE int32 [B] or NULL (0), read clamped to [-2^17, 2^17];  e_t = d_t - offset_b on active frames.  For t < n: S_t = the sum of e_u
 *       and N_t the count over the active u < n with |u - t| <= window.  Where N_t >= 1: m_t = floor((2 S_t + N_t) / (2 N_t)) and
 *       k_t = clamp(floor((depth_q m_t + 128) / 256), -down, up);  elsewhere, t >= n included, k_t = 0.  k_out int32 [B, T], every element written.  (A frame
 *       below the gate -- an unvoiced consonant, a breath -- takes the gain of its neighbours; a row whose guide curve is all 0 gets k = 0 throughout.)
 *       Ranges: T in [1, 65536] (vs_level_offset too), window in [0, 1024], depth_q in [0, 256], up and down in [0, 4096], gate in [-2^16, 2^16], reserved = 0.
 *       With these every intermediate fits int32: |q| <= 2^16, |d| <= 2^17, |e| <= 2^18, |S| <= 2049 2^18, |2 S + N| < 2^31, |m| <= 2^18, |depth_q m| <= 2^26.
 *       One launch: grid (tiles of VS_LEVEL_GAIN_TILE frames, B); the tile plus a halo of `window` frames on both sides is staged in LDS and S, N are
 *       differences of one workgroup prefix sum, as in vs_guide_correct.  16-byte loads and stores when T % 4 == 0 and guide, own, k_out are 16-byte aligned.
 *     vs_level_apply: x, y fp32 [B, L];  k int32 [B, T];  lengths in SAMPLES, DEVICE int64 [B], clamped to [0, L], or NULL (= L);  n = min(len_b / hop, T);  y is x
 *       exactly (in place) or does not overlap it.  For sample i < n hop, in integers (64-bit where i is involved): a = 2 i + 1 - hop;  t0 = floor(a / (2 hop))
 *       (may be -1);  w = a - 2 hop t0, in [0, 2 hop);  ka = k[clamp(t0, 0, n - 1)], kb = k[clamp(t0 + 1, 0, n - 1)], both read clamped to [-4096, 4096];
 *       kappa = ka (2 hop - w) + kb w (|kappa| <= 2^25 with hop <= 2048: (float) kappa is exact);  y = x exp2f((float) kappa / (float)(1024 hop)): one fp32
 *       division, the accurate exp2f, one fp32 product.  The gain is linear in level between frame centres and held before the first and after the last one.
 *       Where kappa == 0, and for every i >= n hop, y is the bits of x, NaNs included.  One launch, 4 samples a lane: 16-byte loads and stores where
 *       L % 4 == 0 and x, y are 16-byte aligned.  VS_EINVAL: NULL x / k / y, y overlapping x partly, k or lengths, B, L, T <= 0, L or T >= 2^31, hop outside
 *       [1, 2048].
 *     All four: VS_EINVAL before anything is launched, the outputs untouched (also: NULL or overlapping buffers, a parameter out of its range).  No allocation,
 *     no atomics, no host synchronisation; every per-item input is read on the device: a captured graph replays on other data by overwriting it.        */
#define VS_LEVEL_GAIN_TILE 1024
VS_API int vs_level_track(const float *wav, const int64_t *lengths, int64_t B, int64_t L, int hop, int half, float *level, int64_t T, void *stream);
VS_API int vs_level_offset(const float *guide, const float *own, const int64_t *lengths, int gate, int32_t *off, int32_t *n_act, int64_t B, int64_t T,
                           void *stream);
VS_API int vs_level_gain(const float *guide, const float *own, const int64_t *lengths, const int32_t *offset, int gate, int window, int depth_q, int up,
                         int down, int reserved, int32_t *k_out, int64_t B, int64_t T, void *stream);
VS_API int vs_level_apply(const float *x, const int32_t *k, const int64_t *lengths, int hop, float *y, int64_t B, int64_t L, int64_t T, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f11 peak limiter (csrc/limiter.hip): a look-ahead sample-peak limiter for a batch of ragged waveforms -- the ceiling behind f10's boost and
 *     f9's overshoot.  Not in the reference (it peak-normalises on the host).  The gain is computed in integers and the ceiling is a hard guarantee.
 *     Unit: f10's, seen from the amplitude: 1/512 of a doubling of AMPLITUDE (= 1/256 of a doubling of power), so a reduction composes with vs_level_apply's gain.
 *     vs_peak_limit: x, y fp32 [B, L];  lengths DEVICE int64 [B], clamped to [0, L], or NULL (= L): n;  c fp32, the ceiling, finite, 0 < c <= 1 (the host makes
 *       it from ceiling_db <= 0 as 10^(dB / 20) in double, rounded once to fp32);  window W in [0, VS_PEAK_LIMIT_MAX_WINDOW] samples;  tab DEVICE int32
 *       [VS_PEAK_LIMIT_TABLE]: tab[j] = ceil(512 log2(1 + (j + 1) / 512)), built on the host in double (the device takes no logarithm): part of the input.
 *       Per sample i of row b:
 *       1. Need.  u_i = 0 where i >= n or where |x_i| > c is false (a NaN needs nothing).  Otherwise rho = |x_i| / c, the correctly rounded fp32 quotient
 *          (>= 1; infinite for an infinite sample or on overflow), e = rho's unbiased exponent (its bits >> 23, less 127), m = its 23 mantissa bits, and
 *          u_i = min(512 e + tab[m >> 14], VS_PEAK_LIMIT_U_MAX) (12288 units = 24 doublings; what an infinity gets: e = 128).  An upper bound by construction:
 *          2^(u_i / 512) >= |x_i| / c, at most about 2.3 units (0.027 dB) over the exact need.
 *       2. Hold.  M_j = the largest u_i over |i - j| <= W, cut at [0, n).
 *       3. Smooth.  g_i = ceil(S_i / N_i) = (S_i + N_i - 1) / N_i in integers, S_i = the sum of M_j over |j - i| <= W cut at [0, n), N_i the number of its terms;
 *          g_i = 0 for i >= n.  Every M_j of that sum has i in its own window, so g_i >= u_i: the ramp in front of a peak never lets the peak through.  A lone
 *          peak gets a triangle of half-width 2 W in the log domain; peaks closer than 2 W + 1 share a plateau.  Everything fits int32: S <= 2049 * 12288.
 *       4. Apply.  y_i is the bits of x_i where g_i = 0 and everywhere beyond n (a NaN within the row comes back as it is only there: within 2 W of an
 *          over-ceiling sample it goes through the product and stays a NaN, its payload not promised).  Otherwise y_i = x_i exp2f(-(float) g_i / 512.0f) -- the
 *          exponent is exact in fp32, the accurate exp2f, one fp32 product -- and then the guard: where |y_i| > c, y_i = copysignf(c, y_i) (exp2f and the product
 *          round; it also brings an infinity to +-c).  After the call |y_i| <= c holds exactly for every i < n that is not a NaN.
 *       5. gain int32 [B, L] or NULL: g, every element written when given.  stats int32 [B, 3] or NULL: the number of samples with u_i > 0, the largest g_i,
 *          the number of samples the guard moved; accumulated with integer vector atomics (order-independent: deterministic); the entry clears it on the
 *          stream before the launch.
 *       W = 0 is a per-sample soft clip onto c.  A row with nothing over c comes back bit for bit.  Sample peaks only: inter-sample (true) peaks are not seen.
 *       A row's result depends on its own samples only: not on B, the row, L, the padding or the launch shape.
 *       One launch: grid (tiles of VS_PEAK_LIMIT_TILE samples, B), one workgroup per tile; the tile plus 2 W samples on both sides is staged in LDS as u (16-byte
 *       loads where L % 4 == 0 and x, y, gain are 16-byte aligned, 4-byte loads otherwise: the same bits), the hold is a log-step doubling maximum, the sum a
 *       difference of one workgroup prefix scan.  A tile that stages no u > 0 copies x's bits.  y == x exactly (in place) is allowed: a tile's halo is then its
 *       neighbour's output, so ONE workgroup per row walks the tiles in order and carries the left halo's u in LDS (the same bits, B workgroups wide), and tiles
 *       without a reduction write nothing.
 *       VS_EINVAL before anything is launched, the outputs untouched: NULL x / y / tab, c not in (0, 1], window outside [0, 1024], B or L < 1, L >= 2^31, y
 *       overlapping x partly, an output overlapping another buffer.  No allocation, no host synchronisation; x, lengths and tab are read on the device: a
 *       captured graph replays on other data by overwriting them.                                                                                       */
#define VS_PEAK_LIMIT_TILE 4096
#define VS_PEAK_LIMIT_MAX_WINDOW 1024
#define VS_PEAK_LIMIT_TABLE 512
#define VS_PEAK_LIMIT_U_MAX 12288
VS_API int vs_peak_limit(const float *x, const int64_t *lengths, const int32_t *tab, float c, int window, float *y, int32_t *gain, int32_t *stats, int64_t B,
                         int64_t L, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f12 pitch tracking as a path (csrc/pitch_track.hip: vs_f0_candidates, csrc/pitch_path.hip: vs_f0_path): f6 decides every frame on its own,
 *     so a weak fundamental costs a few frames an octave up and a d' near the threshold makes the voicing flicker.  Here a frame keeps SEVERAL lag candidates and
 *     a Viterbi path over the phrase chooses among them (the pYIN / "Tony" construction, in integers).  Not in the reference.  vs_f0_yin is unchanged.
 *     vs_f0_candidates.  wav, lengths, B, L, sr, hop, f0_min, f0_max, window, silence, T as in f6; gate in place of threshold.  Outputs cand_hz, cand_d: fp32
 *     [B, T, 8], EVERY element written.  Steps 1 - 2 of f6 and the energy e of step 4 run unchanged, in f6's summation order: the d' row of a frame holds the same
 *     bits as in vs_f0_yin.  A frame t < n_b with e finite and e > silence * W has as candidates the lags tau in [tau_min, tau_max], ascending, with
 *       (tau == tau_min or d'(tau - 1) > d'(tau))  and  d'(tau) <= d'(tau + 1)  and  d'(tau) < gate;
 *     the first 7 fill slots 0 .. 6: cand_hz = sr / (tau + off) by f6 step 5 (p = tau), cand_d = d'(tau).  Every other slot holds hz = 0, d = 1: slot 7 (the
 *     unvoiced state's) always, every slot of a silent or non-finite frame and of a frame t >= n_b.
 *     VS_EINVAL as in f6, with gate finite and > 0 in place of threshold (and B T 8 in range).  One launch, no allocation, no atomics, no host synchronisation.
 *     vs_f0_path.  cand_hz, cand_d: fp32 [B, T, 8] (slot 7 is not read);  n_frames: DEVICE int64 [B] or NULL (= T), clamped to [0, T]: N;  outputs f0_hz fp32
 *     [B, T], state int32 [B, T] or NULL, cost int32 [B] or NULL.  States 0 .. 6 are the candidate slots, state 7 is "unvoiced".  Integer once quantised:
 *       present(t, k): cand_hz finite and > 0.   q(t, k): f7's frame quantiser of cand_hz (unit: 1/16 semitone), the same code.
 *       loc(t, k) = min((int) rintf(1024 clamp(cand_d, 0, 1)), 1024) + w_order k for a present slot (a NaN d counts as 1); an absent slot: 16384.
 *       loc(t, 7) = w_unvoiced.
 *       trans(i -> j) at frame t: 0 when both are unvoiced;  w_switch when exactly one is;  0 when both are voiced and one of them is absent;
 *                                 otherwise min((abs(q(t-1, i) - q(t, j)) w_jump) >> 4, jump_cap).
 *       D(0, s) = loc(0, s);  D(t, j) = loc(t, j) + min_i (D(t-1, i) + trans(i -> j)), the lowest i on a tie (the backpointer).
 *       The end state is the lowest argmin of D(N-1, .), cost that value; then backtrack.  f0_hz[t] = cand_hz[t, s] when s < 7 and the slot is present, else 0;
 *       state[t] = s.  Frames t >= N: f0_hz = 0, state = -1.  N = 0: cost = 0.
 *     Weights w_unvoiced, w_switch, w_order, w_jump, jump_cap in [0, 4096] (defaults 160, 96, 24, 32, 384; gate 0.5), reserved = 0, T in [1, 32768].  The worst
 *     total is 32768 (1024 + 6 * 4096 + 4096) = 973 078 528 < 2^31: int32 holds every D without saturation.
 *     One wave per item, one launch, sequential over the frames (as f7 is): lane (j, i) forms D(t-1, i) + trans, three xor steps take the minimum.  Backpointers
 *     are 8 x 3 bits in one dword a frame, in 4 T bytes of dynamic LDS (up to 128 KiB); no workspace.  An item's outputs depend on its own first N frames only.
 *     VS_EINVAL before anything is launched, nothing written: NULL cand_hz / cand_d / f0_hz, aliased buffers, B < 1, T outside [1, 32768], a weight outside
 *     [0, 4096], reserved != 0.  No allocation, no atomics, no host synchronisation: a captured graph replays on other candidates by overwriting them.      */
#define VS_F0_PATH_MAX_FRAMES 32768
VS_API int vs_f0_candidates(const float *wav, const int64_t *lengths, int64_t B, int64_t L, int sr, int hop, float f0_min, float f0_max, int window,
                            float gate, float silence, float *cand_hz, float *cand_d, int64_t T, void *stream);
VS_API int vs_f0_path(const float *cand_hz, const float *cand_d, const int64_t *n_frames, int64_t B, int64_t T, int w_unvoiced, int w_switch, int w_order,
                      int w_jump, int jump_cap, int reserved, float *f0_hz, int32_t *state, int32_t *cost, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f13 vibrato (csrc/vibrato.hip): a per-note pitch modulation ADDED to the curve the model sings -- the predictor's own curve or a guide --
 *     between the pitch predictor and vs_pitch_condition.  Not in the reference.  f8 keeps, scales or removes the vibrato a recording has; nothing else adds one.
 *     Unit: 1/16 cent; 19200 units are an octave.  The offset is integer arithmetic on a host-built sine table: the device evaluates no transcendental function
 *     for it.  vs_pitch_condition and vs_f0_norm_interp are unchanged: the modulated curve goes into vs_pitch_condition as its f0_norm (with pred beside it when
 *     the voicing is the model's), so a transposition in cents moves the modulated curve and f0_hz_out shows it.
 *     vs_pitch_vibrato: curve fp32, read with an element stride of 1 (a normalised curve [B, T]) or 2 (column 0 of the predictor's [B, T, 2]), values in the
 *       model's domain log2(Hz + 1);  mel2ph int64 [B, T], read clamped to [0, T_ph], 0 = padding;  lengths DEVICE int64 [B], clamped to [0, T], or NULL (= T): Lr;
 *       note_of_token int32 [B, T_ph]: the note a token belongs to, 0 = no note (a rest);  note_depth_q int32 [B, T_ph] or NULL: the depth of a note in units, read
 *       at the note's FIRST token, negative (-1) = the item's;  params int32 [B, VS_VIBRATO_PARAMS]: depth_q, inc, delay, attack, release, min_len per item;
 *       sine int32 [VS_VIBRATO_SINE + 1]: round(16384 sin(2 pi i / 1024)), built on the host in double: part of the input.
 *       depth_q in [0, VS_VIBRATO_MAX_DEPTH_Q] units (one octave);  inc: the phase step per frame in 2^-32 cycles, taken as uint32 (the host makes it as
 *       round(rate_hz hop / sample_rate 2^32));  delay and min_len in [0, VS_VIBRATO_MAX_DELAY] frames;  attack and release in [1, VS_VIBRATO_MAX_RAMP] frames.
 *       The ranges cannot be checked on the device without a readback: they are the caller's to keep (the Python layer does), and a value outside is CLAMPED to
 *       its range, a note_depth_q above the maximum to the maximum: nothing out of range can fault.
 *       Per frame t < Lr:  n[t] = note_of_token[mel2ph[t] - 1], 0 where mel2ph[t] = 0.  start[t] = the last s <= t with s == 0 or n[s] != n[s - 1];
 *       end[t] = the first e > t with e == Lr or n[e] != n[e - 1].  len = end - start, p = t - start - delay, rem = end - 1 - t;  depth = the note's
 *       (note_depth_q at token mel2ph[start] - 1) when that is >= 0, else depth_q.
 *       offset_q[t] = 0 where n[t] == 0, len < min_len, p < 0 or depth == 0.  Otherwise, in integers:
 *         ph = (uint32)(inc * (uint32) p);  i = ph >> 22;  f = (ph >> 6) & 0xFFFF;  s = sine[i] + (((sine[i + 1] - sine[i]) * f) >> 16)  (arithmetic shift: floor);
 *         ea = min(p, attack);  er = min(rem + 1, release);  v = (int64) depth * s * ea * er;  den = 16384 * attack * release;
 *         offset_q[t] = sign(v) * ((|v| + den / 2) / den).
 *       |v| <= 19200 * 16384 * 4096^2 < 2^63, and |offset_q| <= depth.  The first modulated frame of a note is 0 (ea = 0): the vibrato fades in over `attack`
 *       frames behind the delay and out over the last `release` frames of the note.
 *       curve_out[t] = the bits of curve[t] where offset_q[t] == 0;  elsewhere log2f((exp2f(x) - 1) * exp2f((float) offset_q / 19200.0f) + 1), the accurate
 *       exp2f / log2f: the composition vs_pitch_condition uses for its cents.  For t >= Lr: offset_q = 0, curve_out = 0.  Every element of both is written.
 *       A frame's result depends on its own row's frames only: not on B, the row index or T.
 *       One launch: one workgroup per row (grid-strided), chunks of 256 frames walked right to left for `end` (parked in offset_q) and left to right for `start`,
 *       the boundary carried from chunk to chunk in a register, as in vs_f0_norm_interp: a note may span any number of chunks.
 *       VS_EINVAL before anything is launched: a NULL buffer other than lengths / note_depth_q, B, T, T_ph <= 0, T or T_ph >= 2^31, a stride other than 1 or 2,
 *       a stride-2 curve that is not 8-byte aligned, B T out of range, curve / offset_q / curve_out not three buffers.  No workspace, no allocation, no atomics,
 *       no host synchronisation; every input is read on the device: a captured graph replays under other settings by overwriting params.                  */
#define VS_VIBRATO_PARAMS 6
#define VS_VIBRATO_SINE 1024
#define VS_VIBRATO_MAX_DEPTH_Q 19200
#define VS_VIBRATO_MAX_RAMP 4096
#define VS_VIBRATO_MAX_DELAY 65535
VS_API int vs_pitch_vibrato(const float *curve, int curve_stride, const int64_t *mel2ph, const int64_t *lengths, const int32_t *note_of_token,
                            const int32_t *note_depth_q, const int32_t *params, const int32_t *sine, int32_t *offset_q, float *curve_out, int64_t B, int64_t T,
                            int64_t T_ph, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * f14 loudness normalisation (csrc/loudness.hip): the integrated programme loudness of every row of a batch of ragged waveforms -- mono ITU-R
 *     BS.1770-4 / EBU R128: K-weighted, gated, in LUFS -- and the gain that brings the row to a target.  Not in the reference (it peak-normalises on the host).
 *     wav fp32 [B, L] at sr Hz, sr an integer in [VS_LOUD_MIN_RATE, VS_LOUD_MAX_RATE] divisible by 10;  s = sr / 10 samples a step (100 ms);  lengths DEVICE
 *     int64 [B], clamped to [0, L], or NULL (= L): n.  Three entries, three launches, nothing read back in between.
 *     1. K-weighting.  Two biquads in cascade, b / a with a[0] = 1, made by the HOST in double from the rate (the bilinear transform of the standard's analogue
 *        prototypes, which gives the standard's 48 kHz table to the printed digits), K = tan(pi f0 / sr), a0 = 1 + K / Q + K^2:
 *          shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196;  Vh = 10^(G / 20), Vb = Vh^0.4996667741545416;
 *                     b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0],  a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *          high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773;  b = [1, -2, 1],  a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0].
 *        Each in transposed direct form II, in fp64, from a zero state at the row's first sample:  y = b0 x + z1;  z1 = b1 x - a1 y + z2;  z2 = b2 x - a2 y.
 *     2. Steps.  NS = the width of S.  Step i < min(n / s, NS) is the samples i s .. i s + s - 1;  S[b, i] = the fp64 sum of the squares of its weighted samples in
 *        a fixed order (lane l of 256 its c = ceil(s / 256) consecutive samples ascending, then a butterfly over the wave's 64 lanes, then the four waves);
 *        every other element of S is 0.  Only complete steps inside the row count.
 *        vs_loud_steps: coef HOST double [10]: b0 b1 b2 a1 a2 of the shelf, then of the high-pass;  carry DEVICE double [8, 2, 16]: with A the 4 x 4 transition of
 *        the cascade's state (z1, z2, z1', z2') over one sample of zero input and M = A^c, carry[k] is M^(2^k) row major as a pair (the exact power of A's doubles
 *        rounded once, and what that rounding left), built on the host: part of the input.  One workgroup per row walks the steps;  the state in front of every
 *        lane's samples comes from a log-step scan of the lanes' zero-state end states with these matrices, formed in pairs of doubles and rounded once per level.
 *        The result differs from the serial filter's by rounding only: the bound is derived in DESIGN.md 4.21.
 *     3. Blocks and gates (vs_loud_gate), fp64, the sums in a fixed order.  Block j < max(0, min(n / s, NS) - 3) is the steps j .. j + 3 (400 ms, 75 % overlap):
 *        z_j = (((S_j + S_(j+1)) + S_(j+2)) + S_(j+3)) / (4 s).  Absolute gate: z_j > VS_LOUD_ABS_GATE = 10^((-70 + 0.691) / 10).  Relative gate: of those,
 *        z_j > 0.1 (their sum / their number).  loud = -0.691 + 10 log10(the sum of the blocks over both / their number);  -inf when there is none;  NaN when a
 *        block of the row is not finite (a NaN or an infinity among the samples; such a block passes no gate).
 *        stats int32 [B, 3]: the blocks, those over the absolute gate, those over both.
 *     4. Gain.  gain = (float) 10^(min(target - loud, max_gain_db) / 20), formed in fp64 and rounded once;  1.0f where loud is not finite.  target in [-70, 0]
 *        LUFS, max_gain_db in [0, 60].  loud fp64 [B], gain fp32 [B].
 *     5. Apply (vs_gain_apply).  y = x gain[b], one fp32 product, for i < n;  y is the bits of x for i >= n and on every row whose gain is exactly 1.0f.
 *        y == x exactly (in place) is allowed.  16-byte loads and stores where L % 4 == 0 and x, y are 16-byte aligned, 4-byte ones otherwise: the same bits.
 *     A row's results depend on its own samples only: not on B, the row, L, the padding or the launch shape.
 *     VS_EINVAL before anything is launched, the outputs untouched: a NULL buffer other than lengths, s outside [800, 4800], B, L or NS < 1, L or NS >= 2^31, a
 *     coefficient that is not finite, target or max_gain_db out of range, an output overlapping another buffer (y == x apart).  No allocation, no atomics, no
 *     host synchronisation; samples, lengths, S and gain are read on the device: a captured graph replays on other data by overwriting them.            */
#define VS_LOUD_THREADS 256
#define VS_LOUD_MIN_RATE 8000
#define VS_LOUD_MAX_RATE 48000
#define VS_LOUD_ABS_GATE 1.1724653045822981e-07
VS_API int vs_loud_steps(const float *wav, const int64_t *lengths, int64_t B, int64_t L, const double *coef, const double *carry, int s, double *S, int64_t NS,
                         void *stream);
VS_API int vs_loud_gate(const double *S, const int64_t *lengths, int64_t B, int64_t NS, int s, double target, double max_gain_db, double *loud, float *gain,
                        int32_t *stats, void *stream);
VS_API int vs_gain_apply(const float *x, const float *gain, const int64_t *lengths, float *y, int64_t B, int64_t L, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * a13 grouped / strided Conv1d of the scale discriminator (modules/discriminator.py:55-60) and its gradients.
 *     x: [B, c_in, T], w: [c_out, c_in/groups, k], y / gy: [B, c_out, T_out], T_out = (T + 2*pad - k)/stride + 1.
 *     vs_gconv1d_bwd_weight writes one plane per batch item, gw_planes [B][c_out, c_in/groups, k]; gw = their sum.
 *     (The dense convs of both discriminators run on vs_conv_forward; strided ones through their de-interleaved phases.)  */
VS_API int vs_gconv1d_fwd(const float *x, const float *w, const float *bias, float *y, int64_t B, int64_t c_in, int64_t c_out,
                          int64_t T, int k, int stride, int pad, int groups, void *stream);
VS_API int vs_gconv1d_bwd_data(const float *gy, const float *w, float *gx, int64_t B, int64_t c_in, int64_t c_out, int64_t T,
                               int k, int stride, int pad, int groups, void *stream);
VS_API int vs_gconv1d_bwd_weight(const float *gy, const float *x, float *gw_planes, int64_t B, int64_t c_in, int64_t c_out,
                                 int64_t T, int k, int stride, int pad, int groups, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * a9  integer frame bookkeeping -- values are moved, never recomputed: bit-exact.
 *     vs_expand_states:  models/commons/align_ops.py:22-26.  out[b, t, :] = mel2token[b, t] ? h[b, mel2token[b,t]-1, :] : 0.
 *                        h: [B, T_tokens, C] (h_channels_first = 0) or [B, C, T_tokens] (1); out likewise with T_frames.
 *     vs_make_positions: modules/rel_transformer.py:78-88.  positions = cumsum(x != pad) * (x != pad) + pad  (int64),
 *                        x: [B, T] fp32 (the channel-0 slice the callers pass), pad = padding_idx.
 *     vs_slice_segments: modules/commons/utils.py:86-92.  out[b, :, s] = x[b, :, ids_str[b] + s],  x: [B, C, T].
 *     vs_mel2token_to_dur: utils/audio/align.py:105-129.  dur[b, i-1] = #{t : mel2token[b, t] == i}, i in 1..T_tokens
 *                        (index 0 = padding, dropped); clamped to max_dur when max_dur >= 0.  int64 in, int64 out.        */
VS_API int vs_expand_states(const float *h, const int64_t *mel2token, float *out, int64_t B, int64_t T_tokens,
                            int64_t T_frames, int64_t C, int h_channels_first, int out_channels_first, void *stream);
VS_API int vs_make_positions(const float *x, int64_t *positions, int64_t B, int64_t T, int64_t padding_idx, void *stream);
VS_API int vs_slice_segments(const float *x, const int64_t *ids_str, float *out, int64_t B, int64_t C, int64_t T,
                             int64_t segment_size, void *stream);
VS_API int vs_mel2token_to_dur(const int64_t *mel2token, int64_t *dur, int64_t B, int64_t T_frames, int64_t T_tokens,
                               int64_t max_dur, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISINGER_HIP_H */
