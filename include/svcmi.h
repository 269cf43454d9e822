/* svcmi.h -- C ABI of libsvcmi.so, the MI355X (gfx950) kernels of the SVC inference hot path.
 *
 * The reference (PlayVoice/whisper-vits-svc) has NO native/FFI interface: the path sits behind
 * Python callables.  This header is therefore the boundary a maintainer
 * would bind (ctypes stub in INTEGRATION.md).  Each entry point cites the reference code whose
 * arithmetic it replaces.  Conventions:
 *   - extern "C", plain pointers and sizes, no torch / C++ types, no exceptions, no hidden
 *     allocation; the caller owns every buffer and keeps it alive until the stream has drained.
 *   - every pointer is a DEVICE pointer (HBM); `stream` is a hipStream_t passed as void*.
 *   - activations are fp32, time-major / channels-last: element (b, t, c) of a tensor lives at
 *     base + b*bstride + t*ld + c.   (The reference is NCL [B,C,T]; the Python facade converts
 *     at the API edge.)  Leading dimensions are multiples of 4 floats and bases 16-byte aligned
 *     unless a function says otherwise.
 *   - `lengths` (int32[batch], may be NULL = all rows valid) carries the reference's x_mask
 *     (vits/commons.py:147-151): rows t >= lengths[b] are "masked".
 *   - return value: 0 = launched; <0 = svcmi_status (argument error, nothing launched);
 *     >0 = hipError_t from the launch.  Kernels are asynchronous on `stream`.
 */
#ifndef SVCMI_H
#define SVCMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVCMI_ABI_VERSION 22

enum svcmi_status { SVCMI_OK = 0, SVCMI_EINVAL = -1, SVCMI_EUNSUPPORTED = -2, SVCMI_EALIGN = -3 };

enum svcmi_act { SVCMI_ACT_NONE = 0, SVCMI_ACT_RELU = 1, SVCMI_ACT_GELU = 2, SVCMI_ACT_MISH = 3, SVCMI_ACT_TANH = 4, SVCMI_ACT_SIGMOID = 5 };

enum svcmi_conv_flags {
    SVCMI_CONV_ACCUMULATE = 1, /* y += result instead of y = result                          */
    SVCMI_CONV_MASK_IN = 2,    /* input rows >= lengths[b] read as zero   (conv(x * x_mask))  */
    SVCMI_CONV_MASK_OUT = 4,   /* output rows >= lengths[b] written as zero  (... * x_mask)   */
    SVCMI_CONV_PARTIALS = 8,   /* write exactly split_k raw partial slabs [batch][split_k][t_out][n_out] to `workspace` and stop:   */
                               /* no reduction, no epilogue, y untouched (consumer: svcmi_splitk_layernorm_f32)                     */
    /* tuning knob (bits 8-11): force the block tile (time x channels); 0 = library heuristic       */
    SVCMI_CONV_TILE_64x64 = 0x100,
    SVCMI_CONV_TILE_128x64 = 0x200,
    SVCMI_CONV_TILE_128x128 = 0x300,
    /* 16x16x4-MFMA tiles whose N spans the whole (narrow) output: n_out <= 48 / 80 / 160, c_in % 4 == 0 */
    SVCMI_CONV_TILE_P16_64x48 = 0x400,
    SVCMI_CONV_TILE_P16_128x48 = 0x500,
    SVCMI_CONV_TILE_P16_64x80 = 0x600,
    SVCMI_CONV_TILE_P16_128x80 = 0x700,
    SVCMI_CONV_TILE_P16_64x160 = 0x800,
    SVCMI_CONV_TILE_64x128 = 0x900, /* reduced-precision entry points only */
    /* ABI 22: the 64x80 wave tile on EIGHT-wave (512-thread) blocks: 128 x 80 per block = one block per CU at M = 500 x N = 5120 with two
     * waves per SIMD, 26 instead of 36 KB of LDS fill per CU and K-step; fp32 only, vector gathers; bit-identical to SVCMI_CONV_TILE_P16_64x80 */
    SVCMI_CONV_TILE_P16W8_128x80 = 0xA00,
    SVCMI_CONV_TILE_MASK = 0xF00,
    /* tuning knob: 2-deep operand ring instead of the 3-deep one of the 64-row fp32 tiles (64x64, P16 64x48 / 64x80): 33 / 41 KB of LDS
     * per block instead of 49 / 61 KB = one more resident block per CU and room for other streams' blocks beside them.  Slower for a
     * launch that has the chip to itself (one K-step of prefetch less), faster when several streams share it (clips in flight).  Results
     * are bit-identical (the ring depth does not touch the summation order).  Ignored by launches that have no such instantiation. */
    SVCMI_CONV_RING2 = 0x1000
};

int svcmi_abi_version(void);
/* "hip:gfx950" for the product build; the CPU SIMT emulator used by the unit tests says "emu". */
const char* svcmi_build_info(void);

/* ---------------------------------------------------------------------------------------------
 * 1-D convolution / linear layer as an implicit GEMM on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32, exact fp32).  Replaces every nn.Conv1d / nn.Linear / ConvTranspose1d
 * (polyphase-packed) on the path:
 *   whisper/model.py:34-45 (Linear, Conv1d), :144-163 (conv stem), :66-86,:118-129 (q/k/v/out, mlp);
 *   vits/models.py:26-37,44-46,49 (pre, hub, proj); vits/attentions.py:193-196 (conv_q/k/v/o),
 *   :390-403 (FFN); vits/modules.py:148-176,186,196 (WN in/res_skip), :273,281,285 (pre, post, snac);
 *   vits_decoder/generator.py:36-47 (adapter linears), :60,:69-99,:108 (conv_pre, ups, noise_convs,
 *   conv_post); vits_decoder/bigv.py:22-39 (AMP convs).
 *
 *   y[b,t,n] = epilogue( sum_{k<ksize} sum_{ci<c_in} x[b, (t*stride + k*dilation - pad) >> x_row_shift, ci]
 *                                                   * w[n, k*c_in + ci] )
 *   epilogue(v): v += bias[n]; v = act(v); v += res[b,t,n]; v *= alpha; (ACCUMULATE) v += y_old;
 *                (MASK_OUT) v = t < lengths[b] ? v : 0.
 * Input rows outside [0, t_in) (and, with MASK_IN, >= lengths[b]) read as zero.  x_row_shift = 1
 * fuses the np.repeat(ppg, 2, 0) of svc_inference.py:175-182 into the load (t_in is then the
 * repeated length).  w is [n_out][ldw] with ldw >= ksize*c_in, ldw % 4 == 0, zero padded.
 * c_in % 4 == 0 and ldx % 4 == 0 select 16-byte loads; any other c_in/ldx uses scalar loads.
 * y may alias res (in-place residual).  bias / res / lengths may be NULL.
 * Split-K: when the (time x channel) tile grid is too small to fill the GPU the K range can be cut into
 * `split_k` slices whose partial tiles go through `workspace` (caller-owned, >= batch*split_k*t_out*n_out
 * floats, any contents) and are summed in fixed slice order -- by the last block to finish each tile when `counters` is
 * given, by a second kernel otherwise -- deterministic either way (the only atomic is the arrival ticket).
 * split_k = 0 lets the library choose (never more than the workspace allows), 1 disables, workspace = NULL
 * disables.
 */
typedef struct svcmi_conv_desc {
    const float* x;
    const float* w;
    const float* bias;
    const float* res;
    float* y;
    const int32_t* lengths;
    int64_t x_bstride, y_bstride, res_bstride; /* in floats */
    int32_t batch, t_in, t_out, c_in, ldx, n_out, ldw, ldy, ldr;
    int32_t ksize, stride, dilation, pad, x_row_shift;
    int32_t act;   /* enum svcmi_act */
    int32_t flags; /* enum svcmi_conv_flags */
    float alpha;
    int32_t split_k;
    float* workspace;
    int64_t workspace_floats;
    int32_t* counters;     /* optional: >= one int32 per output tile, ALL ZERO on entry (the library leaves them zero).  With it   */
    int64_t counters_len;  /* the slices are combined inside the GEMM launch by the last-arriving block of each tile (fixed slice */
                           /* order: still deterministic); without it a second kernel does the reduction.                         */
    void* y16;             /* optional: a 16-bit copy of y (same values rounded to y16_format = SVCMI_PREC_BF16 | SVCMI_PREC_F16 | _BF16X3 = split), element (b,t,n) */
    int64_t y16_bstride;   /* at y16 + b*y16_bstride + t*ldy16 + n (in 16-bit elements): the A operand of a following _A16 launch, written by    */
    int32_t ldy16;         /* THIS launch's epilogue instead of being rounded in that launch's registers.  Needs the float4 epilogue (n_out,    */
    int32_t y16_format;    /* ldy % 4 == 0, aligned operands), no split-K.                                                                       */
} svcmi_conv_desc;

int svcmi_conv_gemm_f32(const svcmi_conv_desc* d, void* stream);

/* Up to 3 convolutions of one geometry (same batch, t_out, n_out, c_in and gather alignment; taps, dilation, padding, operands
 * and epilogues free) in ONE launch -- the three AMP blocks of a generator stage at the same step (vits_decoder/generator.py:
 * 188-194 runs them one after the other).  The grid holds the blocks of all problems, longest K first, so medium-sized
 * problems fill the chip several blocks deep without multi-stream concurrency.  No split-K, no SVCMI_CONV_PARTIALS, no
 * x_row_shift; tile override bits of descs[0] apply to all.  Outputs of different problems must not overlap. */
int svcmi_conv_gemm_group_f32(const svcmi_conv_desc* descs, int32_t count, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reduced-precision variants of the same convolution: 16-bit MULTIPLICANDS, fp32 accumulation, fp32 activations in
 * HBM on both sides (x, res, y, bias, workspace exactly as above).  The reference drops to fp16 on an accelerator
 * (whisper/inference.py:22-23,43-44: model.half(), mel.half()); here the choice is per call and opt-in:
 *   SVCMI_PREC_BF16X3  x = hi + lo with hi = bf16(x), lo = bf16(x - hi) on both operands, acc += hi*hi + lo*hi + hi*lo:
 *                      three bf16 MFMAs (16x the fp32 matrix rate each) for ~2^-17 relative error per product -- fp32-class
 *                      results (waveform within the 1e-3 parity bar, tests/test_gpu_precision.py) at up to ~5x the fp32 rate;
 *   SVCMI_PREC_BF16    operands rounded to bf16 (8-bit mantissa), one MFMA;
 *   SVCMI_PREC_F16     operands rounded to fp16 (11-bit mantissa, range 65504), one MFMA -- what `.half()` does.
 * Weights are converted ONCE by svcmi_pack_weights_lp from the fp32 operand [n][ldw] svcmi_conv_gemm_f32 takes to a 16-bit
 * image: row n = ldw16 values (K order permuted inside every block of 32 to match the kernel's fragment reads; bf16x3: hi row
 * followed by lo row, 2*ldw16 values per n); ldw16 % 32 == 0, ldw16 >= ldw, `out` 16-byte aligned and n*ldw16*2 (x2 for bf16x3)
 * bytes.  svcmi_conv_gemm_lp / svcmi_conv_gemm_group_lp take the SAME descriptor with d->w = that image and d->ldw = ldw16;
 * everything else (epilogue, masks, split-K, SVCMI_CONV_PARTIALS, grouping rules) is unchanged.  Activations are rounded in
 * registers inside the kernel, so no other kernel of the path changes.  Not supported (SVCMI_EUNSUPPORTED): per-element
 * gathers (c_in % 4 != 0 or unaligned x) and the in-launch split-K combine (`counters` is ignored). */
enum svcmi_precision { SVCMI_PREC_F32 = 0, SVCMI_PREC_BF16X3 = 1, SVCMI_PREC_BF16 = 2, SVCMI_PREC_F16 = 3,
                       /* 16-bit ACTIVATIONS as well: d->x is a bf16 / fp16 tensor (ldx, x_bstride in 16-bit elements; c_in, ldx, x_bstride % 8 == 0, x 16-byte
                        * aligned, no x_row_shift) that the producing kernel wrote (y16 of a convolution, svcmi_splitk_layernorm_f32, svcmi_layernorm_f32,
                        * svcmi_attention_f32, svcmi_snake_alias_group_f32), so nothing is rounded in this launch's registers and the operand tile in LDS is
                        * half the size.  Same products as SVCMI_PREC_BF16 / _F16 (the same fp32 values, rounded the same way); the weight image is packed
                        * by svcmi_pack_weights_lp with the _A16 code (natural k order instead of the permuted order of the other modes).
                        * SVCMI_PREC_BF16X3_A16: the split-bf16 products of SVCMI_PREC_BF16X3 on 16-bit activations: a row of d->x is [hi: ldx/2 values |
                        * lo: ldx/2 values] (what the producers write for y16_format = SVCMI_PREC_BF16X3; ldx % 16 == 0, c_in <= ldx/2), the weight image
                        * [hi row | lo row] in natural k order. */
                       SVCMI_PREC_BF16_A16 = 4, SVCMI_PREC_F16_A16 = 5, SVCMI_PREC_BF16X3_A16 = 6,
                       /* model-level only (svcmi_synth_model.precision): every layer CLASS of the synthesizer runs in its own mode,
                        * svcmi_synth_model.class_prec[] -- the per-layer mixed policy that keeps the 16-bit waveform error inside the parity bar */
                       SVCMI_PREC_MIXED = 7,
                       /* fp16 activations x SPLIT fp16 weights (round 4): a mode of a model / layer class that behaves like SVCMI_PREC_F16 (fp16 activation
                        * rows from the producers, fp16 attention) except that a convolution reading 16-bit activations runs as SVCMI_PREC_F16W2_A16: the
                        * static weight w = hi + lo with hi = fp16(w), lo = fp16(w - hi) (exact to 2^-22; the matrix cores honour the subnormal lo values:
                        * scripts/probes/mfma_f16_subnormal.hip), acc += a*hi + a*lo -- two MFMAs per fragment pair, the error of the product is the
                        * ACTIVATION rounding alone (0.6-0.7x of plain fp16, scripts/precision_sensitivity.py --operands a).  Weight image of the _A16 code:
                        * rows [hi: ldw16 | lo: ldw16] in natural k order; the non-_A16 launches of such a layer use the plain SVCMI_PREC_F16 image. */
                       SVCMI_PREC_F16W2 = 8, SVCMI_PREC_F16W2_A16 = 9 };
int svcmi_pack_weights_lp(const float* w, int32_t n, int32_t ldw, int32_t precision, void* out, int32_t ldw16, void* stream);
int svcmi_conv_gemm_lp(const svcmi_conv_desc* d, int32_t precision, void* stream);
int svcmi_conv_gemm_group_lp(const svcmi_conv_desc* descs, int32_t count, int32_t precision, void* stream);

/* LayerNorm over the channel dim of time-major rows, optional pre-add:
 *   y[r,:] = (v - mean(v)) / sqrt(var(v) + eps) * gamma + beta,   v = x[r,:] + (res ? res[r,:] : 0)
 * rows = batch*rows_per_batch contiguous rows of stride ldx/ldr/ldy.  gamma/beta (NULL = 1/0) are
 * indexed [ (r / rows_per_batch) * gb_bstride + c ] so a per-utterance affine can be applied.
 * Replaces whisper/model.py:28-31 (attn_ln, mlp_ln, ln_post), vits/modules.py:19-22 fused with the
 * `x + y` of vits/attentions.py:66,70, and the speaker-conditioned LN of
 * vits_decoder/generator.py:36-47 (gamma/beta = W_scale(spk)/W_bias(spk), gb_bstride = c).
 * c % 4 == 0, c <= 2048. */
int svcmi_layernorm_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                        int32_t batch, int32_t rows_per_batch, int32_t c, int32_t ldx, int32_t ldr, int32_t ldy,
                        int32_t gb_bstride, float eps, void* y16, int32_t ldy16, int32_t y16_format, void* stream);
/* (y16 / ldy16 / y16_format here and below: an optional second output, the same rows rounded to bf16 / fp16 (SVCMI_PREC_BF16 |
 * SVCMI_PREC_F16) with leading dimension ldy16 in 16-bit elements -- the A operand of a following SVCMI_PREC_*_A16 convolution.
 * SVCMI_PREC_BF16X3: split rows, hi = bf16(v) at [c] and lo = bf16(v - hi) at [ldy16/2 + c] (ldy16 % 8 == 0, ldy16/2 >= the row
 * length) for SVCMI_PREC_BF16X3_A16.  NULL = none.) */

/* Per-channel normalisation over time + GELU: GroupNorm(num_groups = c, c) followed by exact-erf GELU, the first layer of
 * HuBERT's feature extractor (hubert/hubert_model.py:78,88): y[b,t,ch] = gelu((x[b,t,ch] - mean_t) / sqrt(var_t + eps) *
 * gamma[ch] + beta[ch]) with mean / biased variance over the t axis of batch item b.  x, y: [batch][t][ld] time-major
 * (y may alias x); scratch: >= batch * 129 * c doubles.  c % 4 == 0. */
int svcmi_channel_norm_gelu_f32(const float* x, const float* gamma, const float* beta, float* y, double* scratch,
                                int32_t batch, int32_t t, int32_t c, int32_t ldx, int32_t ldy, float eps, void* stream);

/* Split-K tail fused with the residual update and the LayerNorm that follows it (whisper/model.py:118-129:
 * `x = x + attn(...)` / `x = x + mlp(...)` then the next `ln(x)`):
 *   x[r,:] += bias + sum_{s<split} partials[b, s, t, :]   (slice order fixed);   y[r,:] = LayerNorm(x[r,:]) * gamma + beta
 * partials: the slabs a SVCMI_CONV_PARTIALS launch of svcmi_conv_gemm_f32 left in its workspace ([batch][split][t][c]).
 * rows r = b*rows_per_batch + t.  c % 4 == 0, c <= 2048. */
int svcmi_splitk_layernorm_f32(const float* partials, int32_t split, const float* bias, float* x, const float* gamma,
                               const float* beta, float* y, int32_t batch, int32_t rows_per_batch, int32_t c,
                               int32_t ldx, int32_t ldy, float eps, void* y16, int32_t ldy16, int32_t y16_format, void* stream);

/* Multi-head self-attention with exact (fp32, online) softmax.
 *   S[i,j] = scale * ( q_i . k_j  +  (|j-i| <= window ? q_i . rel_k[j-i+window] : 0) )
 *   S[i,j] = -1e4 where i >= lengths[b] or j >= lengths[b]           (masked_fill, attentions.py:249)
 *   P = softmax_j(S);  o_i = sum_j P[i,j] v_j  +  sum_{|j-i|<=window} P[i,j] rel_v[j-i+window]
 * q/k/v/o: element (b, t, h, d) at base + b*bstride + t*ld + h*head_dim + d (so q,k,v can point into
 * one fused [T, 3C] projection).  rel_k/rel_v: [2*window+1][head_dim] shared by heads, or NULL
 * (then window is ignored).  head_dim in {16, 32, 64, 96}.
 * Replaces whisper/model.py:88-101 (scale = head_dim^-0.5, no rel, no mask) and
 * vits/attentions.py:225-274 incl. the relative-position skew helpers :276-347. */
int svcmi_attention_f32(const float* q, const float* k, const float* v, float* o,
                        int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                        int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride,
                        int32_t batch, int32_t t, int32_t heads, int32_t head_dim, float scale,
                        const float* rel_k, const float* rel_v, int32_t window,
                        const int32_t* lengths, void* o16, int32_t ldo16, int64_t o16_bstride, int32_t o16_format, void* stream);

/* The same attention on the 16-bit matrix cores, for the bf16 / f16 modes (rel_k / rel_v / window as above, fp32 tables, or NULL): q / k / v are 16-bit tensors
 * (`format` = SVCMI_PREC_BF16 | SVCMI_PREC_F16; element (b, t, h, d) at base + b*bstride16 + t*ld16 + h*head_dim + d, in 16-bit elements --
 * the y16 copy of the fused QKV projection), products on v_mfma_f32_16x16x32, softmax statistics / rescale / accumulation in fp32, P
 * rounded to `format` before the PV product.  K / V tiles of a head are staged once per block through LDS (V transposed on the way in).
 * Outputs: o (fp32, may be NULL) and / or o16 (16-bit copy in `format`, may be NULL): the out-projection's A operand.  head_dim in {32, 64}
 * without the band, {32, 96} with it.  Replaces whisper/model.py:88-101 under `.half()` (whisper/inference.py:22-23) and, in the 16-bit
 * modes of the synthesizer, vits/attentions.py:225-274. */
int svcmi_attention16(const void* q, const void* k, const void* v, int32_t ld16, int64_t bstride16, float* o, int32_t ldo,
                      int64_t o_bstride, void* o16, int32_t ldo16, int64_t o16_bstride, int32_t batch, int32_t t, int32_t heads,
                      int32_t head_dim, float scale, const float* rel_k, const float* rel_v, int32_t window,
                      const int32_t* lengths, int32_t format, void* stream);

/* Anti-aliased SnakeBeta (vits_decoder/alias/act.py:124-129): 2x Kaiser-sinc polyphase upsample with
 * replicate padding (resample.py:25-33), x + sin^2(x*e^alpha)/(e^beta + 1e-9) (act.py:79-92), 12-tap
 * low-pass + 2x decimation (filter.py:86-95).  x,y: [batch][len][ld] time-major, c <= ld channels;
 * alpha_log/beta_log: [c]; filt: the 12 taps (filter.py:28-57).  SURVEY.md A.5.  One batch item is addressed with 32-bit byte
 * offsets: len * ld * 4 >= 2^31 returns SVCMI_EUNSUPPORTED (a 32 kHz x 10-channel tensor of that size is 1.5 hours of audio). */
int svcmi_snake_alias_f32(const float* x, float* y, const float* alpha_log, const float* beta_log,
                          const float* filt, int32_t batch, int32_t len, int32_t c, int32_t ld, void* stream);
/* The same activation for up to 3 tensors of one shape in one launch (x[i] -> y[i] with alpha_log[i] / beta_log[i]): the AMP
 * blocks of a generator stage at the same step.  The pointer arrays are host arrays read during the call. */
int svcmi_snake_alias_group_f32(const float* const* x, float* const* y, const float* const* alpha_log,
                                const float* const* beta_log, const float* filt, int32_t count, int32_t batch,
                                int32_t len, int32_t c, int32_t ld, void* const* y16, int32_t y16_format, void* stream);
/* (y16 != NULL: tensor i is written as bf16 / fp16 rows (y16_format, same ld) to y16[i] INSTEAD of fp32 to y[i] -- the activation only
 * feeds the following convolution, which then runs as an SVCMI_PREC_*_A16 launch; y / y[i] may be NULL then.  y16_format =
 * SVCMI_PREC_BF16X3: split rows of 2*ld values, [hi: ld | lo: ld].) */
/* y[i] = ((xs[0][i] + xs[1][i]) + xs[2][i]) / count, count <= 3: the `xs / num_kernels` of vits_decoder/generator.py:188-194
 * when the AMP blocks ran side by side in grouped launches.  n % 4 == 0, 16-byte aligned pointers; y may alias xs[0]. */
int svcmi_block_mean_f32(const float* const* xs, int32_t count, float* y, int64_t n, void* stream);

/* Fused AMP half-step for the narrow generator stages (vits_decoder/bigv.py:50-58: `xt = act(x); xt = conv(xt)`):
 *   y[b,t,n] = alpha * ( bias[n] + sum_{k<ksize} sum_{ci<c} w[n, k*ld + ci] * S[b, t + (k - (ksize-1)/2)*dilation, ci]
 *                        + res[b,t,n] )  (+ y_old[b,t,n] when accumulate != 0),      n < c
 * with S = SnakeAlias(x) exactly as svcmi_snake_alias_f32 computes it and S rows outside [0, len) read as zero
 * (the convolution's 'same' zero padding, stride 1).  x, y, res: [batch][len][ld] time-major; channels c..ld-1
 * of y are written as zero.  w: [ld][ldw] packed like svcmi_conv_gemm_f32's (tap-major, ld channels per tap).
 * res may alias y; x must not.  Supported shapes: (c, ld) in {(10,12), (20,20), (40,40)}, ksize in {3,7,11},
 * dilation 1..5 -- svcmi_snake_conv_supported() tells; other shapes return SVCMI_EUNSUPPORTED and the caller
 * uses svcmi_snake_alias_f32 + svcmi_conv_gemm_f32. */
int svcmi_snake_conv_supported(int32_t c, int32_t ld, int32_t ksize, int32_t dilation);
/* 1 where the fused kernel is also the FASTER choice on MI355X (narrowest stages); the facade follows it. */
int svcmi_snake_conv_preferred(int32_t c, int32_t ld, int32_t ksize, int32_t dilation);
int svcmi_snake_conv_f32(const float* x, const float* w, const float* bias, const float* res, float* y,
                         const float* alpha_log, const float* beta_log, const float* filt,
                         int32_t batch, int32_t len, int32_t c, int32_t ld, int32_t ldw, int32_t ksize,
                         int32_t dilation, float alpha, int32_t accumulate, void* stream);

/* The same half-step for up to 3 AMP blocks of a stage in one launch (own taps / dilation / weights / activation
 * parameters / tensors; shared shape batch x len x ld and channel count c).  Problems are run most-taps-first.  Outputs of
 * different problems must not overlap.  Same support matrix as svcmi_snake_conv_f32. */
typedef struct svcmi_snake_conv_desc {
    const float* x; const float* w; const float* bias; const float* res; float* y;
    const float* alpha_log; const float* beta_log;
    int32_t ldw, ksize, dilation, accumulate;
    float alpha;
} svcmi_snake_conv_desc;
int svcmi_snake_conv_group_f32(const svcmi_snake_conv_desc* descs, int32_t count, const float* filt, int32_t batch,
                               int32_t len, int32_t c, int32_t ld, void* stream);

/* The grouped half-step with its convolution on the fp16 matrix cores -- the narrow stages' member of the per-layer mixed-precision
 * policy (classes amp3 / amp4).  `precision`: SVCMI_PREC_F16 (weights rounded to fp16, one MFMA per tile) or SVCMI_PREC_F16W2 (weights as
 * hi + lo fp16, two MFMAs: only the activated input is rounded).  x / res / y / bias / weights are the SAME fp32 tensors the _f32 entry
 * takes (the block converts its problem's weights to MFMA fragment order in LDS); accumulation, epilogue and SnakeAlias are fp32.
 * 10 and 20 channels; y, res and bias 16-byte aligned. */
int svcmi_snake_conv_lp_supported(int32_t c, int32_t ld, int32_t ksize, int32_t dilation, int32_t precision);
int svcmi_snake_conv_group_lp(const svcmi_snake_conv_desc* descs, int32_t count, const float* filt, int32_t batch,
                              int32_t len, int32_t c, int32_t ld, int32_t precision, void* stream);

/* Stage entry of the narrow generator stages in one launch (vits_decoder/generator.py:183-186):
 *   y[b, u*q + r, co] = b_up[r*cp+co] + sum_{k<taps} sum_{ci<c_in} x[b, q + k - pad, ci] * w_up[r*cp+co, k*c_in + ci]      (ups[i], polyphase)
 *                     + b_nz[co] + sum_{k<nz_k} src[b, (u*q+r)*nz_stride - nz_pad + k] * w_nz[co, k]                       (noise_convs[i])
 * x: [batch][t_in][c_in]; w_up / b_up: the polyphase operands svcmi_conv_gemm_f32 would take ([u*cp][ldw_up], rows outside
 * the tensor read as zero); src: [batch][src_len]; y: [batch][t_in*u][cp].  x == NULL selects the noise-only mode: y already
 * holds ups[i](x) and only the second line is added (20-channel stage: its transposed convolution is faster on the
 * matrix cores).  Supported: u == 2, cp in {12, 20}, c_in % 4 == 0
 * (svcmi_upsample_noise_supported); other shapes use two svcmi_conv_gemm_f32 launches. */
int svcmi_upsample_noise_supported(int32_t u, int32_t cp, int32_t c_in);
int svcmi_upsample_noise_f32(const float* x, const float* w_up, const float* b_up, const float* src, const float* w_nz,
                             const float* b_nz, float* y, int32_t batch, int32_t t_in, int32_t c_in, int32_t ldw_up,
                             int32_t taps, int32_t pad, int32_t u, int32_t cp, int64_t src_len, int32_t nz_k,
                             int32_t nz_stride, int32_t nz_pad, int32_t ldw_nz, void* stream);

/* Output layer of the generator in one launch (vits_decoder/generator.py:196-199: activation_post, conv_post, tanh):
 *   y[b, t] = tanh( sum_{k < ksize} sum_{ci < c} w[k*ld + ci] * S[b, t + k - (ksize-1)/2, ci] ),  S = SnakeAlias(x) zero-padded
 * x: [batch][len][ld] time-major, w: conv_post.weight packed as one row (tap-major, ld floats per tap; no bias),
 * y: [batch][len].  Supported: c == 10, ld == 12, ksize == 7 (svcmi_snake_post_supported); other widths use
 * svcmi_snake_alias_f32 + svcmi_conv_gemm_f32. */
int svcmi_snake_post_supported(int32_t c, int32_t ld, int32_t ksize);
int svcmi_snake_post_f32(const float* x, const float* w, float* y, const float* alpha_log, const float* beta_log,
                         const float* filt, int32_t batch, int32_t len, int32_t c, int32_t ld, int32_t ksize, void* stream);

/* Development knobs for the tuning scripts (kernel SHAPE choices only: results never depend on them beyond fp32 re-association):
 *   "amp_tt"   {0 = default, 1, 2, 4}   time steps per thread of svcmi_snake_conv_f32
 *   "amp_u"    {0 = measured choice, -1 = never, 1 = wherever it exists}  grouped fused narrow-stage kernel with the up-sampled activation tile in LDS
 *   "amp_grouped" {1 = default, 0}      0 forces the one-launch-per-AMP-block fallback of the generator stages (stage host)
 *   "group_nst" {0 = default, 2, 3}     LDS ring depth of the grouped implicit-GEMM launches
 *   "attn_ns"  {0 = heuristic, 1, 2, 4, 8}  key-split waves per block of svcmi_attention_f32
 *   "attn_q32" {-1 = heuristic, 0, 1}   two query tiles per wave (band-free attention, head_dim <= 64)
 *   "attn16"   {0 = heuristic, 41, 42, 44, 81, 82; with the band: 14, 21, 24, 42, 44}  block shape (10 * query tiles + key ranges) of svcmi_attention16
 *   "attn_lds" {0 = heuristic, -1 = never, 1, 10*QT+KS}  band-free attention with K / V tiles staged through LDS and shared by QT in
 *              {2, 4, 8} query tiles x KS in {1, 2, 4} key ranges per block (1 = 4 x 2; compiled shapes 21 22 24 41 42 44 81 82)
 * Process-wide, not thread-safe against concurrent launches.  Returns 0, or SVCMI_EINVAL for an unknown name / value. */
int svcmi_tune_set(const char* name, int32_t value);
/* ABI 22: the current value of "ring2" / "amp_grouped" / "amp_lp" / "group_nst", and "last_conv_ring" = which instantiation the last
 * svcmi_conv_gemm_f32 launch took: 2 = the SVCMI_CONV_RING2 one, 3 = the tile's default (tests assert which kernel a flag selected).  0, or SVCMI_EINVAL. */
int svcmi_tune_get(const char* name, int32_t* value);

/* WaveNet gate, vits/commons.py:126-133 with input_b == 0 (vits/modules.py:190-193):
 *   out[b, t, c] = tanh(v[b, t, c]) * sigmoid(v[b, t, h + c]),  c < h,  v = bias + sum_s a[b][s][t][:]
 * a: `splits` slabs per batch item, [batch][splits][t][lda] -- the raw split-K partials of the in_layer convolution
 * (SVCMI_CONV_PARTIALS, lda == 2h) summed here in slab order with the layer bias, so that the reduce pass, the bias and the
 * gate are one launch; or the finished activations with splits == 1 (bias may be NULL). */
int svcmi_wn_gate_f32(const float* a, const float* bias, float* out, int32_t batch, int32_t t, int32_t h, int32_t lda,
                      int32_t ldo, int32_t splits, void* stream);

/* WaveNet residual/skip bookkeeping, vits/modules.py:196-203, from rs = res_skip_layer(acts):
 *   !last: x = (x + rs[:, :h]) * mask ; skip (+)= rs[:, h:2h]        last: skip (+)= rs[:, :h]; skip *= mask
 * `first` makes skip = instead of += (output = zeros_like(x) at :179). */
int svcmi_wn_update_f32(const float* rs, float* x, float* skip, const int32_t* lengths,
                        int32_t batch, int32_t t, int32_t h, int32_t ldrs, int32_t first, int32_t last, void* stream);

/* Speaker-normalised coupling, reverse direction (vits/modules.py:288-321 with mean_only).
 * ms_vs: [batch][2*half] = snac(spk) laid out (m_s | v_s), already permuted for flipped layers.
 * pre :  out[b,t,c] = (x[b,t,x0_off+c] - m_s[c]) * exp(-v_s[c]) * mask
 * post:  x1 = x[b,t,x1_off+c];  x1 = (x1 - m[b,t,c]) * mask;  x[b,t,x1_off+c] = (m_s[c] + x1*exp(v_s[c])) * mask
 * torch.flip (modules.py:225-229) is folded into the x0/x1 offsets and weight permutations at load. */
int svcmi_coupling_pre_f32(const float* x, int32_t ldx, int32_t x0_off, const float* ms_vs, float* out, int32_t ldo,
                           const int32_t* lengths, int32_t batch, int32_t t, int32_t half, void* stream);
int svcmi_coupling_post_f32(float* x, int32_t ldx, int32_t x1_off, const float* m, int32_t ldm, const float* ms_vs,
                            const int32_t* lengths, int32_t batch, int32_t t, int32_t half, void* stream);

/* x[b,t,:] = (x[b,t,:] + emb[f0_to_coarse(pit[b,t]), :]) * mask   -- vits/utils.py:20-33 (Hz -> bin 1..255)
 * + nn.Embedding lookup and the sum/mask of vits/models.py:44-48.  emb: [256][c]. */
int svcmi_embed_pitch_f32(float* x, int32_t ldx, const float* pit, const float* emb, const int32_t* lengths,
                          int32_t batch, int32_t t, int32_t c, void* stream);

/* z[b,t,c] = (m + noise[b,c,t] * exp(logs)) * mask with (m | logs) = stats[b,t,0:i | i:2i]
 * (vits/models.py:49-51).  noise is the reference's randn_like(m) in ITS layout [batch][i][t]. */
int svcmi_sample_prior_f32(const float* stats, int32_t lds, const float* noise_ncl, const int32_t* lengths,
                           float* z, int32_t ldz, int32_t batch, int32_t t, int32_t i, void* stream);

/* Layout bridges at the API edge.  ncl_to_nlc: y[b,t,c] = x[b,c,t] + add_scale*add[b,c,t] (add may be NULL;
 * used for `mel + 0.1*randn`, whisper/inference.py:46).  nlc_to_ncl: y[b,c,t] = x[b,t,c]. */
int svcmi_ncl_to_nlc_f32(const float* x, const float* add, float add_scale, float* y,
                         int32_t batch, int32_t c, int32_t t, int32_t ldy, void* stream);
int svcmi_nlc_to_ncl_f32(const float* x, int32_t ldx, float* y, int32_t batch, int32_t c, int32_t t, void* stream);

/* Harmonic source (vits_decoder/generator.py:160-165 -> nsf.py:223-253,284-316,383-394).
 * Step 1: per-frame phase prefix.  rad[f,k] = fmodf(f0[b,f]*(k+1)/sr, 1) in fp32 exactly as :228; the sample-level
 *   double cumsum of :246-253 collapses (F0 is piecewise constant over a hop) to
 *   prefix[b,f,k] = frac(rand_ini[b,k] + hop * sum_{f'<f} rad[f',k]) accumulated in fp64.  rand_ini column 0 is
 *   treated as 0 (:235).
 * Step 2: out[b, f*hop+j] = tanh(sum_k merge_w[k]*(0.1*sin(2*pi*(prefix + (j+1)*rad))*uv + amp*noise[b,t,k]) + merge_b),
 *   uv = f0 > 0, amp = uv ? 0.003 : 0.1/3 (:305-314); noise: [batch][t*hop][11] as drawn by randn_like(:311). */
int svcmi_pitch_prefix_f64(const float* f0, const float* rand_ini, double* prefix,
                           int32_t batch, int32_t t, int32_t hop, float sr, void* stream);
int svcmi_pitch_source_f32(const float* f0, const double* prefix, const float* noise, const float* merge_w,
                           float merge_b, float* out, int32_t batch, int32_t t, int32_t hop, float sr, void* stream);

/* Whisper log-mel front-end (whisper/audio.py:68-100), the glue around two svcmi_conv_gemm_f32 launches (the windowed DFT
 * is a stride-160 / 400-tap / 1-channel convolution with a [hann*cos | -hann*sin] basis, the mel projection a linear
 * layer):
 *   reflect_pad:     y[b, i] = x[b, reflect(i - pad)], i < n + 2*pad          (torch.stft center=True, pad_mode="reflect")
 *   power_spectrum:  p[r, f] = ri[r, f]^2 + ri[r, half + f]^2, f < nbins; p[r, nbins..ldp) = 0
 *   logmel_finish:   v = log10(max(mel_power, 1e-10)); v = max(v, max_b(v) - 8); out[b, c, t] = (v[b, t, c] + 4) / 4
 *                    mel_power [batch][t][c] is overwritten; scratch >= 64*batch floats; out is NCL like the reference. */
int svcmi_reflect_pad_f32(const float* x, float* y, int32_t batch, int64_t n, int32_t pad, void* stream);
int svcmi_power_spectrum_f32(const float* ri, float* p, int64_t rows, int32_t nbins, int32_t half, int32_t ldri, int32_t ldp, void* stream);
int svcmi_logmel_finish_f32(float* mel_power, float* scratch, float* out, int32_t batch, int32_t t, int32_t c, void* stream);

/* Any-rate wav input (whisper/audio.py:24-26, librosa.load(file, sr=16000)): PCM decode, channel downmix and rational resampling
 * by up / down in one launch (added under ABI 22: purely additive).
 *   pcm:  `frames` interleaved frames of `channels` (1..8) samples as the file holds them; fmt 0 = float32 (as is), 1 = int16 (/ 2^15),
 *         2 = int32 ((float)v / 2^31), 3 = uint8 ((v - 128) / 128).  A frame's channels are summed in channel order in fp32 and
 *         divided by (float)channels (bit-equal to numpy's float32 mean(axis=1) for up to 7 channels).
 *   taps: the low-pass h (2 * half + 1 values, already scaled by up) packed by phase: taps[p * taps_per_phase + k] = h[p + k * up], 0 past
 *         the end of h; taps_per_phase = ceil((2 * half + 1) / up).  With c = m * down + half, p = c mod up, j = c div up:
 *             out[m] = sum_{k < taps_per_phase} x[j - k] * taps[p * taps_per_phase + k],      x = 0 outside [0, frames)
 *         accumulated with fmaf in ascending k -- scipy.signal.resample_poly's output for its own default filter, to fp32 rounding.
 *         taps == NULL (only with up == down == 1): decode + downmix only.
 *   out:  n_out = ceil(frames * up / down) floats.
 * SVCMI_EINVAL before anything is launched for null pcm / out, frames <= 0, an unknown fmt, channels outside 1..8, up or down < 1,
 * another n_out, taps == NULL with up != 1 or down != 1, another taps_per_phase; SVCMI_EALIGN for a pcm / taps / out pointer that is
 * not aligned to its element; SVCMI_EUNSUPPORTED for taps_per_phase > 4096 (down / up beyond ~200). */
int svcmi_pcm_resample_f32(const void* pcm, int32_t fmt, int32_t channels, int64_t frames, const float* taps, int32_t up, int32_t down,
                           int32_t taps_per_phase, int32_t half, float* out, int64_t n_out, void* stream);

/* Speaker encoder (row N5; speaker/models/lstm.py, speaker/utils/audio.py -- added under ABI 22: purely additive).
 *   lstm_step:  ONE time step t of one nn.LSTM layer for all batch rows (gate order i, f, g, o; zero initial state):
 *                   G = gx[b][t][:] + h_{t-1}[b] * W_hh^T;   c = sigmoid(f) c + sigmoid(i) tanh(g);   h_t = sigmoid(o) tanh(c)
 *               gx:   [batch][t_total][4 * hidden] (batch stride gx_bstride floats) = X * W_ih^T + b_ih + b_hh, columns in TILE ORDER:
 *                     column 16 * (j / 4) + 4 * gate + j % 4 holds gate `gate` of hidden unit j (a block of the kernel owns 4 units);
 *               whh:  W_hh [4 * hidden][hidden] with its rows in the same order (row stride = hidden), 16-byte aligned;
 *               hseq: the layer's output sequence [batch][t_total][ldh]: row t - 1 is read (nothing at t = 0), row t is written;
 *               c:    the cell state [batch][ldc], updated in place (not read at t = 0).
 *               The T steps of a layer are T launches in stream order.  K is reduced in a fixed order: a row's bits depend neither on
 *               the run nor on the batch it is launched in.  Saturated gates give exactly 0 / 1 / +-1, never NaN.
 *               SVCMI_EINVAL (before any launch): a null pointer, batch / hidden / t_total < 1, t outside [0, t_total), ldh or ldc < hidden,
 *               strides smaller than a sequence; SVCMI_EUNSUPPORTED: batch > 64; SVCMI_EALIGN: hidden % 4, ldh % 4, h_bstride % 4, whh /
 *               hseq not 16-byte aligned.
 *   preemph_pad: y[b][i] = p[reflect(i - pad)], p[n] = x[n] - coef * x[n - 1], p[0] = x[0] (lfilter([1, -coef], [1], x), then the
 *               reflect padding of a centred STFT); x [batch][n], y [batch][n + 2 * pad], pad < n.
 *   magnitude_spectrum: as svcmi_power_spectrum_f32, with sqrt(re^2 + im^2).
 *   speaker_mel_finish: in place on `total` mel-projected magnitudes m: S = 20 log10(max(1e-5, m)) - ref_level_db;
 *               S = (S - min_level_db) / -min_level_db;  S = 2 max_norm S - max_norm;  clipped to +-max_norm (AudioProcessor.normalize).
 *   l2norm_rows: y[r][:] = x[r][:] / max(|x[r]|_2, 1e-12) (torch.nn.functional.normalize).
 *   group_mean: y[g][:] = mean of rows g * rows_per_group .. of x [groups * rows_per_group][d], summed in row order. */
int svcmi_lstm_step_f32(const float* gx, int64_t gx_bstride, const float* whh, float* hseq, int64_t h_bstride, int32_t ldh,
                        float* c, int32_t ldc, int32_t batch, int32_t hidden, int32_t t, int32_t t_total, void* stream);
int svcmi_preemph_pad_f32(const float* x, float* y, int32_t batch, int64_t n, int32_t pad, float coef, void* stream);
int svcmi_magnitude_spectrum_f32(const float* ri, float* p, int64_t rows, int32_t nbins, int32_t half, int32_t ldri, int32_t ldp, void* stream);
int svcmi_speaker_mel_finish_f32(float* mel, int64_t total, float ref_level_db, float min_level_db, float max_norm, void* stream);
int svcmi_l2norm_rows_f32(const float* x, int64_t ldx, int32_t rows, int32_t d, float* y, int64_t ldy, void* stream);
int svcmi_group_mean_f32(const float* x, int32_t rows_per_group, int32_t groups, int32_t d, float* y, void* stream);

/* Linear spectrogram of a training item (prepare/preprocess_spec.py -> vits/spectrogram.py:41-76, spectrogram_torch with center=False)
 * in one launch (added under ABI 22: purely additive):
 *   xp[p] = x[b][reflect(p - pad)], p < n + 2 * pad (F.pad mode="reflect", as index arithmetic on the load: no padded copy);
 *   out[b][k][t] = sqrt(re^2 + im^2 + eps),  re | im = sum_{i < n_fft} xp[t * hop + i] * basis[i][2k | 2k + 1],  k < bins = n_fft / 2 + 1,
 *   t < frames = 1 + (n + 2 * pad - n_fft) / hop  (torch.stft without centring).
 *   x:     [batch][n] fp32, batch stride x_bstride floats (>= n);
 *   basis: [n_fft][2 * bins] fp32, made by the host in float64 and rounded once: basis[i][2k] = w[i] cos(2 pi ((k i) mod n_fft) / n_fft), the odd
 *          column with sin; w = the periodic Hann window of win_length, centred and zero padded to n_fft as torch.stft does (the window lives
 *          in the table, so win_length < n_fft costs nothing);
 *   out:   [batch][bins][frames] contiguous, the layout the reference saves.
 * The DFT runs on the fp32 matrix cores (K = n_fft, N = 2 * bins, M = frames).  Every output is one accumulator chain over i in ascending
 * order followed by sqrtf(fmaf(re, re, fmaf(im, im, eps))): its bits depend on the frame's n_fft padded samples and the table alone, not on the
 * tile, the number of frames, the batch index or the stream.
 * SVCMI_EINVAL before anything is launched for a null pointer, batch < 1, hop < 1, pad < 0, an odd n_fft (or < 2), n <= pad (the reference's
 * reflect pad raises there), n + 2 * pad < n_fft (frames < 1), another `frames`, x_bstride < n with batch > 1; SVCMI_EALIGN for a pointer
 * that is not 4-byte aligned; SVCMI_EUNSUPPORTED for batch > 65535. */
int svcmi_linear_spectrogram_f32(const float* x, int64_t x_bstride, int32_t batch, int64_t n, const float* basis, int32_t n_fft, int32_t hop,
                                 int32_t pad, float eps, float* out, int64_t frames, void* stream);

/* Checkpoint scoring (vits_extend/validation.py, stft.py, stft_loss.py) without materialised spectrograms (csrc/spectral_loss.hip; added
 * under ABI 22: purely additive).
 *   stft_distance: one STFT resolution of a pair, x = the predicted and y = the recorded signal, [batch][n] fp32 with batch strides
 *               x_bstride / y_bstride floats (>= n).  With re | im as in svcmi_linear_spectrogram_f32 (the same `basis`, pad and frames;
 *               torch.stft's center=True is pad = n_fft / 2, frames = 1 + n / hop) and m = sqrt(max(re^2 + im^2, floor)) (stft_loss.py:28,
 *               floor = 1e-7):   out[b][0] = sum (my - mx)^2,  out[b][1] = sum my^2,  out[b][2] = sum |log my - log mx|
 *               over all k < bins and t < frames, as doubles.  Each table fragment feeds both signals, which go through the same
 *               arithmetic chain: stft_distance(x, x) is exactly (0, sum, 0).  No atomics: every block of the grid (32 frames x 64 bins)
 *               writes one fp32 triple to its own slot of `partials`, and a second kernel adds an item's slots in ascending order in
 *               fp64.  The three doubles of an item depend on its samples and the table alone, not on the batch index, the batch size
 *               or the stream.  `partials`: at least svcmi_stft_distance_workspace_bytes(batch, n, n_fft, hop, pad) bytes
 *               (= 12 * batch * ceil(frames / 32) * ceil(bins / 64)), overwritten; launches that may overlap need their own.
 *               SVCMI_EINVAL before anything is launched or written for a null pointer, batch < 1, hop < 1, pad < 0, an odd n_fft (or
 *               < 2), n <= pad, n + 2 * pad < n_fft, another `frames`, a batch stride < n with batch > 1, floor <= 0, partials_bytes too
 *               small; SVCMI_EALIGN for x / y / basis / partials not 4-byte or out not 8-byte aligned; SVCMI_EUNSUPPORTED for
 *               batch > 65535.  The workspace query returns SVCMI_EINVAL (negative) for a geometry the launch would refuse.
 *   log_mel:    out[b][m][t] = log(max(sum_{k < bins} mel[m][k] * spec[b][k][t], clip)), TacotronSTFT.mel_spectrogram after the magnitude
 *               (stft.py:94-104, clip = 1e-5); spec [batch][bins][frames] (svcmi_linear_spectrogram_f32 with eps = 1e-9), out
 *               [batch][n_mel][frames], both contiguous.  The filterbank comes TRANSPOSED: melT[k][m], k < bins, row stride ldm floats,
 *               ldm >= n_mel rounded up to a multiple of 32, the columns m >= n_mel finite (zeros): a half-wave reads 32 consecutive
 *               floats.  On the fp32 matrix cores, every output one accumulator chain over k in ascending order.  SVCMI_EINVAL for a null
 *               pointer, batch / bins / frames / n_mel < 1, a smaller ldm, clip <= 0; SVCMI_EALIGN; SVCMI_EUNSUPPORTED for batch > 65535.
 *   abs_diff_sum: out[b] = sum_{i < count} |a[b][i] - b[b][i]| as a double (the mel L1 before its division); batch strides in floats
 *               (>= count).  A block sums 4096 consecutive elements in a fixed order into its own slot of `partials` (at least
 *               svcmi_abs_diff_sum_workspace_bytes(batch, count) = 4 * batch * ceil(count / 4096) bytes); the slots are added in ascending
 *               order in fp64.  Errors as stft_distance. */
int64_t svcmi_stft_distance_workspace_bytes(int32_t batch, int64_t n, int32_t n_fft, int32_t hop, int32_t pad);
int svcmi_stft_distance_f32(const float* x, int64_t x_bstride, const float* y, int64_t y_bstride, int32_t batch, int64_t n, const float* basis,
                            int32_t n_fft, int32_t hop, int32_t pad, float floor_, int64_t frames, float* partials, int64_t partials_bytes,
                            double* out, void* stream);
int svcmi_log_mel_f32(const float* spec, int32_t batch, int32_t bins, int64_t frames, const float* melT, int32_t ldm, int32_t n_mel, float clip,
                      float* out, void* stream);
int64_t svcmi_abs_diff_sum_workspace_bytes(int32_t batch, int64_t count);
int svcmi_abs_diff_sum_f32(const float* a, int64_t a_bstride, const float* b, int64_t b_bstride, int32_t batch, int64_t count, float* partials,
                           int64_t partials_bytes, double* out, void* stream);

/* CREPE F0 extractor glue (row N3; the six convolutions and the classifier are svcmi_conv_gemm_f32 launches):
 *   crepe_frames: crepe/core.py:664-703 -- frame f = samples [f*hop - 512, f*hop + 512) of the waveform (zeros outside
 *                 [0, n)), minus its mean, divided by max(1e-10, unbiased std).  Written as rows of `ld` (>= 1532, % 4 == 0)
 *                 floats: 254 zeros, the 1024 samples, zeros -- the zero padding of the first convolution (model.py:119),
 *                 placed so that its stride-4 / 512-tap window reads 16-byte aligned groups of 4 samples, i.e. the first
 *                 layer is a stride-1, 128-tap convolution over rows of 4 "channels".
 *   bn_maxpool2:  y[r, c] = max(x[2r, c], x[2r+1, c] as a' = a*scale[c] + shift[c]) -- eval-mode BatchNorm2d applied after
 *                 the ReLU, then max_pool2d((2,1)) (model.py:128-134); rows_out = rows_in / 2, rows never straddle frames
 *                 because every per-frame length is even. */
int svcmi_crepe_frames_f32(const float* audio, int64_t n, int32_t hop, int32_t frame0, int32_t frames, float* out, int32_t ld, void* stream);
int svcmi_bn_maxpool2_f32(const float* x, const float* scale, const float* shift, float* y, int64_t rows_out, int32_t c,
                          int32_t ldx, int32_t ldy, void* y16, int32_t ldy16, int32_t y16_format, void* stream);
/* (y16: optional 16-bit copy of the pooled rows for the next layer's SVCMI_PREC_*_A16 convolution, formats as for svcmi_layernorm_f32;
 * y may be NULL when y16 is given.) */
/* Viterbi decoding of the 360-bin pitch posteriorgram (crepe/decode.py:53-80; librosa.sequence.viterbi semantics: uniform
 * prior, log domain): prob [frames][360] = the network's sigmoid outputs; bins outside [minidx, maxidx) are excluded
 * (crepe/core.py:597-598); softmax over the rest in fp32, DP in fp64, independently per batch of `batch_frames` frames
 * (crepe/core.py:683-686).  log_trans: [360][360] doubles = log(transition + tiny).  band > 0 declares the matrix banded:
 * every entry with |i - j| > band equals log_trans[0][359] (CREPE's transition: band = 11); the DP then evaluates 2*band + 1
 * predecessors plus the best out-of-band one per state instead of all 360 (same result, ties to the lowest index).  band = 0:
 * dense.  lp_scratch: frames*360 floats, ptr_scratch: frames*360 int16.  path: [frames] decoded bins. */
int svcmi_viterbi_decode(const float* prob, const double* log_trans, float* lp_scratch, int16_t* ptr_scratch, int32_t* path,
                         int32_t frames, int32_t batch_frames, int32_t minidx, int32_t maxidx, int32_t band, void* stream);

/* Feature retrieval (row N4; feature_retrieval/index.py:57-94 -- faiss search_and_reconstruct + the RVC weighting):
 *   row_sqnorm: out[r] = sum_c x[r, c]^2 (the |b|^2 term of the bank, computed once per index).
 *   knn_blend:  for every query row i < t: the k (<= 8) stored vectors with the smallest squared L2 distance, ranked by
 *               |x|^2 + bank_sq[j] - 2*dots[i, j] with dots = X * Bank^T from svcmi_conv_gemm_f32 (ties -> smaller j);
 *               the 8 best-ranked candidates are re-measured as sum_c (x - b)^2 and the k nearest of those kept (so fp32
 *               cancellation in the ranking cannot swap near-equidistant neighbours), weight_q = (1/dist_q)^2 / sum_q' (1/dist_q')^2, and
 *               out[i, :] = (1 - ratio) * x[i, :] + ratio * sum_q weight_q * bank[nn_q, :].
 *               An exact search, i.e. faiss IVF-Flat with nprobe = nlist (the reference's nprobe = 1 is its approximation). */
int svcmi_row_sqnorm_f32(const float* x, int32_t ldx, int64_t rows, int32_t d, float* out, void* stream);
int svcmi_knn_blend_f32(const float* x, int32_t ldx, const float* bank, int32_t ldb, const float* dots, int64_t ldd,
                        const float* bank_sq, float* out, int32_t ldo, int32_t t, int32_t n, int32_t d, int32_t k,
                        float ratio, void* stream);

/* The reference's own index type: faiss IVF-Flat searched with nprobe = 1 (feature_retrieval/index.py:145-151 builds
 * index_factory("IVF{n},Flat", METRIC_L2) and sets nprobe = 1; :57-62 search_and_reconstruct; :163-166 read_index).  faiss 1.7.4 is
 * pinned by the reference's requirements.txt and not vendored; its published algorithm is restated (parity unpinned: no faiss here):
 *   ivf_assign:   coarse quantizer = IndexFlatL2 over the nlist centroids: assign[i] = argmin_j max(0, |x_i|^2 + cent_sq[j] -
 *                 2*dots[i, j]) with dots = X * Centroids^T from svcmi_conv_gemm_f32 (ties -> smaller j); dist (optional) = that
 *                 minimum.  Also the assignment step of the k-means that trains the centroids (Clustering.cpp).
 *   ivf_blend:    the inverted list of cell assign[i] = rows [list_off[a], list_off[a+1]) of `bank` (stored vectors grouped by cell,
 *                 insertion order inside a cell) is scanned with exact distances sum_c (x - b)^2; the k (<= 8) nearest, ascending (ties ->
 *                 earlier row), get weight (1/dist)^2 normalised and out[i] = (1 - ratio) * x[i] + ratio * sum_q weight_q * bank[nn_q].
 *                 A cell with fewer than k vectors uses the ones it has, an empty cell leaves x[i] unchanged (faiss pads with label -1
 *                 and a NaN reconstruction there, which makes the reference emit a NaN frame).  out_idx [t][k] (optional): the chosen
 *                 rows of `bank`, -1 padded; out_dist [t][k] (optional): their distances, +inf padded.
 *   segment_mean: k-means centroid update: out[c] = mean of x[order[r]], r in [seg_off[c], seg_off[c+1]), summed in that order;
 *                 an empty segment leaves out[c] untouched. */
int svcmi_ivf_assign_f32(const float* x, int32_t ldx, const float* dots, int64_t ldd, const float* cent_sq, int32_t t,
                         int32_t nlist, int32_t d, int32_t* assign, float* dist, void* stream);
int svcmi_ivf_blend_f32(const float* x, int32_t ldx, const int32_t* assign, const int32_t* list_off, const float* bank,
                        int32_t ldb, float* out, int32_t ldo, int32_t t, int32_t d, int32_t k, float ratio,
                        int32_t* out_idx, float* out_dist, void* stream);
int svcmi_segment_mean_f32(const float* x, int32_t ldx, const int32_t* order, const int32_t* seg_off, float* out, int32_t ldo,
                           int32_t segments, int32_t d, void* stream);

/* int16 side output, vits_decoder/generator.py:167-173: clamp(32768*x, -32768, 32767) truncated to short. */
int svcmi_source2wav_i16(const float* x, int16_t* y, int64_t n, void* stream);


/* =============================================================================================
 * Stage-level entry points: the composition of the kernels above into the
 * reference's forward passes, done by a C++ host INSIDE this library -- no Python in the loop, so a
 * non-Python caller can run a stage, and the Python facade (svcmi.SynthesizerInfer.inference,
 * svcmi.whisper AudioEncoder) is one ctypes call per stage.
 *
 * Models are plain structs of DEVICE pointers to operands already in the packed layouts the kernels
 * take (weight-norm folded, Conv1d [N,Cin,K] -> [N][K*Cin], ConvTranspose1d polyphase, q|k|v fused,
 * Flip folded into permutations: svcmi/weights.py does this once at load; `python -m svcmi.tools
 * pack` writes the same arena to a file a non-Python host can mmap / upload).  The structs are read
 * on the host during the call only.
 *
 * Memory: every intermediate lives in ONE caller-owned device workspace; svcmi_*_workspace_bytes
 * runs the same allocation plan without launching and returns the size needed for a shape.  Nothing
 * is allocated, nothing synchronises, every launch goes to `stream`: a call can be captured into a
 * hipGraph.  Return value as above (first failing launch aborts the stage).
 */
#define SVCMI_MAX_WHISPER_BLOCKS 32
#define SVCMI_MAX_ENC_LAYERS 8
#define SVCMI_MAX_FLOWS 8
#define SVCMI_MAX_WN_LAYERS 8
#define SVCMI_MAX_STAGES 6
#define SVCMI_MAX_AMP_BLOCKS 3
#define SVCMI_MAX_AMP_DILATIONS 3

/* one packed GEMM operand: w [n][ldw] fp32 as svcmi_conv_gemm_f32 takes it; bias [n] or NULL; w16 = the svcmi_pack_weights_lp
 * image for the model's `precision` (NULL = this layer always runs fp32), ldw16 its leading dimension */
typedef struct svcmi_weight {
    const float* w;
    const float* bias;
    const void* w16;
    const void* w16a;     /* the natural-k-order image of the SVCMI_PREC_*_A16 kernels (same ldw16), or NULL: 16-bit activations are not used here */
    int32_t n, ldw, ldw16;
    int32_t prec16;       /* enum svcmi_precision the w16 / w16a images were packed for (0 = unknown: trusted to match the model's mode); a launch
                           * whose mode differs runs on the fp32 operand instead of misreading the image */
} svcmi_weight;

/* ---- Whisper audio encoder, truncated as whisper/inference.py:11-29 does (n_layers = the kept blocks) */
typedef struct svcmi_whisper_block {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;     /* attn_ln, mlp_ln (whisper/model.py:113-116) */
    svcmi_weight qkv, o, m1, m2;                    /* q|k|v fused [3S][S] (key has no bias: zeros), out, mlp.0, mlp.2 */
} svcmi_whisper_block;

typedef struct svcmi_whisper_model {
    int32_t n_state, n_heads, n_layers, n_mels, n_ctx;
    int32_t precision;                              /* enum svcmi_precision of the linear layers (w16 images must match) */
    svcmi_weight conv1, conv2;                      /* whisper/model.py:144-145 */
    const float* pos;                               /* positional_embedding [n_ctx][n_state] */
    const float *lnp_g, *lnp_b;                     /* ln_post */
    svcmi_whisper_block blocks[SVCMI_MAX_WHISPER_BLOCKS];
    /* tuning (0 = the library's table for MI355X): K slices of the two N = n_state projections and tile overrides (>> 8) for
     * single windows (M <= small_m_rows rows); batched windows use the heuristic of svcmi_conv_gemm_f32 */
    int32_t split_o, split_mlp, tile_qkv, tile_o, tile_mlp1, tile_mlp2, small_m_rows, reserved;
    float lp_min_flops;                             /* launches below this stay fp32 in a 16-bit mode (0 = 1.5e9) */
    int32_t reserved2;
} svcmi_whisper_model;

int64_t svcmi_whisper_workspace_bytes(const svcmi_whisper_model* m, int32_t batch, int32_t n_frames);
/* AudioEncoder.forward, whisper/model.py:147-163, on mel [batch][n_mels][n_frames] (the reference's NCL layout) with the
 * `mel + noise_scale * noise` of whisper/inference.py:46,58 fused into the layout change (noise: same layout, or NULL):
 * conv1 + GELU, conv2 (stride 2) + GELU, + positional_embedding, n_layers x ResidualAttentionBlock (:118-129), ln_post.
 * out: [batch][tw][n_state] time-major, tw = (n_frames - 1) / 2 + 1 <= n_ctx (else SVCMI_EINVAL: "incorrect audio shape", :156). */
int svcmi_whisper_encoder_fwd(const svcmi_whisper_model* m, const float* mel, const float* noise, float noise_scale,
                              int32_t batch, int32_t n_frames, float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- LSTMSpeakerEncoder (speaker/models/lstm.py:35-71, use_lstm_with_projection = True): n_layers x [nn.LSTM(d_in, lstm_dim) +
 * Linear(lstm_dim, proj_dim, bias=False)], the last time step of the last layer L2-normalised.  fp32 only. */
#define SVCMI_MAX_LSTM_LAYERS 8
typedef struct svcmi_lstm_layer {
    svcmi_weight ih;                                /* W_ih [4H][d_in] with bias = b_ih + b_hh, rows in the tile order of svcmi_lstm_step_f32 */
    svcmi_weight lin;                               /* linear.weight [proj_dim][H], no bias */
    const float* whh;                               /* W_hh [4H][H], rows in tile order */
    const void* reserved;
} svcmi_lstm_layer;
typedef struct svcmi_speaker_model {
    int32_t input_dim, lstm_dim, proj_dim, n_layers;
    svcmi_lstm_layer layers[SVCMI_MAX_LSTM_LAYERS];
} svcmi_speaker_model;

int64_t svcmi_speaker_encoder_workspace_bytes(const svcmi_speaker_model* m, int32_t batch, int32_t t);
/* LSTMSpeakerEncoder.inference on mel [batch][t][input_dim] -> emb [batch][proj_dim].  Per layer: one GEMM for the input projections of
 * all t steps, t launches of svcmi_lstm_step_f32, one GEMM for the output projection (the last layer projects only row t - 1); then
 * svcmi_l2norm_rows_f32.  Checked before anything is launched: SVCMI_EINVAL for a null pointer, batch < 1, t < 1, n_layers outside
 * 1..SVCMI_MAX_LSTM_LAYERS, a workspace that is too small or not 256-byte aligned; SVCMI_EUNSUPPORTED for batch > 64 (the caller loops);
 * SVCMI_EALIGN for lstm_dim / input_dim / proj_dim % 4 or a W_hh that is not 16-byte aligned. */
int svcmi_speaker_encoder_fwd(const svcmi_speaker_model* m, const float* mel, int32_t batch, int32_t t, float* emb, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ---- Silero voice-activity detector (vad/utils.py, the 16 kHz model of vad/assets/silero_vad.jit; svc_inference_post.py).  Added under
 * ABI 22: purely additive.  fp32 only.  Per window of 512 samples: reflect pad by 96 inside the window, 8 STFT frames (258 basis rows of
 * 256 taps, hop 64), magnitude, log1p(2^20 mag) minus its smoothed mean, four ConvBlocks relu(pw(relu(dw(x))) + res(x)) (depthwise k = 5)
 * of 258 -> 16 -> 32 -> 32 -> 64 channels, each followed by a 1x1 convolution (stride 2, 2, 2, 1) + BatchNorm + ReLU: one 64-vector;
 * then ONE step of a 2-layer LSTM(64, 64) (gate order i, f, g, o) whose state runs from window to window, and
 * p = sigmoid(dec_w . relu(h of layer 1) + dec_b). */
typedef struct svcmi_vad_conv_block {
    const float *dw_w, *dw_b;                       /* depthwise [c_in][5], [c_in] */
    const float *pw_w, *pw_b;                       /* pointwise [c_out][c_in], [c_out] */
    const float *proj_w, *proj_b;                   /* residual 1x1 [c_out][c_in], [c_out]; both NULL = identity (c_in == c_out) */
    int32_t c_in, c_out;
} svcmi_vad_conv_block;
typedef struct svcmi_vad_down {
    const float *w, *b;                             /* 1x1 convolution [c][c], [c] */
    const float *scale, *shift;                     /* BatchNorm in eval mode: scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale */
    int32_t c, stride;
} svcmi_vad_down;
typedef struct svcmi_vad_model {
    const float* basis_t;                           /* the STFT basis TRANSPOSED: [256 taps][260], column r < 258 = basis row r */
    const float* filt;                              /* the normaliser's 7 smoothing taps */
    svcmi_vad_conv_block block[4];                  /* 258 -> 16, 16 -> 32, 32 -> 32, 32 -> 64 */
    svcmi_vad_down down[4];                         /* strides 2, 2, 2, 1 */
    const float *gate0_w, *gate0_b;                 /* W_ih of LSTM layer 0 [256][64] and b_ih + b_hh [256] */
    const float *whh0_t, *wih1_t, *whh1_t;          /* W_hh0, W_ih1, W_hh1 TRANSPOSED: [64][256] (element [k][j] = row j, column k) */
    const float* gate1_b;                           /* b_ih + b_hh of layer 1 [256] */
    const float* dec_w;                             /* [64] */
    float dec_b;
    int32_t reserved;
} svcmi_vad_model;
int64_t svcmi_vad_model_bytes(void);                /* sizeof(svcmi_vad_model), for a binding's layout check */

/* The three kernels (csrc/vad.hip).  Recordings: `batch` mono 16 kHz signals inside one buffer, recording b = audio[offsets[b] ..
 * offsets[b] + lengths[b]); offsets / lengths are DEVICE arrays of int64.  Recording b has W_b = min(wmax, ceil(lengths[b] / 512))
 * windows, the last one zero-padded on the right.  feat [batch][wmax][64], gates [batch][wmax][256], probs [batch][wmax]: rows
 * w >= W_b are not written.
 *   vad_frontend:  everything in front of the LSTM, one block per window: feat = the 64-vector, gates = W_ih0 feat + b_ih0 + b_hh0.
 *                  Every sum is one chain in ascending index order, no atomics: a window's bits depend on its 512 samples and the
 *                  weights alone, not on the run, on wmax or on the batch.
 *   vad_lstm_scan: both LSTM layers and the decoder over a recording's W_b windows, one block per recording (recordings of different
 *                  lengths each scan their own W_b; no block waits for another).  state: NULL = start from zero; else
 *                  [batch][4][64] = h0, c0, h1, c1, read at the start and overwritten with the state after the last window.
 *                  Saturated gates give exactly 0 / 1, never NaN.
 *   mask_spans:    out[i] = in[i] if some span s has spans[s][0] * ratio <= i < spans[s][1] * ratio, else 0, for
 *                  i < n_out = min(n_in, ratio * n_ref) (svc_inference_post.py:39-49 with ratio = 2).  spans: device int32
 *                  [n_spans][2], sorted and disjoint; n_spans = 0 (spans may be NULL) zeroes everything.
 * SVCMI_EINVAL before anything is launched for a null pointer (model members included), batch < 1, wmax < 1, n_in / n_ref / ratio < 1,
 * n_spans < 0, another n_out; SVCMI_EUNSUPPORTED for channel counts or strides other than the architecture above, batch > 65535;
 * SVCMI_EALIGN for a pointer that is not aligned to its element. */
int svcmi_vad_frontend_f32(const svcmi_vad_model* m, const float* audio, const int64_t* offsets, const int64_t* lengths, int32_t batch,
                           int32_t wmax, float* feat, float* gates, void* stream);
int svcmi_vad_lstm_scan_f32(const svcmi_vad_model* m, const float* gates, const int64_t* lengths, int32_t batch, int32_t wmax, float* state,
                            float* probs, void* stream);
int svcmi_mask_spans_f32(const float* in, int64_t n_in, const int32_t* spans, int32_t n_spans, int64_t n_ref, int32_t ratio, float* out,
                         int64_t n_out, void* stream);
/* The two launches on one workspace: probs [batch][wmax] (rows w >= W_b not written).  The workspace holds feat and gates:
 * svcmi_vad_workspace_bytes(batch, wmax) = 1280 * batch * wmax + 256 bytes (SVCMI_EINVAL for batch or wmax < 1).  SVCMI_EINVAL also for a
 * workspace that is too small or not 256-byte aligned. */
int64_t svcmi_vad_workspace_bytes(int32_t batch, int32_t wmax);
int svcmi_vad_probs_fwd(const svcmi_vad_model* m, const float* audio, const int64_t* offsets, const int64_t* lengths, int32_t batch,
                        int32_t wmax, float* state, float* probs, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Salience F0 extractor (pitch/inference.py:31-44 compute_f0_salience -> pitch/core/salience.py).  Added under ABI 22: purely
 * additive.  fp32 / fp64 only.  A centred STFT (zero padding, window folded into the table) restricted to the bins whose
 * instantaneous frequency can fall into [f_min, f_max); per frame the heterodyned phase increment gives every bin an instantaneous
 * frequency, its power |X|^2 is added into the log-frequency bin floor(bins_per_octave log2(f / f_min) + 0.5) (ascending STFT bin per
 * log-frequency bin: a fixed order, no floating-point atomics), the column is smoothed along frequency, thresholded against the
 * global maximum, summed over harmonics and thresholded again; then ONE dynamic programme over the whole clip in fp64.
 * The plan is made by the host (svcmi/pitch/core/salience.py salience_plan); every pointer is a DEVICE pointer. */
typedef struct svcmi_salience_plan {
    const float* basis;                             /* [n_fft][2 n_bins]: column 2j = w[i] cos(2 pi (k_lo + j) i / n_fft), 2j + 1 = -w[i] sin(..), made in float64 */
    const float* smooth;                            /* the smoothing taps [smooth_len] (symmetric, odd length) */
    const int32_t* harm_off;                        /* harmonic summation, sparse: z[b] = sum_m harm_w[m] lf[b + harm_off[m]], m ascending */
    const float* harm_w;                            /* [n_harm] */
    int32_t n_fft, hop, k_lo, n_bins;               /* STFT bins k_lo .. k_lo + n_bins - 1 of n_fft / 2 + 1 */
    int32_t n_pitch, smooth_len, n_harm, tol;       /* B log-frequency bins; |i - j| <= tol is the cheap transition */
    float fs, f_min, f_max, bins_per_octave;        /* 1200 / R */
    double thresh;                                  /* 10^(gamma / 20): a cell stays iff v / max + 2^-23 < thresh (a NaN quotient, max = 0, zeroes it) */
    double log_hi, log_lo;                          /* log(score_high + 2^-23), log(score_low + 2^-23) */
} svcmi_salience_plan;
int64_t svcmi_salience_plan_bytes(void);            /* sizeof(svcmi_salience_plan), for a binding's layout check */
#define SVCMI_SALIENCE_MAX_BINS 1024                /* n_bins, n_pitch and tol may not exceed this */

/* The kernels (csrc/salience.hip).  frames = 1 + n / hop throughout, at least 2 (the phase increment needs a neighbour).
 *   salience_stft: X [frames][n_bins] complex64 (re, im interleaved) of x zero-padded by n_fft / 2 on both sides (index arithmetic on the
 *                  load).  On the fp32 matrix cores, every output one accumulator chain over the taps in ascending order: the bits
 *                  depend on the frame's n_fft padded samples and the table alone, not on the tile, the frame count or the stream.
 *   salience_map:  X -> lf [frames][n_pitch] (the smoothed, thresholded log-frequency spectrogram) and z [frames][n_pitch] (the
 *                  salience map), both time-major.  gmax: two 32-bit words of scratch; afterwards the bit patterns of max(lf) and
 *                  max(z) BEFORE thresholding (integer atomic max on non-negative floats: order-independent).  Frame 0 takes frame
 *                  1's instantaneous frequencies.  An all-zero X gives all-zero maps, no NaN.
 *   salience_dp:   z [frames][n_pitch] -> path int32 [frames]: D[b, 0] = log(z[0][b] + 2^-23), D[b, t] = max_j(T[b, j] + D[j, t - 1]) +
 *                  log(z[t][b] + 2^-23) with T = log_hi for |b - j| <= tol, else log_lo, in fp64; every predecessor is evaluated, the
 *                  lowest index wins a tie (numpy's argmax).  One block per clip.  ptr: int16 [frames][n_pitch] scratch.
 * SVCMI_EINVAL before anything is launched for a null pointer (plan members included), frames < 2 or != 1 + n / hop, n < 1, hop < 1, an odd
 * n_fft (or < 2), a bin range outside 0 .. n_fft / 2, n_pitch / n_harm < 1, an even smooth_len, tol < 0; SVCMI_EUNSUPPORTED for n_bins,
 * n_pitch or tol above SVCMI_SALIENCE_MAX_BINS, smooth_len > 65, frames >= 2^31 / n_pitch; SVCMI_EALIGN for a pointer that is not aligned to
 * its element (X: 8 bytes). */
int svcmi_salience_stft_f32(const svcmi_salience_plan* p, const float* x, int64_t n, float* X, int64_t frames, void* stream);
int svcmi_salience_map_f32(const svcmi_salience_plan* p, const float* X, int64_t frames, float* lf, float* z, uint32_t* gmax, void* stream);
int svcmi_salience_dp_f64(const float* z, int64_t frames, int32_t n_pitch, int32_t tol, double log_hi, double log_lo, int16_t* ptr,
                          int32_t* path, void* stream);
/* waveform -> path as ONE stage call on one workspace (X, lf, the back pointers, gmax; z too when the caller passes NULL for it).
 * SVCMI_EINVAL also for a workspace that is too small or not 256-byte aligned; the query returns a negative code for a geometry the
 * stage would refuse. */
int64_t svcmi_salience_workspace_bytes(const svcmi_salience_plan* p, int64_t n);
int svcmi_salience_f0_fwd(const svcmi_salience_plan* p, const float* x, int64_t n, int32_t* path, float* z, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- pYIN F0 extractor (pitch/core/pyin.py, libf0's pYIN: the network-free extractor that decides voicing).  Added under ABI 22: purely
 * additive.  fp64 throughout (the clip is fp32 and widens exactly).  Per frame YIN's cumulative mean normalised difference function
 * (CMNDF) over the lags 1 .. p_max, n_thr thresholds weighted by a beta distribution into one observation column over n_pitch voiced
 * and n_pitch unvoiced states, then ONE Viterbi pass over the clip and the refinement of every voiced frame by the closest per-threshold
 * YIN estimate.  The device reproduces the reference as it executes under numpy, defects included.
 * The plan is made by the host (svcmi/pitch/core/pyin.py pyin_plan); every pointer is a DEVICE pointer. */
typedef struct svcmi_pyin_plan {
    const double* thresholds;                       /* [n_thr], ascending */
    const double* beta;                             /* [n_thr]: the beta-binomial weight of every threshold */
    const double* f_axis;                           /* [n_pitch]: f_min 2^(b R / 1200) */
    const double* band;                             /* [n_pitch][2 max_step + 1]: band[i][d] = log(A[i - max_step + d][i] + tiny), the voiced block of
                                                       the transition matrix gathered by COLUMN (the unvoiced block is the same); entries whose
                                                       row lies outside 0 .. n_pitch - 1 are never read */
    int32_t n_fft, hop, p_min, p_max;               /* frame length (even), hop, max(ceil(fs / f_max), 1), ceil(fs / f_min) <= n_fft */
    int32_t n_pitch, n_thr, max_step, reserved;
    double fs, tol_cents;                           /* sampling rate; the refinement's tolerance R in cents */
    double absolute_min_prob, voicing_prob;
    double log_tiny, log_cross, log_c, tiny;        /* log(tiny), log(0.01 + tiny) (voiced <-> unvoiced), log(1 / (2 n_pitch) + tiny), tiny = 2^-1022 */
} svcmi_pyin_plan;
int64_t svcmi_pyin_plan_bytes(void);                /* sizeof(svcmi_pyin_plan), for a binding's layout check */
#define SVCMI_PYIN_MAX_BINS 1024                    /* n_pitch */
#define SVCMI_PYIN_MAX_THRESHOLDS 128               /* n_thr */
#define SVCMI_PYIN_MAX_NFFT 4096                    /* p_max <= n_fft <= this */
#define SVCMI_PYIN_MAX_BAND 33                      /* 2 max_step + 1 */

/* The kernels (csrc/pyin.hip).  frames = 1 + n / hop for a clip of n samples.
 *   pyin_cmndf:   x [n] fp32 -> cmndf [frames][p_max + 1] and rms [frames].  Frame m covers the samples m hop - n_fft / 2 .. + n_fft - 1 of
 *                 x (zeros outside).  d(tau) = sum_j (x[j] - x[j + tau])^2 in its direct form, one fixed accumulation order per (frame,
 *                 tau): the bits depend on the frame's samples alone.  cmndf[0] = 1; silence gives exact zeros, no NaN.  frames >= 2.
 *   pyin_observe: cmndf rows -> O [frames][2 n_pitch] (time-major: the voiced half times voicing_prob, then the unvoiced constant of the
 *                 frame), logO = log(O + tiny) (may be NULL), lag_thr and val_thr [frames][n_thr].  frames >= 1.
 *   pyin_viterbi: logO [frames][2 n_pitch] -> path int32 [frames], numpy's argmax index for index: D[i, 0] = log_c + logO[0][i],
 *                 D[i, t] = max_j(logA[j][i] + D[j, t - 1]) + logO[t][i], logA = band / log_cross where the matrix is not zero and
 *                 log_tiny everywhere else; the lowest index wins among equal ROUNDED sums.  One block per clip.  ptr: int16
 *                 [frames][2 n_pitch] scratch.  logO must not hold NaN.  frames >= 2.
 *   pyin_finish:  path, O, rms, lag_thr, val_thr -> f0 and conf [frames].  frames >= 1.
 * SVCMI_EINVAL before anything is launched for a null pointer (plan members included; logO of pyin_observe excepted), too few frames or
 * frames != 1 + n / hop, n < 1, hop < 1, an odd n_fft (or < 2), p_min < 1, p_max < p_min, n_pitch / n_thr / max_step < 1,
 * n_pitch < 2 max_step + 1, fs / tol_cents / tiny <= 0, voicing_prob outside 0 .. 1; SVCMI_EUNSUPPORTED for n_pitch, n_thr, n_fft or
 * 2 max_step + 1 above the limits, p_max > n_fft, frames >= 2^31 / (row length); SVCMI_EALIGN for a pointer that is not aligned to its
 * element. */
int svcmi_pyin_cmndf_f64(const svcmi_pyin_plan* p, const float* x, int64_t n, double* cmndf, double* rms, int64_t frames, void* stream);
int svcmi_pyin_observe_f64(const svcmi_pyin_plan* p, const double* cmndf, int64_t frames, double* O, double* logO, double* lag_thr,
                           double* val_thr, void* stream);
int svcmi_pyin_viterbi_f64(const double* logO, int64_t frames, int32_t n_pitch, int32_t max_step, const double* band, double log_tiny,
                           double log_cross, double log_c, int16_t* ptr, int32_t* path, void* stream);
int svcmi_pyin_finish_f64(const svcmi_pyin_plan* p, const int32_t* path, const double* O, const double* rms, const double* lag_thr,
                          const double* val_thr, int64_t frames, double* f0, double* conf, void* stream);
/* clip -> f0, conf [frames] float64 and path int32 [frames] as ONE stage call on one workspace (the CMNDF rows, logO, the back pointers,
 * and whichever of rms [frames], O [frames][2 n_pitch], lag_thr, val_thr [frames][n_thr] the caller passes NULL for).  SVCMI_EINVAL also
 * for a workspace that is too small or not 256-byte aligned; the query returns a negative code for a geometry the stage would refuse. */
int64_t svcmi_pyin_workspace_bytes(const svcmi_pyin_plan* p, int64_t n);
int svcmi_pyin_f0_fwd(const svcmi_pyin_plan* p, const float* x, int64_t n, double* f0, double* conf, int32_t* path, double* rms, double* O,
                      double* lag_thr, double* val_thr, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- YIN F0 extractor (pitch/core/yin.py, libf0's YIN: pYIN's front half without the threshold sweep and the HMM; the one extractor that
 * reports an aperiodicity per frame, a continuous voicing measure).  Added under ABI 22: purely additive.  fp64 throughout (the clip is
 * fp32 and widens exactly).  Per frame the CMNDF over the lags 0 .. lag_max -- pYIN's kernel, the same bits --, the first strict local
 * minimum below the threshold with its parabolic refinement, a second search inside +/- 25 cents of it, f0 = fs / lag, and the
 * aperiodicity of the frame at that lag.  The device reproduces the reference as it executes under numpy.  The plan is
 * plain data made by the host (svcmi/pitch/core/yin.py yin_plan): it holds no pointer. */
typedef struct svcmi_yin_plan {
    int32_t n_fft, hop, lag_min, lag_max;           /* frame length (even), hop, max(ceil(fs / f_max), 1), ceil(fs / f_min) <= n_fft */
    double fs, threshold;                           /* sampling rate; the absolute threshold on the CMNDF (+inf is allowed: every minimum qualifies) */
    double ratio_up, ratio_down;                    /* 2^(25 / 1200), 2^(-25 / 1200): the refinement window's two factors as the host computes them */
} svcmi_yin_plan;
int64_t svcmi_yin_plan_bytes(void);                 /* sizeof(svcmi_yin_plan), for a binding's layout check */
#define SVCMI_YIN_MAX_NFFT 4096                     /* lag_max <= n_fft <= this */

/* The kernels (csrc/yin.hip).  frames = 1 + n / hop for a clip of n samples; one frame is enough.
 *   yin_cmndf:        x [n] fp32 -> cmndf [frames][lag_max + 1], bit for bit the rows of svcmi_pyin_cmndf_f64 at p_max = lag_max (it is that
 *                     kernel), and rms [frames], which the kernel writes as well (YIN does not use it).
 *   yin_pick:         cmndf rows -> lag [frames]; f0 = fs / lag, lag_first (the first search's result) and kind int32 [frames] may be NULL.
 *                     A search over [lo, hi): lo == hi gives lo; else the first i in [lo, hi) with c[i] < c[i - 1], c[i] < c[i + 1] and
 *                     c[i] < threshold, moved by -b / (2 a), a = eps + (y1 + y3 - 2 y2) / 2, b = (y3 - y1) / 2, eps = 2^-52, and c[i] replaced
 *                     by y2 - b^2 / (4 a) in the kernel's copy of the row; else the lowest index of the smallest c[lo .. hi - 1], an
 *                     integer.  First over [lag_min, lag_max) with the plan's threshold; then with threshold = +inf over
 *                     [rint(fs / ((fs / lag) ratio_up)), rint(fs / ((fs / lag) ratio_down))), half to even, clipped to lag_min .. lag_max.
 *                     kind: 1 = the first search took the lowest-value branch, 2 = the second returned its lower limit because the window
 *                     was empty, 4 = the second took the lowest-value branch.  The rows are not modified.  They must not hold NaN or inf.
 *   yin_aperiodicity: x, lag [frames] -> ap [frames] = res / (pwr + eps): with f the frame, g = (f, f reversed) and s[j] = g[L + j]
 *                     (L = floor(lag); a lag without fractional part) or (1 - frac) g[L + j] + frac g[L + 1 + j], pwr = (mean f^2 +
 *                     mean s^2) / 2, res = mean (f - s)^2 / 2.  The three sums in one fixed order per frame: the bits depend on the
 *                     frame's samples and the lag alone.  Silence gives exactly 0.  0 <= lag <= n_fft, a fractional one < n_fft; the
 *                     kernel reads nothing outside the frame whatever the lag holds.
 * SVCMI_EINVAL before anything is launched for a null pointer (the optional outputs excepted), n < 1, frames < 1 or frames != 1 + n / hop,
 * hop < 1, an odd n_fft (or < 2), lag_min < 1, lag_max < lag_min, fs <= 0, a NaN threshold, a ratio <= 0; SVCMI_EUNSUPPORTED for n_fft above
 * the limit, lag_max > n_fft, frames >= 2^31 / (lag_max + 1); SVCMI_EALIGN for a pointer that is not aligned to its element. */
int svcmi_yin_cmndf_f64(const svcmi_yin_plan* p, const float* x, int64_t n, double* cmndf, double* rms, int64_t frames, void* stream);
int svcmi_yin_pick_f64(const svcmi_yin_plan* p, const double* cmndf, int64_t frames, double* lag, double* f0, double* lag_first, int32_t* kind,
                       void* stream);
int svcmi_yin_aperiodicity_f64(const svcmi_yin_plan* p, const float* x, int64_t n, const double* lag, int64_t frames, double* ap, void* stream);
/* clip -> f0, ap [frames] float64 as ONE stage call: three launches on one workspace (the CMNDF rows, the rms the first kernel writes, and
 * lag when the caller passes NULL for it), nothing waits.  lag, lag_first float64 [frames] and kind int32 [frames] may be NULL.
 * SVCMI_EINVAL also for a workspace that is too small or not 256-byte aligned; the query returns a negative code for a geometry the
 * stage would refuse. */
int64_t svcmi_yin_workspace_bytes(const svcmi_yin_plan* p, int64_t n);
int svcmi_yin_f0_fwd(const svcmi_yin_plan* p, const float* x, int64_t n, double* f0, double* ap, double* lag, double* lag_first, int32_t* kind,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* ---- SWIPE' F0 extractor (pitch/core/swipe_slim.py, libf0's swipe_slim: the spectral one of the network-free extractors; it reports a
 * pitch strength per frame).  Added under ABI 22: purely additive.  Per window size N (a power of two, hop N / 2) the magnitudes of a
 * centred Hann STFT are resampled onto n_log log-frequency bins by a cubic spline -- a fixed linear map W_N the host tabulates --, every
 * column is normalised and correlated with the kernel rows K_N of that window's candidates; the windows' strengths are interpolated
 * linearly in time onto ceil(n / hop) output frames and summed with a weight per (window, candidate); the arg-max per frame is refined by
 * a parabola.  fp32 on the matrix cores, the finish in float64.  The device reproduces the reference's two edge defects (DESIGN.md
 * 4.11).  The plan is made by the host (svcmi/pitch/core/swipe_slim.py swipe_plan); every pointer is a DEVICE pointer.  Table rows are
 * zero-padded to a multiple of 8 floats: ld(v) = (v + 7) & ~7. */
#define SVCMI_SWIPE_MAX_WINDOWS 8
#define SVCMI_SWIPE_MAX_NFFT 4096
#define SVCMI_SWIPE_MAX_LOGBINS 1024                /* n_log */
#define SVCMI_SWIPE_MAX_CANDIDATES 1024             /* n_pitch */
typedef struct svcmi_swipe_window {
    const float* basis;                             /* [n_fft][2 (n_fft / 2 + 1)]: hann[i] cos(2 pi i k / n_fft) at column 2k, -hann[i] sin(..) at 2k + 1 */
    const float* resample;                          /* W_N [n_log][ld(n_fft / 2 + 1)]: the cubic spline from the linear to the log axis */
    const float* kernels;                           /* K_N [n_cand][ld(n_log)]: the kernel rows of this window's candidates */
    const int32_t* cand;                            /* [n_cand]: the candidate index of every row, strictly ascending, < n_pitch */
    const float* mu;                                /* [n_cand]: 1 - |err - octave| */
    int32_t n_fft, n_cand;
} svcmi_swipe_window;
typedef struct svcmi_swipe_plan {
    svcmi_swipe_window win[SVCMI_SWIPE_MAX_WINDOWS]; /* ascending n_fft: the order in which the strengths are summed */
    int32_t n_win, hop, n_log, n_pitch;             /* windows, output hop H, log-frequency bins, pitch candidates B */
    double f_min, step, threshold;                  /* F_min; R / 1200 (octaves per candidate); strength_threshold */
} svcmi_swipe_plan;
int64_t svcmi_swipe_plan_bytes(void);               /* sizeof(svcmi_swipe_plan), for a binding's layout check */

/* The kernels (csrc/swipe.hip).  For a clip of n samples window w has 1 + (n + N) / (N / 2) frames (svcmi_swipe_frames(p, w, n)) and the
 * output has ceil(n / hop) (window = -1).
 *   swipe_mag:      x [n] fp32 -> Y [frames_w][ld(N / 2 + 1)]: |STFT| of x padded with N zeros at the end, centred (N / 2 zeros in front,
 *                   index arithmetic), Hann, hop N / 2, all N / 2 + 1 bins; the pad columns are written as zeros.  One ascending
 *                   accumulation chain per output: the bits depend on the frame's samples alone.
 *   swipe_resample: Y -> L [frames][ld(n_log)] = W_N Y per frame (pad columns zero), one fixed accumulation order per output.
 *   swipe_strength: L -> SN [frames][n_cand] = K_N L / (sqrt(sum_f L^2) + eps) per frame, eps = 2^-52; the norm in one fixed order.
 *   swipe_accum:    SN of all windows back to back (window w at the float offset sum_{v < w} frames_v n_cand_v) -> S [ceil(n / hop)][n_pitch]:
 *                   S[j][cand[c]] = sum over the windows in ascending order of mu[c] (s0 + w (s1 - s0)), the two frames around j hop / (N / 2).
 *   swipe_finish:   S [frames][n_pitch] -> f0, conf float64 [frames], amax int32 [frames] (may be NULL), flags uint32 [1].  Arg-max with
 *                   the lowest index on ties; S[i - 1] at i = 0 is S[n_pitch - 1] (numpy's wrap); shift = -b / (2 a), a = eps + (y1 + y3 -
 *                   2 y2) / 2, b = (y3 - y1) / 2; f0 = f_min 2^(step (i + shift)), 0 where conf = S[i] < threshold.  A frame whose arg-max
 *                   is n_pitch - 1 takes shift 0 and adds 1 to flags[0] (zeroed first): the reference raises IndexError for such a clip.
 *                   S must not hold NaN.
 * SVCMI_EINVAL before anything is launched for a null pointer (plan members included), n < 1, frames < 1, a window index outside the
 * plan, n_win outside 1 .. 8, n_fft no power of two in 8 .. 4096, n_log outside 2 .. 1024, n_pitch outside 1 .. 1024, n_cand outside
 * 1 .. n_pitch, hop < 1, f_min or step <= 0, a NaN threshold; SVCMI_EALIGN for a pointer that is not aligned to its element (16 bytes
 * for resample, kernels, Y and L); SVCMI_EUNSUPPORTED for n >= 2^31 - 16384. */
int64_t svcmi_swipe_frames(const svcmi_swipe_plan* p, int32_t window, int64_t n);
int svcmi_swipe_mag_f32(const svcmi_swipe_plan* p, int32_t window, const float* x, int64_t n, float* Y, void* stream);
int svcmi_swipe_resample_f32(const svcmi_swipe_plan* p, int32_t window, const float* Y, int64_t frames, float* L, void* stream);
int svcmi_swipe_strength_f32(const svcmi_swipe_plan* p, int32_t window, const float* L, int64_t frames, float* SN, void* stream);
int svcmi_swipe_accum_f32(const svcmi_swipe_plan* p, const float* SN, int64_t n, float* S, void* stream);
int svcmi_swipe_finish_f64(const float* S, int64_t frames, int32_t n_pitch, int32_t n_log, double f_min, double step, double threshold,
                           double* f0, double* conf, int32_t* amax, uint32_t* flags, void* stream);
/* clip -> f0, conf float64 [ceil(n / hop)] and the flag word as ONE stage call on one workspace (Y and L of the largest window, every
 * window's SN, and S when the caller passes NULL for it): 3 launches per window, then accum, zero, finish.  SVCMI_EINVAL also for a
 * workspace that is too small or not 256-byte aligned; the query returns a negative code for a geometry the stage would refuse. */
int64_t svcmi_swipe_workspace_bytes(const svcmi_swipe_plan* p, int64_t n);
int svcmi_swipe_f0_fwd(const svcmi_swipe_plan* p, const float* x, int64_t n, double* f0, double* conf, float* S, uint32_t* flags,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---- SynthesizerInfer (vits/models.py:211-256) */
/* layer classes of the per-layer mixed-precision policy: prior encoder (enc_p: pre / hub / attention + FFN layers / proj, and its attention
 * kernel), flow (pre / in / res_skip / post of every coupling layer), the generator's trunk (conv_pre + every ups[i]), and the AMP-block
 * convolutions of generator stage i (SVCMI_CLASS_AMP0 + i; stages on the fused vector-ALU kernels compute in fp32 whatever this says) */
#define SVCMI_AMP_CLASSES 5                         /* amp0 .. amp4; a generator with a sixth stage (SVCMI_MAX_STAGES) runs it in amp4's mode */
enum svcmi_prec_class { SVCMI_CLASS_ENC = 0, SVCMI_CLASS_FLOW = 1, SVCMI_CLASS_UPS = 2, SVCMI_CLASS_AMP0 = 3 /* .. AMP0 + SVCMI_AMP_CLASSES - 1 */,
                        /* the prior encoder's ATTENTION kernel: SVCMI_PREC_BF16 / _F16 = both products on the 16-bit matrix cores
                         * (svcmi_attention16, from a 16-bit copy of the QKV projection's output), anything else = the fp32 kernel */
                        SVCMI_CLASS_ENC_ATTN = 8 };
#define SVCMI_PREC_CLASSES 12
#ifdef __cplusplus
static_assert(SVCMI_CLASS_AMP0 + SVCMI_AMP_CLASSES <= SVCMI_CLASS_ENC_ATTN, "AMP classes must not reach the encoder-attention class");
#endif
typedef struct svcmi_enc_layer {                    /* attentions.Encoder layer i, vits/attentions.py:36-72 */
    svcmi_weight qkv, o, f1, f2;                    /* conv_q|k|v fused, conv_o, FFN conv_1 / conv_2 */
    const float *rel_k, *rel_v;                     /* emb_rel_k / emb_rel_v [2*window+1][H/heads] */
    const float *g1, *b1, *g2, *b2;                 /* norm_layers_1 / _2 */
} svcmi_enc_layer;

typedef struct svcmi_wn_layer { svcmi_weight in, rs; } svcmi_wn_layer;   /* WN in_layers[l], res_skip_layers[l] (modules.py:148-176) */

typedef struct svcmi_flow_layer {                   /* one ResidualCouplingLayer in EXECUTION order of reverse=True, Flip folded in */
    int32_t x0_off, x1_off, n_wn, reserved;
    svcmi_weight pre, post, snac;                   /* pre writes (h | skip) rows of 2H (upper H output channels zero) */
    svcmi_wn_layer wn[SVCMI_MAX_WN_LAYERS];
} svcmi_flow_layer;

typedef struct svcmi_amp_block {                    /* AMPBlock, vits_decoder/bigv.py:22-58 */
    int32_t k, n_dil;
    int32_t dil[SVCMI_MAX_AMP_DILATIONS];
    int32_t reserved;
    svcmi_weight c1[SVCMI_MAX_AMP_DILATIONS], c2[SVCMI_MAX_AMP_DILATIONS];
    const float *a1_alpha[SVCMI_MAX_AMP_DILATIONS], *a1_beta[SVCMI_MAX_AMP_DILATIONS];   /* activations[2q]   (log-scale alpha / beta) */
    const float *a2_alpha[SVCMI_MAX_AMP_DILATIONS], *a2_beta[SVCMI_MAX_AMP_DILATIONS];   /* activations[2q+1] */
} svcmi_amp_block;

typedef struct svcmi_gen_stage {                    /* ups[i] + noise_convs[i] + resblocks[i*nk .. i*nk+nk) (generator.py:183-194) */
    int32_t u, c, cp, up_taps, up_pad, nz_k, nz_stride, nz_pad, n_blocks, reserved;
    svcmi_weight up, nz;                            /* polyphase ConvTranspose1d operand [u*cp][taps*cin_p]; noise conv [cp][>= nz_k] */
    svcmi_amp_block blocks[SVCMI_MAX_AMP_BLOCKS];
} svcmi_gen_stage;

typedef struct svcmi_synth_model {
    int32_t hidden, inter, n_heads, enc_window, enc_ffn_kernel, flow_kernel, n_enc, n_flow, n_stages;
    int32_t ppg_dim, vec_dim, spk_dim, upsample_input, hop;
    int32_t precision;                              /* enum svcmi_precision of prior encoder / flow / generator GEMMs, or SVCMI_PREC_MIXED */
    float lp_min_flops;                             /* 0 = 1.5e9 */
    float sampling_rate, merge_b;
    /* SVCMI_PREC_MIXED: the mode (SVCMI_PREC_F32 / _BF16X3 / _BF16 / _F16) of each layer class -- enum svcmi_prec_class; the w16 images of a
     * class's weights must be packed for its mode.  Ignored in every other `precision`. */
    int32_t class_prec[SVCMI_PREC_CLASSES];
    svcmi_weight pre, hub, proj;                    /* enc_p.pre / hub / proj (vits/models.py:26-37) */
    const float* pit_emb;                           /* enc_p.pit [256][hidden] */
    svcmi_enc_layer enc[SVCMI_MAX_ENC_LAYERS];
    svcmi_flow_layer flow[SVCMI_MAX_FLOWS];
    svcmi_weight adapter, conv_pre, post;           /* SpeakerAdapter W_scale|W_bias fused [2U][spk]; conv_pre; conv_post (1 row, no bias) */
    const float* merge_w;                           /* NSF merge weights [11] (nsf.py:378-381) */
    const float* filt;                              /* the 12 Kaiser-sinc taps */
    const float *post_alpha, *post_beta;            /* activation_post */
    svcmi_gen_stage stages[SVCMI_MAX_STAGES];
} svcmi_synth_model;

enum svcmi_synth_stop { SVCMI_STOP_NONE = 0, SVCMI_STOP_PRIOR = 1, SVCMI_STOP_FLOW = 2, SVCMI_STOP_GEN_PRE = 3, SVCMI_STOP_STAGE0 = 4 /* + i */ };

typedef struct svcmi_synth_io {
    /* inputs, all device pointers */
    const float* ppg;        /* [batch][t >> ppg_row_shift][ppg_dim] (+ ppg_bstride): shift 1 = the 50 fps Whisper output, x2 repeat fused */
    const float* vec;        /* [batch][t][vec_dim] */
    const float* pit;        /* [batch][t] Hz */
    const float* spk;        /* [batch][spk_dim] */
    const int32_t* lengths;  /* [batch] */
    const float* source;     /* [batch][t*hop] harmonic source (svcmi_pitch2source_fwd) */
    const float* noise;      /* [batch][inter][t]: the randn_like(m) of vits/models.py:51 in the reference's layout */
    int64_t ppg_bstride;     /* floats; 0 = dense */
    int32_t ppg_row_shift, batch, t;
    int32_t stream_frames;   /* 0 = the generator sees the whole chunk; N = time tiles of N frames + 32-frame halos (bit-identical for every N: */
                             /* the kernels' per-row arithmetic does not depend on the launch size, tile policies are pinned by stage width) */
    int32_t stop_after;      /* enum svcmi_synth_stop: timing aid (scripts/stage_times.py): the pipeline stops there, `wave` is not written */
    int32_t reserved;
    /* outputs */
    float* wave;             /* [batch][t*hop] */
    float* z_p;              /* optional [batch][t][inter] time-major copies of the prior sample / flow output (NULL = skip) */
    float* z;
} svcmi_synth_io;

int64_t svcmi_synth_workspace_bytes(const svcmi_synth_model* m, int32_t batch, int32_t t, int32_t stream_frames);
/* Generator.pitch2source, vits_decoder/generator.py:160-165: svcmi_pitch_prefix_f64 + svcmi_pitch_source_f32.  workspace >= batch*t*11 doubles. */
int svcmi_pitch2source_fwd(const svcmi_synth_model* m, const float* f0, const float* rand_ini, const float* noise, int32_t batch,
                           int32_t t, float* source, void* workspace, int64_t workspace_bytes, void* stream);
/* TextEncoder.forward (vits/models.py:39-52 + attentions.py:60-72): z_p [batch][t][inter] time-major */
int svcmi_text_encoder_fwd(const svcmi_synth_model* m, const svcmi_synth_io* io, float* z_p, void* workspace, int64_t workspace_bytes, void* stream);
/* ResidualCouplingBlock.forward(reverse=True) (vits/models.py:89-94): x [batch][t][inter] updated in place */
int svcmi_flow_reverse_fwd(const svcmi_synth_model* m, const svcmi_synth_io* io, float* x, void* workspace, int64_t workspace_bytes, void* stream);
/* Generator.inference (vits_decoder/generator.py:175-200) on z [batch][t][inter] time-major -> io->wave */
int svcmi_generator_fwd(const svcmi_synth_model* m, const svcmi_synth_io* io, const float* z, void* workspace, int64_t workspace_bytes, void* stream);
/* SynthesizerInfer.inference (vits/models.py:251-256): the three stages above on one workspace */
int svcmi_synth_infer_fwd(const svcmi_synth_model* m, const svcmi_synth_io* io, void* workspace, int64_t workspace_bytes, void* stream);

/* Key sweep (svc_inference_shift.py: one clip rendered at every transposition of a range).  Across keys only the pitch changes, so the
 * two front convolutions of the prior encoder run once at batch 1 and everything behind the pitch embedding is an equal-length batch
 * over the keys.  Added under ABI 22: new symbols only, no existing struct or entry point changes.
 *   svcmi_sweep_pitch_f32  pit_k[k][t] = (float)((double)pit[t] * factors[k]) -- the reference's `np.array(pit) * 2 ** (shift / 12)` in
 *                          float64, then torch.FloatTensor.  `factors` is HOST memory (n_keys doubles): the values travel in the kernel
 *                          arguments.  The caller computes them (2 ** (shift / 12)); the kernel calls no pow.
 *   svcmi_sweep_embed_f32  x[k][t][:] = (xs[t][:] + emb[f0_to_coarse(pit_k[k][t])][:]) * (t < length[0]) with the arithmetic of
 *                          svcmi_embed_pitch_f32 (same device function, same operation order: the same bits as that kernel on n_keys
 *                          copies of xs).  xs [t][ldxs] is the masked sum of the two front convolutions; x [n_keys][t][ldx] dense over
 *                          keys; emb [256][c]; length: one int32 on the device, NULL = t.
 * SVCMI_EINVAL before anything is launched for a null pointer (length excepted), n_keys / t / c < 1, ldxs or ldx < c; SVCMI_EUNSUPPORTED
 * for n_keys > SVCMI_SWEEP_MAX_KEYS; SVCMI_EALIGN for c / ldxs / ldx % 4, xs / x / emb not 16-byte aligned, another pointer not aligned
 * to its element. */
#define SVCMI_SWEEP_MAX_KEYS 32
int svcmi_sweep_pitch_f32(const float* pit, const double* factors, float* pit_k, int32_t n_keys, int32_t t, void* stream);
int svcmi_sweep_embed_f32(const float* xs, int32_t ldxs, const float* pit_k, const float* emb, const int32_t* length, float* x,
                          int32_t ldx, int32_t n_keys, int32_t t, int32_t c, void* stream);

/* The whole sweep of one chunk as ONE call: the front convolutions at batch 1 (the launches svcmi_synth_infer_fwd makes for one clip),
 * the two kernels above, then attention encoder, projection, prior sample, reverse flow and generator exactly as svcmi_synth_infer_fwd
 * runs them at batch = n_keys (shared host code).  spk and length are replicated into the workspace.  With n_keys = 1 and factor 1.0 the
 * call makes the launches of svcmi_synth_infer_fwd at batch 1 (the embedding through svcmi_sweep_embed_f32) and gives its bits. */
typedef struct svcmi_sweep_io {
    /* inputs at batch 1, device pointers */
    const float* ppg;        /* [t >> ppg_row_shift][ppg_dim] */
    const float* vec;        /* [t][vec_dim] */
    const float* pit;        /* [t] Hz, the untransposed track */
    const float* spk;        /* [spk_dim] */
    const int32_t* length;   /* [1] */
    /* per key, device pointers */
    const float* source;     /* [n_keys][t*hop] harmonic sources of the transposed tracks (svcmi_pitch2source_fwd at batch n_keys on pit_k) */
    const float* noise;      /* [n_keys][inter][t] */
    double factors[SVCMI_SWEEP_MAX_KEYS];      /* 2 ** (shift / 12) per key, plain data */
    int32_t ppg_row_shift, t, n_keys, stream_frames;
    /* outputs */
    float* wave;             /* [n_keys][t*hop] */
    float* pit_k;            /* optional [n_keys][t]: the transposed tracks (NULL = kept in the workspace) */
} svcmi_sweep_io;
int64_t svcmi_sweep_io_bytes(void);      /* sizeof(svcmi_sweep_io), for FFI bindings */
/* negative (SVCMI_EINVAL; SVCMI_EUNSUPPORTED for n_keys > SVCMI_SWEEP_MAX_KEYS) for a geometry the stage would refuse */
int64_t svcmi_synth_sweep_workspace_bytes(const svcmi_synth_model* m, int32_t n_keys, int32_t t, int32_t stream_frames);
int svcmi_synth_sweep_fwd(const svcmi_synth_model* m, const svcmi_sweep_io* io, void* workspace, int64_t workspace_bytes, void* stream);

/* Singer sweep (svcmi.svc_inference_singers: one clip rendered in many timbres).  Across singers nothing up to and including the prior
 * statistics sees the speaker, so the whole prior encoder runs once at batch 1; the speaker enters at the reverse flow and at the
 * generator's SpeakerAdapter, which run as an equal-length batch over the singers.  Added under ABI 22: new symbols only.
 *   svcmi_sweep_sample_prior_f32  z[r][t][:] = (m[t][:] + noise[r][:][t] * exp(logs[t][:])) * (t < length[0]) for n_rows noise draws on ONE
 *                                 set of statistics.  stats [t][lds] holds m | logs at batch 1 (lds >= 2 i); noise_ncl [n_rows][i][t] in
 *                                 the reference's randn_like(m) layout; z [n_rows][t][ldz] time-major; length: one int32 on the
 *                                 device, NULL = t.  Row r holds exactly the bits svcmi_sample_prior_f32 writes on a copy of `stats`
 *                                 with noise[r] (same device functions, csrc/prior_sample.h); exp is taken once per element, not per row.
 * SVCMI_EINVAL before anything is launched for a null pointer (length excepted), n_rows / t / i < 1, lds < 2 i or ldz < i;
 * SVCMI_EUNSUPPORTED for n_rows > SVCMI_SINGERS_MAX; SVCMI_EALIGN for a pointer not aligned to its element. */
#define SVCMI_SINGERS_MAX 32
int svcmi_sweep_sample_prior_f32(const float* stats, int32_t lds, const float* noise_ncl, const int32_t* length,
                                 float* z, int32_t ldz, int32_t n_rows, int32_t t, int32_t i, void* stream);

/* One chunk in n_singers timbres as ONE call: the front convolutions, the pitch embedding, the attention encoder and the projection at
 * batch 1 (the launches svcmi_synth_infer_fwd makes for one clip), the kernel above into z_p [n_singers][t][inter], then reverse flow and
 * generator exactly as svcmi_synth_infer_fwd runs them at batch = n_singers (shared host code) with the caller's spk rows.  The length and
 * the ONE harmonic source are replicated into the workspace.  With n_singers = 1 the call makes the launches of svcmi_synth_infer_fwd at
 * batch 1 (the sample through svcmi_sweep_sample_prior_f32) and gives its bits. */
typedef struct svcmi_singers_io {
    /* inputs at batch 1, device pointers */
    const float* ppg;        /* [t >> ppg_row_shift][ppg_dim] */
    const float* vec;        /* [t][vec_dim] */
    const float* pit;        /* [t] Hz */
    const int32_t* length;   /* [1] */
    const float* source;     /* [t*hop]: ONE harmonic source, shared by all singers */
    /* per singer, device pointers */
    const float* spk;        /* [n_singers][spk_dim] */
    const float* noise;      /* [n_singers][inter][t] */
    int32_t ppg_row_shift, t, n_singers, stream_frames;
    /* outputs */
    float* wave;             /* [n_singers][t*hop] */
    float* z_p;              /* optional [n_singers][t][inter] (NULL = skip) */
} svcmi_singers_io;
int64_t svcmi_singers_io_bytes(void);    /* sizeof(svcmi_singers_io), for FFI bindings */
/* negative (SVCMI_EINVAL; SVCMI_EUNSUPPORTED for n_singers > SVCMI_SINGERS_MAX) for a geometry the stage would refuse */
int64_t svcmi_synth_singers_workspace_bytes(const svcmi_synth_model* m, int32_t n_singers, int32_t t, int32_t stream_frames);
int svcmi_synth_singers_fwd(const svcmi_synth_model* m, const svcmi_singers_io* io, void* workspace, int64_t workspace_bytes, void* stream);

/* y[r][0:cols] = x[r][0:cols] for `rows` rows of leading dimensions ldy / ldx (floats): the strided device copies of the host
 * above (time tiles of the streaming decoder, optional z_p / z outputs) as a kernel, so that they are stream-ordered and graph-capturable. */
int svcmi_copy2d_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int64_t cols, void* stream);

/* Per-launch timing of the stage entry points (bench.py's roofline leg): between svcmi_trace_begin and svcmi_trace_end every
 * kernel launch the host makes on the calling thread is bracketed by HIP events on its stream.  svcmi_trace_end waits for the last one and
 * fills `out` (up to `cap` records, in launch order); returns the number of launches seen.  Not for production use. */
typedef struct svcmi_trace_record { int32_t op; float ms; double flops, bytes; } svcmi_trace_record;
/* (op: bits 0-7 = the entry point, svcmi_trace_op_name(op); bits 8+ = the enum svcmi_precision code a reduced-precision GEMM launch ran
 * with, so a test can tell an _A16 launch from one that rounds in registers) */
int svcmi_trace_begin(int32_t max_records);
int svcmi_trace_end(svcmi_trace_record* out, int32_t cap);
const char* svcmi_trace_op_name(int32_t op);

/* Packed-model files: a whole model for a host without Python.  `python -m svcmi.tools pack --config cfg.yaml --model sovits5.0.pth
 * --out synth.svcmi` (or --whisper large-v2.pt) writes header + relocation table + the model struct with every pointer stored as
 * (byte offset into the arena + 1; 0 = NULL) + the flat fp32 weight arena in the packed layouts.  The host reads / mmaps the file,
 * asks svcmi_packed_model_info where the arena lies (kind: 1 = svcmi_synth_model, 2 = svcmi_whisper_model), uploads those
 * arena_bytes to device memory (256-byte aligned) and calls svcmi_packed_model_bind, which fills `model_out` (model_bytes = sizeof of the
 * struct of that kind) with device pointers.  examples/stage_host.cpp does exactly this and runs svcmi_synth_infer_fwd. */
int svcmi_packed_model_info(const void* file, int64_t file_bytes, int32_t* kind, int64_t* arena_offset, int64_t* arena_bytes);
int svcmi_packed_model_bind(const void* file, int64_t file_bytes, const void* device_arena, void* model_out, int64_t model_bytes);

/* Layout check for FFI bindings: out[i] = sizeof of svcmi_weight, svcmi_whisper_model, svcmi_synth_model, svcmi_synth_io,
 * svcmi_trace_record, svcmi_conv_desc, svcmi_snake_conv_desc (in this order, up to `cap`); returns the count written.  A binding
 * compares them with its own struct sizes before it trusts a filled struct (svcmi/_lib.py does at load). */
int svcmi_struct_sizes(int64_t* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SVCMI_H */
