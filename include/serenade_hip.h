/*
 * serenade_hip.h — C ABI of libserenade_hip.so (MI355X / gfx950 only).
 *
 * The reference (imulki/serenade) is pure Python on PyTorch and has NO FFI or operator
 * registry: its boundary is the Python class API.  This header is
 * therefore the boundary this build defines *behind* that API: one entry point per
 * arithmetic stage of the inference hot path, each citing the reference code it replaces.
 * The Python mirror classes (serenade_amd.models / serenade_amd.vocoder) keep the
 * reference's signatures and state_dict layout and call only these functions.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (fp32 unless noted), borrowed for the call only;
 *   - activations are channels-last: (batch, time, channels), channels contiguous;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, negative on error; srn_last_error() gives the message
 *     (thread-local).  No allocation, no global mutable state, re-entrant.
 */
#ifndef SERENADE_HIP_H
#define SERENADE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRN_ABI_VERSION 4
#define SRN_MAX_TAPS 16

/* prologue activation applied to the gathered input elements */
enum { SRN_ACT_NONE = 0, SRN_ACT_LEAKY = 1, SRN_ACT_SILU = 2, SRN_ACT_MISH = 3 };
/* residual mode */
enum { SRN_RES_NONE = 0, SRN_RES_ADD = 1, SRN_RES_AXPY = 2 };
/* post op */
enum {
  SRN_POST_NONE = 0,
  SRN_POST_DIV = 1, /* v / post_div (HiFi-GAN: cs / num_blocks, hifigan.py:186) */
  SRN_POST_TANH = 2,
  SRN_POST_RELU = 3,
  SRN_POST_LEAKY = 4, /* LeakyReLU with slope post_div */
  SRN_POST_GELU = 5   /* GELU (erf form, nn.GELU()): HuBERT / ContentVec feature convs and feed-forward */
};
/* arithmetic of the contraction */
enum {
  SRN_PREC_FP32 = 0,  /* exact fp32 MFMA */
  SRN_PREC_BF16X3 = 1, /* split-bf16 (hi + lo), 3 MFMA per product, fp32 accumulate: ~2^-17 per product */
  SRN_PREC_BF16X6 = 2  /* fp32-faithful emulation: exact (hi + mid + lo) split, 6 MFMA per product, fp32 accumulate:
                        * <= 2^-26 per product (below fp32's own rounding unit).  Kernels without a bf16x6 variant
                        * (generic conv_gemm, halo / strip, srn_hifigan_resunit) run their exact-fp32 path instead. */
};
/* SrnConvParams.route: which kernels srn_conv_gemm may choose from (testing / A-B timing; 0 in the product) */
enum {
  SRN_ROUTE_AUTO = 0,
  SRN_ROUTE_TILED = 1,     /* tiled kernels only: no halo, no strip */
  SRN_ROUTE_HALO = 2,      /* the halo kernel whenever it is eligible */
  SRN_ROUTE_GENERIC = 3,   /* the generic conv_gemm kernel only */
  SRN_ROUTE_STRIP = 4,     /* the strip kernel whenever it is eligible */
  SRN_ROUTE_FAST_FP32 = 5  /* exact fp32 on conv_fast.hip's loop instead of conv_f32.hip's */
};
/* kernel families behind srn_conv_gemm (srn_conv_gemm_route) */
enum {
  SRN_FAMILY_GENERIC = 0, /* conv_gemm.hip */
  SRN_FAMILY_F32 = 1,     /* conv_f32.hip */
  SRN_FAMILY_FAST = 2,    /* conv_fast.hip */
  SRN_FAMILY_HALO = 3,    /* conv_halo.hip */
  SRN_FAMILY_STRIP = 4    /* conv_strip.hip (tile 0: the kernel follows from C_in and N) */
};

/*
 * Generalised implicit-GEMM "conv1d" on channels-last fp32 tensors.  Arithmetic of the contraction per
 * `precision`: SRN_PREC_FP32 = exact fp32 on v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fma chain, the
 * reference's precision); SRN_PREC_BF16X3 = every fp32 operand split into (hi, lo) bf16, three
 * v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate (~2^-17 relative per product):
 *
 *   out[z, t*out_t_stride + out_t_off, n] = epilogue( alpha * sum_{tap, c} w[n, tap*C_in + c] *
 *                                  act( in[z, t*in_stride + tap_off[tap], c] ) + bias[n] )
 *
 * Covers, with different parameters, every contraction on the hot path:
 *   Conv1d k3/k7/k11 (+dilation, stride 2, zero or reflect padding)   decoder.py:70,107,271,335;
 *                                                                      serenade.py:282-294,366-373;
 *                                                                      hifigan.py:71-77,140-148; residual_block.py:187-226
 *   ConvTranspose1d (one call per output phase)                        decoder.py:191; hifigan.py:96-104
 *   Conv1d k1 / nn.Linear                                              decoder.py:90,341; transformer.py:120-138
 *   QK^T and PV of the self-attention (batched over batch x heads)     transformer.py:292-301 (diffusers Attention)
 * Input rows t >= len_in[zb] are read as zero (the reference's `x * mask`), rows outside
 * [0, T_in) are zero or reflected.  The input may be the channel-concatenation of two tensors
 * (decoder.py:405,449 `pack([x, skip])`) without materialising it.
 */
typedef struct SrnConvParams {
  int32_t n_batch;   /* z range = n_batch * n_head */
  int32_t n_head;    /* >= 1; z -> (zb = z / n_head, zh = z % n_head) */
  int32_t T_in, T_out;
  int32_t C_in;      /* channels per tap seen by the input gather (multiple of 4) */
  int32_t C_in0;     /* channels taken from in0; the remaining C_in - C_in0 come from in1 (multiple of 32 if < C_in) */
  int32_t C_w;       /* valid k per tap on the weight side (<= C_in; = C_in normally) */
  int32_t N;         /* GEMM N (weight rows) */
  int32_t N_out;     /* stored output channels: 0 (the default), N, or N/2 for GEGLU; anything else is refused */
  int32_t n_taps;
  int32_t tap_off[SRN_MAX_TAPS];
  int32_t in_stride;
  int32_t pad_reflect; /* 0: zero padding, 1: reflection at the tensor's ends, 2: reflection at 0 and at the item's own
                        * end len_in[zb] (exact ragged batches: what nn.ReflectionPad1d does to the unpadded item).
                        * One mirror per end: t < 0 -> -t, then t >= end -> 2 (end - 1) - t; a row still outside
                        * [0, len_in) after that reads as zero (tap offsets are only bounded by T_in, so an item
                        * shorter than the table's reach gets zeros there, not a second reflection) */
  int32_t w_nmajor;    /* 0: w is [N][n_taps*C_in] (k contiguous); 1: w is [K][N] (n contiguous), n_taps == 1 */
  int32_t pro_act;
  float pro_slope;
  float alpha;
  float beta;        /* SRN_RES_AXPY: out = res + beta * val */
  int32_t geglu;     /* 1: weight rows interleaved in 32-row (value | gate) groups, out = value * gelu(gate) */
  int32_t res_mode;
  int32_t post;
  float post_div;
  int32_t out_t_stride, out_t_off;
  int32_t tile;      /* 0 = auto, else a tile-config id (see conv_gemm.hip) */
  const float* in0; int64_t in0_bs, in0_hs; int32_t ld_in0;
  const float* in1; int64_t in1_bs; int32_t ld_in1;
  const float* w;   int64_t w_bs, w_hs; int32_t ldw;
  const float* bias;
  const int32_t* len_in;   /* per zb, or NULL */
  const int32_t* len_out;  /* per zb, or NULL: output rows t >= len_out are multiplied by 0 */
  const float* res;  int64_t res_bs, res_hs; int32_t ld_res;
  const float* res2; int64_t res2_bs; int32_t ld_res2;  /* second additive residual (HiFi-GAN stage sum) */
  float* out; int64_t out_bs, out_hs; int32_t ld_out;
  int32_t precision;  /* SRN_PREC_* */
  int32_t route;      /* SRN_ROUTE_*: kernel selection behind this entry point (testing / A-B timing) */
  /* ws / ws_bytes: optional caller-owned workspace (16-byte aligned, at least srn_conv_gemm_workspace_bytes(p)
   * bytes, shared by all calls of one stream).  With it, launches whose tile grid cannot fill the chip are split
   * over K (conv_splitk.hip); without it (NULL) they run unsplit.  Results agree to fp32 summation order.
   * w_lo (SRN_PREC_BF16X6 only): the lo plane of the pre-split weights, bf16 [N][n_taps][roundup(C_in, 32) / 32][32];
   *   w_hi then holds [hi 32 | mid 32].  NULL otherwise.
   * w_hi (SRN_PREC_BF16X3 only): the static weights already split at load time, bf16
   * [N][n_taps][roundup(C_in, 32) / 32][hi 32 | lo 32]; NULL: the kernel splits the fp32 rows of `w` per call. */
  void* ws; int64_t ws_bytes;
  const void* w_hi; const void* w_lo;
  float* gn_partials; /* or NULL: [zb][ceil(T_out/32)][N/32][2] per-32x32-tile (sum, sumsq) of the stored values */
  /* Transposed tail, or out_tr == NULL: GEMM columns c >= out_tr_col0 (a multiple of 32) are written to
   * out_tr[zb][c - out_tr_col0][t] (row stride ld_out_tr, batch stride out_tr_bs) INSTEAD of `out`.  The QKV
   * projection writes V^T with it, so P.V (transformer.py:292-301) contracts k-major rows like every other GEMM and
   * no transpose pass runs.  Plain epilogue only (no GEGLU / residual / post op / row stride / heads). */
  float* out_tr; int64_t out_tr_bs; int32_t ld_out_tr; int32_t out_tr_col0;
} SrnConvParams;

int srn_abi_version(void);
const char* srn_last_error(void);

/* the workhorse above */
int srn_conv_gemm(const SrnConvParams* p, void* stream);
/* bytes of workspace the split-K path would use for this call (0: the call is never split) */
int64_t srn_conv_gemm_workspace_bytes(const SrnConvParams* p);
/* the kernel srn_conv_gemm would launch for *p, without touching a device: out = {SRN_FAMILY_*, tile id, K slices}
 * (K slices > 1: the f32 / fast slice launch followed by the split-K reduce).  Validates *p as srn_conv_gemm does. */
int srn_conv_gemm_route(const SrnConvParams* p, int32_t out[3]);
/* the kernel forms behind srn_conv_gemm, from the lists the launch and the route read, without touching a device.
 * Returns their number and fills the first `capacity` rows of SRN_FORM_FIELDS values each (rows may be NULL):
 * {SRN_FAMILY_*, tile id, SRN_PREC_* of the arithmetic, B is n-major, the family's form for K slices,
 *  tile rows, tile columns, columns of one wave's tile, LDS stages}.  The generic family's fp32 rows run bf16x6 too. */
#define SRN_FORM_FIELDS 9
int srn_conv_gemm_forms(int32_t* rows, int capacity);

/*
 * GroupNorm(8 groups, eps) -> Mish -> (+ time_bias[c]) -> * mask   (Block1D tail + the time-embedding add of
 * ResnetBlock1D; decoder.py:71-77,96-97).  Statistics come from the per-tile partials written by
 * srn_conv_gemm and run over the full padded length T (as the reference's GroupNorm does).
 *   x, y: (B, T, C); gamma, beta: (C); time_bias: (C) at time_bias + b * time_bias_bs, or NULL; lens: (B) or NULL.
 * valid_stats = 1 (exact ragged batches): the statistics run over the item's own lens[b] rows -- the producing conv
 * must have zeroed its padded rows (len_out) so that they add nothing to the partial sums -- which makes every item of a
 * padded batch equal to its B = 1 run; 0 = the reference's batched semantics above.
 */
int srn_gn_mish_apply(const float* x, const float* gn_partials, const float* gamma, const float* beta,
                      const float* time_bias, int64_t time_bias_bs, const int32_t* lens, float* y, int B, int T,
                      int C, int groups, float eps, int valid_stats, void* stream);

/*
 * Tail of ResnetBlock1D (decoder.py:98-101, 34-45):
 *   v = Mish(GroupNorm(c2)) * mask + r ;  y = (v - mean_c) / sqrt(var_c + eps) * scale[b] + shift[b]
 * c2, r, y: (B, T, C); scale, shift: row b at scale + b * ld_ss (C values each).
 */
int srn_resblock_tail(const float* c2, const float* gn_partials, const float* gamma, const float* beta,
                      const int32_t* lens, const float* r, const float* scale, const float* shift, int64_t ld_ss,
                      float* y, int B, int T, int C, int groups, float gn_eps, float ln_eps, int valid_stats,
                      void* stream);

/* The same, and in the same launch the LayerNorm that opens the transformer block behind every ResnetBlock1D
 * (decoder.py:411-421 -> transformer.py:286, norm1):  y2 = LayerNorm(y; ln2_gamma, ln2_beta, ln2_eps), from the row still
 * in registers (one HBM pass and one launch fewer per block; y2 equals srn_layernorm(y) bit for bit). */
int srn_resblock_tail_ln(const float* c2, const float* gn_partials, const float* gamma, const float* beta,
                         const int32_t* lens, const float* r, const float* scale, const float* shift, int64_t ld_ss,
                         float* y, int B, int T, int C, int groups, float gn_eps, float ln_eps, int valid_stats,
                         const float* ln2_gamma, const float* ln2_beta, float* y2, float ln2_eps, void* stream);

/* nn.LayerNorm over the last dim (transformer.py:211,249): x, y (rows, C). */
int srn_layernorm(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int C, float eps,
                  void* stream);

/*
 * Row softmax of attention scores with a key-padding mask (F.scaled_dot_product_attention semantics at
 * transformer.py:292-301): s (Z, L, ld) in place; keys k >= lens[z / n_head] get probability 0;
 * columns [L, ld) are written as 0 whatever they held (the callers never zero the score buffer).  lens[b] >= 1: a row
 * without a valid key has no softmax.  ld <= 9216.
 */
int srn_softmax_rows(float* s, const int32_t* lens, int Z, int n_head, int L, int ld, void* stream);

/* SinusoidalPosEmb (decoder.py:54-63): out row i (stride ld) = [sin(scale*t_i*f_k), cos(scale*t_i*f_k)], t (n) on device. */
int srn_sinusoidal_emb(const float* t, float* out, int n, int dim, int ld, float scale, void* stream);

/* Generic channels-last copy with channel offset/strides: dst[b,t,dc0+c] = src[b,t,sc0+c] * a + bvec?  (pack/concat) */
int srn_copy_channels(const float* src, int64_t src_bs, int ld_src, int sc0, float* dst, int64_t dst_bs, int ld_dst,
                      int dc0, int B, int T, int C, void* stream);

/* Ragged time-concat (serenade.py:202 `cat([ref_mu, src_mu], dim=1)` per item of a batch whose prompts differ in
 * length): rows [0, n_rows[b]) of src item b -> dst rows row_off[b] + r, channels [dc0, dc0 + C).  NULL row_off = 0,
 * NULL n_rows = T. */
int srn_scatter_rows(const float* src, int64_t src_bs, int ld_src, float* dst, int64_t dst_bs, int ld_dst, int dc0,
                     const int32_t* row_off, const int32_t* n_rows, int B, int T, int C, void* stream);

/* (B, C, T) <-> (B, T, C) transposes at the API edge (reference tensors are (B, C, T); decoder.py:405-467). */
int srn_transpose_ct(const float* src, float* dst, int B, int R, int Cc, int64_t src_bs, int ld_src, int64_t dst_bs,
                     int ld_dst, void* stream);
/* Many such transposes in ONE launch (the table travels in the kernel arguments: capturable): entry e does
 * dst_e[b][c][r] = src_e[b][r][c] for b < B, r < R, c < Cc.  The training step re-lays every conv / linear weight
 * once per step (torch (N, C, k) -> the k-major rows srn_conv_gemm reads, and W^T for the input gradient; what autograd
 * does implicitly for decoder.py's Conv1d / Linear under trainers/ssc.py:57-96): ~140 launches of a few microseconds
 * each when issued one by one. */
#define SRN_TR_LIST_MAX 40
typedef struct SrnTransposeList {
  int32_t n;
  int32_t pad_;
  const float* src[SRN_TR_LIST_MAX];
  float* dst[SRN_TR_LIST_MAX];
  int64_t src_bs[SRN_TR_LIST_MAX], dst_bs[SRN_TR_LIST_MAX];
  int32_t B[SRN_TR_LIST_MAX], R[SRN_TR_LIST_MAX], Cc[SRN_TR_LIST_MAX];
  int32_t ld_src[SRN_TR_LIST_MAX], ld_dst[SRN_TR_LIST_MAX];
  int32_t first_block[SRN_TR_LIST_MAX + 1];  /* filled by the library */
} SrnTransposeList;
int srn_transpose_multi(const SrnTransposeList* list, void* stream);

/* y = (x * a[c] + b[c] - c[c]) / d[c] (Vocoder.decode normalisation, vocoder.py:52-56); x, y (rows, C). */
int srn_renorm(const float* x, const float* trg_scale, const float* trg_mean, const float* voc_mean,
               const float* voc_scale, float* y, int64_t rows, int C, void* stream);

/* HiFi-GAN output stage: LeakyReLU(slope) -> Conv1d(C -> 1, k, pad (k-1)/2) -> tanh  (hifigan.py:137-149).
 * x (B, T, C) channels-last, w (k, C), y (B, T). */
int srn_out_conv_tanh(const float* x, const float* w, const float* bias, float* y, int B, int T, int C, int k,
                      float slope, void* stream);
/* The same stage over a ragged batch: item b holds L_b = min(lens[b], T) rows (lens: device, B int32, each >= 1).
 * y[b, t] for t < L_b is bit for bit what srn_out_conv_tanh gives for that item alone (B = 1, T = L_b): rows at or
 * past L_b count as the zero padding of that call and are not read, whatever they hold.  y[b, t] = 0 for
 * L_b <= t < T.  Kernel choice as in the dense call (C = 32, k = 7 specialised; generic otherwise). */
int srn_out_conv_tanh_ragged(const float* x, const float* w, const float* bias, float* y, const int32_t* lens, int B,
                             int T, int C, int k, float slope, void* stream);
/* The output stage of a causal generator: LeakyReLU(slope) -> CausalConv1d(C -> 1, k) -> tanh (hifigan.py:151-162,
 * vocoder/layers/causal_conv.py:11-41).  x (B, (k - 1) + T, C): per item k - 1 history rows, then the T rows of this
 * call; w (k, C); y (B, T):
 *     y[b, t] = tanh(bias + sum_i w[i] . LeakyReLU(x[b, t + i])),  i < k.
 * History rows of zeros are the conv's causal zero padding (LeakyReLU(0) = 0), so the start of an utterance needs no
 * length: the one-shot call passes zeros, a call in mid-stream the last k - 1 rows of the call before.  Kernel choice
 * as in the dense call (C = 32, k = 7 specialised; generic otherwise), argument checks as the dense call. */
int srn_out_conv_tanh_causal(const float* x, const float* w, const float* bias, float* y, int B, int T, int C, int k,
                             float slope, void* stream);

/*
 * One residual unit of HiFiGANResidualBlock with use_additional_convs (residual_block.py:243-258, loop body):
 *     xt = Conv1d_k,dil(LeakyReLU(x));  xt = Conv1d_k,1(LeakyReLU(xt));  y = xt + x
 * fused into ONE launch for thin stages (C = 32 or 64): the receptive-field rows of x are staged once in LDS, the
 * intermediate `xt` never leaves LDS, weights stream through a double-buffered LDS stage -- one HBM read and one
 * write per unit instead of five passes.  Optionally the stage bookkeeping of HiFiGANGenerator.forward
 * (hifigan.py:183-186) rides in the epilogue:  y = (y + res2) / post_div.
 *   x, out, res2: (n_batch, T, C) channels-last fp32, rows contiguous (ld = C), items x_bs / out_bs / res2_bs apart;
 *   out must not alias x (res2 may be out: in-place running sum).  x: 16-byte aligned, x_bs % 4 == 0; out and res2 need
 *   no more than a float's alignment.
 *   w1, w2: packed [C][k * C] fp32 (tap-major, as srn_conv_gemm's k-major weights); b1, b2: (C).
 *   w1_hi, w2_hi: SRN_PREC_BF16X3 only -- the same weights as bf16 planes [C][k][C / 32][hi 32 | lo 32].
 */
typedef struct SrnResUnitParams {
  int32_t n_batch, T, C;
  int32_t k, dilation;      /* conv1: kernel k, dilation `dilation`; conv2: kernel k, dilation 1; both "same" padded
                             * (srn_hifigan_resunit_causal: both left-padded) */
  float slope;              /* LeakyReLU negative slope in front of both convs */
  const float* x; int64_t x_bs;
  const float* w1; const float* b1; const float* w2; const float* b2;
  const void* w1_hi; const void* w2_hi;
  const float* res2; int64_t res2_bs;  /* or NULL */
  float post_div;           /* 0 or 1: none */
  float* out; int64_t out_bs;
  int32_t precision;        /* SRN_PREC_* */
  int32_t route;            /* 0 = automatic; SRN_RESUNIT_ROUTE_SHARED: resunit.hip's exact-fp32 form (testing / A-B timing) */
} SrnResUnitParams;
enum { SRN_RESUNIT_ROUTE_SHARED = 1 };


int srn_hifigan_resunit(const SrnResUnitParams* p, void* stream);
/* The implementation srn_hifigan_resunit runs for these params, from the very code its launch runs (pure host code, no
 * launch): out[0] = form (SRN_RESUNIT_FORM_*), out[1] = output tiles per batch item, out[2] = workgroups launched
 * (each walks the tiles of the whole batch, out[2] apart).  Returns the launch's validation error where the launch would.
 * Exact fp32 (and SRN_PREC_BF16X6, which runs it) takes resunit_f32.hip's form unless the route asks for the shared one,
 * slope lies outside [0, 1] or one item reaches 2^31 bytes. */
enum { SRN_RESUNIT_FORM_F32 = 0, SRN_RESUNIT_FORM_SHARED_F32 = 1, SRN_RESUNIT_FORM_BF16X3 = 2 };
int srn_hifigan_resunit_route(const SrnResUnitParams* p, int32_t out[3]);
/* The residual unit over a ragged batch: lengths are data, not shape.  `lens`: device array of n_batch int32, each
 * >= 1; item b holds L_b = min(lens[b], T) rows and is computed exactly as srn_hifigan_resunit computes a call with
 * n_batch = 1, T = L_b on that item alone -- in every form (resunit_f32.hip, the shared fp32 form, bf16x3) the dense
 * results bit for bit, because the tile grid (sized by T), the MFMA order and the epilogue order are the dense call's:
 *   - rows t >= L_b of x and res2 are never read as data (they may hold anything, NaN included);
 *   - intermediate rows outside [0, L_b) are zero, as conv2's zero padding of the item alone;
 *   - output rows t >= L_b are left untouched.
 * A tile lying wholly past its item's end is computed and stores nothing.  The same params, validation and route as
 * the dense call (p.T sizes the grid); a NULL `lens` is a validation error, nothing is launched.
 * srn_hifigan_resunit_ragged_route reports what srn_hifigan_resunit_route reports for the same params (the lengths
 * are device data and cannot steer the route; the argument may be NULL). */
int srn_hifigan_resunit_ragged(const SrnResUnitParams* p, const int32_t* lens, void* stream);
int srn_hifigan_resunit_ragged_route(const SrnResUnitParams* p, const int32_t* lens_or_null, int32_t out[3]);
/* The residual unit of a causal generator (HiFiGANResidualBlock with use_causal_conv, residual_block.py:195-258 over
 * vocoder/layers/causal_conv.py:11-41): both convs are left-padded with zeros,
 *     xt = CausalConv_k,dil(LeakyReLU(x));  xt = CausalConv_k,1(LeakyReLU(xt));  y = xt + x   [+ res2] [/ post_div].
 * The same params struct, read differently in one place: p->x points at (n_batch, H + T, C) rows per item, with
 * H = (k - 1) (dilation + 1) -- H history rows followed by the T rows of this call -- items x_bs apart.  out and res2
 * are (n_batch, T, C) as in the dense unit; the residual x of output row t is input row H + t; res2, post_div and the
 * out / res2 aliasing rule are the dense unit's.
 * `lead`: device array of n_batch int32; with v_b = clamp(lead[b], 0, H), item b is computed as the unit applied to an
 * utterance that starts v_b rows before this call's first row:
 *   - input rows before H - v_b are never read as data (they may hold anything, NaN included) and count as zeros;
 *   - intermediate rows that lie before that utterance's row 0 are zero -- the second conv's causal padding -- and not
 *     conv1(0) + b1;
 *   - v_b = 0 is the one-shot causal unit on T rows, v_b = H any call in mid-stream: the left edge is data, as the
 *     right edge is in the ragged call, so one prebuilt call (and one captured graph) serves every chunk of a stream.
 * Forms: the two exact-fp32 ones -- resunit_f32.hip's, and the shared one under SRN_RESUNIT_ROUTE_SHARED (or where the
 * fp32 form is not eligible: slope outside [0, 1], an item of 2^31 bytes) -- each the CAUSAL instance of the one kernel
 * text its dense unit runs: the same tile grid, the same number of staged rows (all of them on the left), the same LDS.
 * There is no split-bf16 variant: SRN_PREC_BF16X3 and SRN_PREC_BF16X6 run the exact-fp32 form (w1_hi / w2_hi are not
 * read).  Validation as the dense call (C 32 or 64, k odd, (k - 1) dilation <= 50, alignment of x); a NULL `lead` is a
 * validation error, nothing is launched.  srn_hifigan_resunit_causal_route reports {form, output tiles per item,
 * workgroups} like srn_hifigan_resunit_route (the leads are device data; the argument may be NULL). */
int srn_hifigan_resunit_causal(const SrnResUnitParams* p, const int32_t* lead, void* stream);
int srn_hifigan_resunit_causal_route(const SrnResUnitParams* p, const int32_t* lead_or_null, int32_t out[3]);

/* SiFiGAN pitch-dependent dilated-conv operand gather (row a9; un-vendored `sifigan` package, parity unpinned):
 * out (B, T, 3C) = [lrelu(x[t]) | lrelu(x[t - r]) | lrelu(x[t + r])], r = rint(d[b, t] * dilation), zero outside. */
int srn_pd_gather(const float* x, const float* d, float* out, int B, int T, int C, float dilation, float slope,
                  void* stream);
/* The same gather over a ragged batch: item b holds L_b = min(lens[b], T) rows (lens: device, B int32, each >= 1; x, d
 * and out keep their (B, T, ...) strides).  out[b, t] for t < L_b is bit for bit what srn_pd_gather gives for that item
 * alone (B = 1, T = L_b): r comes from the item's own d[b, t], the neighbours t -+ r are valid inside [0, L_b) only and
 * zero outside.  Rows t >= L_b of x and d are not loaded, whatever they hold (NaN included); rows t >= L_b of out are
 * not written -- the kernel's loop runs over L_b * C / 4, dead rows cost nothing.  Argument checks as the dense call,
 * plus a non-NULL `lens`. */
int srn_pd_gather_ragged(const float* x, const float* d, const int32_t* lens, float* out, int B, int T, int C,
                         float dilation, float slope, void* stream);

/* GST style encoder (serenade/modules/gst/style_encoder.py:142-191,235-252).  Its Conv2d(k3, s2, p1) + BatchNorm2d(eval)
 * + ReLU layers are srn_conv_gemm launches (one stride-2 three-tap contraction along the mel axis per kernel row, BatchNorm
 * folded into the weights); the two entry points below are the tail. */
/* torch.nn.GRU's last hidden state (style_encoder.py:169,188-189; gates r, z, n) with the input projection hoisted out:
 * gi (B, T, 3H) = x W_ih^T + b_ih comes from one srn_conv_gemm over all (b, t) rows; this call runs only the recurrence
 * h -> W_hh h.  w_hh_t (H, 3H) = W_hh transposed. */
int srn_gru_recur_last(const float* gi, const float* w_hh_t, const float* b_hh, float* h, int B, int T, int H,
                       void* stream);
/* The same recurrence over a ragged batch: gi keeps its (B, T_cap, 3H) strides, item b's recurrence ends after
 * min(n_steps[b], T_cap) steps (n_steps: device, B int32, each >= 1).  h[b] is bit for bit what srn_gru_recur_last gives
 * on that item's own (1, n_steps[b], 3H) rows: one kernel, stated once, runs both.  Rows of gi at or past an item's step
 * count are not loaded, whatever they hold (NaN included).  Argument checks as the dense call, plus a non-NULL
 * `n_steps`. */
int srn_gru_recur_last_ragged(const float* gi, const float* w_hh_t, const float* b_hh, float* h, const int32_t* n_steps,
                              int B, int T_cap, int H, void* stream);
/* The mask of the style encoder's ragged batch (time is the head axis of its Conv2d launches, which len_in / len_out
 * do not reach): for item b, rows h in [n_rows[b], rows_cap) of x + b * bs, n_cols contiguous floats each and rows back
 * to back, become +0.0; rows below n_rows[b] are not touched, n_rows[b] >= rows_cap writes nothing (n_rows: device, B
 * int32, each >= 0).  NULL pointers, non-positive sizes and items that overlap (bs < rows_cap * n_cols with B > 1) are
 * refused. */
int srn_zero_rows_ragged(float* x, int64_t bs, int n_cols, const int32_t* n_rows, int B, int rows_cap, void* stream);
/* The ReplicationPad1d((1, 0)) in front of a CausalConvTranspose1d (vocoder/layers/causal_conv.py:44-77), keyed on
 * device data: where lead[b] <= 0 (item b's stream has not begun), row 0 of x + b * bs becomes a copy of its row 1, rows
 * of n_cols contiguous floats back to back; where lead[b] > 0 the item is not touched (row 0 holds the last row of the
 * chunk before).  lead: device, B int32.  NULL pointers, non-positive sizes and overlapping items are refused. */
int srn_replicate_first_row(float* x, int64_t bs, int n_cols, const int32_t* lead, int B, void* stream);
/* The state a chunked causal generator keeps between calls (the few input rows each CausalConv1d reaches back,
 * vocoder/layers/causal_conv.py:11-41, which the reference recomputes from the whole utterance), moved on with the
 * pushed frame counts as device data: ONE launch for every [history | chunk] buffer of a plan and every item.  Entry e
 * describes a buffer inside `arena`: item b at arena + off + b * bs holds H + T rows of C contiguous floats, `scale`
 * rows per input frame.  n: device, B int32.  For item b of entry e, with m = min(n[b], T / scale) * scale:
 *   n[b] < 0   rows [0, H) become +0.0 (a new utterance begins: zero history is the causal padding);
 *   n[b] == 0  nothing is written (the item was idle, its state stays);
 *   n[b] > 0   rows [0, H) take the values rows [m, m + H) held before the launch -- the snapshot (memmove) result where
 *              the two spans overlap (m < H), with no scratch pass: one workgroup owns a (buffer, item) pair and reads
 *              a block into registers before it stores it.
 * Rows at or past H are never written, rows at or past m + H never read.  The table is passed by value in the kernel
 * arguments.  NULL pointers, B outside [1, 65535], n outside [1, SRN_CARRY_MAX], an entry with off < 0, H < 0, T < 0,
 * C < 1 or scale < 1, and items that overlap (bs < (H + T) C with B > 1) are refused before any launch. */
#define SRN_CARRY_MAX 96
typedef struct SrnCarryEntry {
  int64_t off;
  int64_t bs;
  int32_t H, T, C, scale;
} SrnCarryEntry;
typedef struct SrnCarryTable {
  int32_t n;
  int32_t pad_;
  SrnCarryEntry e[SRN_CARRY_MAX];
} SrnCarryTable;
int srn_history_carry_ragged(float* arena, const SrnCarryTable* table, const int32_t* n, int B, void* stream);

/* StyleTokenLayer (style_encoder.py:235-252 + gst/attention.py:110-184,298-300): ref (B, Dq) -> out (B, F), with its
 * input-independent parts formed at weight-packing time: k, v (n_tok, F) = tanh(embs) W_k^T + b_k / W_v^T + b_v;
 * wq_t (Dq, F), wo_t (F, F) = W_q, W_out transposed.  Limits: n_head <= 256, F % n_head == 0 and
 * (2 F + n_head n_tok + Dq) floats of LDS <= 64 KiB; anything past them is refused. */
int srn_style_token_attention_kv(const float* ref, const float* wq_t, const float* bq, const float* k, const float* v,
                                 const float* wo_t, const float* bo, float* out, int B, int Dq, int n_tok, int F,
                                 int n_head, void* stream);

/*
 * Feature front-end in front of the hot path (serenade/bin/preprocess.py:126-203: `loudness_extract`,
 * `logmelfilterbank`; their arithmetic lives in the un-vendored librosa, restated in oracle/features_oracle.py --
 * parity unpinned).  The STFT itself is srn_conv_gemm over the reflect-padded signal viewed as rows of 16 samples with
 * the window x DFT basis as weights; its output rows are [re(0..n_bins-1) | im(0..n_bins-1) | pad] with stride ld.
 */
/* numpy.pad(x, pad, mode) per batch row, zero-filled up to ld: x (B, n) -> out (B, ld).  mode 0 = "reflect" (what
 * logmelfilterbank passes to librosa.stft, preprocess.py:174-181), 1 = "constant" zeros (librosa.stft's default since
 * 0.10, which loudness_extract's call preprocess.py:131 takes).  B <= 65535. */
int srn_pad_signal(const float* x, float* out, int B, int n, int pad, int ld, int mode, void* stream);
/* out (frames, n_mels) = log_b(max(eps, |spec| @ mel^T)); mel_t (n_bins, n_mels) = filterbank transposed;
 * log_mode 10 / 2 / 0 (natural)  (preprocess.py:176-203). */
int srn_logmel(const float* spec, const float* mel_t, float* out, int64_t frames, int n_bins, int ld, int n_mels,
               float eps, int log_mode, void* stream);
/* out (B, frames) = log(mean_f 10^((max(10 log10(max(amin, |spec|^2)), max_db(utterance) - top_db) + a_weight_db[f])
 * / 20) + add_eps)  (preprocess.py:126-137: power_to_db -> perceptual_weighting -> db_to_amplitude -> mean -> log).
 * gmax_ws: B uint32 of scratch.  B <= 65535. */
int srn_loudness(const float* spec, const float* a_weight_db, uint32_t* gmax_ws, float* out, int B, int frames,
                 int n_bins, int ld, float amin, float top_db, float add_eps, void* stream);
/* The same three for a padded batch of unequal utterances, each item treated as its own B = 1 call treats it (the
 * reference runs both functions on one utterance at a time, preprocess.py:435-447,471-472). */
/* numpy.pad(x[b][:L], pad, "constant") with L = min(lens[b], n) (librosa.stft's default pad_mode since 0.10, which
 * loudness_extract's call preprocess.py:131 takes): out (B, ld)[b][pad + j] = x[b][j] for j < L, 0 everywhere else up
 * to ld; x (B, n) at row stride x_bs is not read at j >= L.  lens: B device int32.  The constant-mode twin of
 * srn_pad_ragged. */
int srn_pad_ragged_zero(const float* x, int64_t x_bs, const int32_t* lens, float* out, int B, int n, int pad, int ld,
                        void* stream);
/* srn_logmel on spec (B, T, ld) -> out (B, T, n_mels) with per-item frame counts `frames` (B device int32): rows
 * t < min(frames[b], T) are srn_logmel's (preprocess.py:176-203), rows at or past it are 0 and nothing of spec is read
 * for them. */
int srn_logmel_ragged(const float* spec, const float* mel_t, const int32_t* frames, float* out, int B, int T,
                      int n_bins, int ld, int n_mels, float eps, int log_mode, void* stream);
/* srn_loudness on spec (B, T, ld) -> out (B, T) with per-item frame counts: the top_db floor of item b comes from the
 * maximum power over its own frames t < min(frames[b], T) only (power_to_db of one utterance, preprocess.py:126-137);
 * rows at or past it are 0 and not read.  gmax_ws: B uint32 of scratch. */
int srn_loudness_ragged(const float* spec, const float* a_weight_db, const int32_t* frames, uint32_t* gmax_ws,
                        float* out, int B, int T, int n_bins, int ld, float amin, float top_db, float add_eps,
                        void* stream);

/*
 * Training step of the estimator: the backward of the decoder blocks that CFM.compute_loss
 * differentiates (flow_matching.py:95-133 -> matcha_components/decoder.py:34-45,66-101,384-467, transformer.py:120-146,
 * 286-352) and the optimizer update (bin/ssc_train.py:331-349, trainers/ssc.py:86-96).  GEMM-shaped gradients (dgrad of
 * convs / projections, dP, dQ) are srn_conv_gemm launches with transposed weights; these are the HBM-bound pieces.
 * Column sums come back as per-row-chunk partial sums the host adds (bit-reproducible, no atomics).
 */
/* y[b,t,:] = LayerNorm_C(x[b,t,:]) * m[b] + a[b]  (no affine inside): nn.LayerNorm with m = gamma, a = beta and batch
 * strides 0; SpeakerAdapter (decoder.py:34-45) with m = W_scale spk + b, a = W_bias spk + b and batch strides C. */
int srn_rowln_fwd(const float* x, const float* m, int64_t m_bs, const float* a, int64_t a_bs, float* y, int B, int T,
                  int C, float eps, void* stream);
/* dx of the above; partial (B, srn_rowln_chunks(T), 2, C): [0] = sum_t dy * xhat (-> dm), [1] = sum_t dy (-> da). */
int srn_rowln_bwd(const float* x, const float* dy, const float* m, int64_t m_bs, float* dx, float* partial, int B, int T,
                  int C, float eps, void* stream);
int srn_rowln_chunks(int T);
/* Block1D's GroupNorm -> Mish -> mask (decoder.py:66-77) backward, statistics over the padded length T.
 * mean, rstd (B, groups); step 1: partial (B, srn_gn_chunks(T), 2, C): [0] = sum_t dg, [1] = sum_t dg * xhat with
 * dg = dy * mish'(gamma xhat + beta) on rows < lens[b]; the host forms d beta, d gamma and gsum (B, groups, 2) =
 * per-group sums of (gamma * [0], gamma * [1]); step 2: dh = rstd (dg gamma - gsum0 / n - xhat gsum1 / n). */
int srn_gn_mish_bwd_partial(const float* h, const float* dy, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, const int32_t* lens, float* partial, int B, int T, int C, int groups,
                            void* stream);
int srn_gn_mish_bwd_apply(const float* h, const float* dy, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, const float* gsum, const int32_t* lens, float* dh, int B, int T, int C,
                          int groups, void* stream);
int srn_gn_chunks(int T);
/* (mean, rstd)[b][g] of GroupNorm from the producing conv's 32 x 32 tile sums (SrnConvParams.gn_partials), statistics
 * over the padded length T: what srn_gn_mish_apply uses internally, kept for the backward pass. */
int srn_gn_stats(const float* partials, float* mean, float* rstd, int B, int T, int C, int groups, float eps,
                 void* stream);
/* col (B, 2, C) = sum over chunks of a (B, n_chunk, 2, C) partial-sum buffer of the kernels above; with gsum != NULL
 * also gsum (B, groups, 2) = per-group sums of gamma * col (step between srn_gn_mish_bwd_partial and _apply). */
int srn_chunk_colsum(const float* partial, const float* gamma, float* col, float* gsum, int B, int n_chunk, int C,
                     int groups, void* stream);
/* out (B, N) = column sums of B row-major (R, N) matrices with row stride ld, batch stride R * ld (bias gradients
 * dY^T 1 with B = 1; the gradient of a per-item broadcast add): two launches, partial (B, srn_colsum_chunks(R), N) is
 * scratch.  Fixed summation order. */
int srn_colsum(const float* x, float* partial, float* out, int B, int64_t R, int N, int ld, void* stream);
int srn_colsum_chunks(int64_t R);
/* softmax backward in place on dp: dp <- scale * p o (dp - rowsum(dp o p)); rows of L with stride ld. */
int srn_softmax_bwd(const float* p, float* dp, int64_t rows, int L, int ld, float scale, void* stream);
/* GEGLU (transformer.py:120-146): hg (rows, 2 inner) = [h | g]; a = h * gelu_erf(g); backward dhg from da. */
int srn_geglu_fwd(const float* hg, float* a, int64_t rows, int inner, void* stream);
int srn_geglu_bwd(const float* hg, const float* da, float* dhg, int64_t rows, int inner, void* stream);
/* torch.optim.AdamW step `step` (1-based) over one flat fp32 buffer: g is scaled by grad_scale first (the
 * clip_grad_norm_ coefficient of trainers/ssc.py:90-94), then p *= 1 - lr wd; m, v updated; p -= lr/bc1 m/(sqrt(v/bc2)+eps). */
int srn_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int step, float grad_scale, void* stream);
/* The same update with the step-dependent scalars in device memory, dyn = {lr, 1 - beta1^step, 1 - beta2^step,
 * grad_scale}: an identical launch every step, so a training step captured as a hipGraph can replay it. */
int srn_adamw_dyn(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                  float weight_decay, const float* dyn, void* stream);
/* clip_grad_norm_'s total norm: partial[i], i < srn_sumsq_blocks(n) (<= 1024), = fp64 sums of squares of slices of g;
 * the host adds them and takes the root. */
int srn_sumsq(const float* g, int64_t n, double* partial, void* stream);
/* the same with a second operand: partial sums of a . b (b == NULL: of a) -- the loss sums of the training step (a torch
 * reduction of this size zeroes its semaphores with hipMemsetAsync, which a captured hipGraph replays wrongly). */
int srn_dot(const float* a, const float* b, int64_t n, double* partial, void* stream);
/* Many small device-to-device copies in one launch (gradients of 262 parameter tensors into the flat gradient buffer):
 * entry e copies len[e] floats from src[e] to dst + off[e].  The table is passed by value in the kernel arguments. */
#define SRN_COPY_LIST_MAX 160
typedef struct SrnCopyList {
  int32_t n;
  int32_t pad_;
  const void* src[SRN_COPY_LIST_MAX];
  int64_t off[SRN_COPY_LIST_MAX];
  int64_t len[SRN_COPY_LIST_MAX];
} SrnCopyList;
int srn_multi_copy(const SrnCopyList* list, float* dst, void* stream);
int srn_sumsq_blocks(int64_t n);
/* torch.nn.utils.weight_norm of the content encoder's convs (serenade/models/serenade.py `Conv1dResnet`; w = g v / ||v||
 * per output channel) fused with the re-layout the conv kernels want: forward writes the packed k-major rows
 * w[n][j * C + c] = g[n] v[n][c][j] / ||v[n]||, optionally W^T for the input gradient wd[c][j * N + n], and 1 / ||v[n]||;
 * backward takes the packed dW and returns dv (N, C, k) and dg (N,).  One workgroup per output channel, fixed summation
 * order.  (Eleven convs x ~14 torch launches per step otherwise.) */
int srn_weight_norm_fwd(const float* v, const float* g, float* w_packed, float* wd, float* inv_norm, int N, int C, int k,
                        void* stream);
int srn_weight_norm_bwd(const float* dw_packed, const float* v, const float* g, const float* inv_norm, float* dv,
                        float* dg, int N, int C, int k, void* stream);

/*
 * Analysis front-end between HiFi-GAN and SiFiGAN -- SURVEY 8 row f1, serenade/bin/ssc_postprocessing.py:142-222.
 * The reference calls pyworld (`pw.cheaptrick` :167, `pw.d4c` :168, `pw.code_aperiodicity` :171), pysptk
 * (`pysptk.sp2mc` :169) and sifigan.utils.features (`dilated_factor` :201-210, `SignalGenerator` :105-111,219-222):
 * third-party code absent from the reference tree, restated from the published algorithms in oracle/world_oracle.py
 * (parity unpinned).  `convert_continuos_f0` (:51-72) and the np.interp length match (:159-166) are in-tree and pinned.
 * All analysis arithmetic is float64 (WORLD's precision); one workgroup per 5 ms frame, everything in LDS.
 */
typedef struct SrnWorldParams {
  int32_t n_batch, max_frames;  /* grid = max_frames x n_batch; frames >= n_frames[b] are skipped */
  int32_t fs, fft_size;         /* cheaptrick: 512 / 1024 / 2048 (GetFFTSizeForCheapTrick); d4c: 1024 / 2048 */
  const double* x; int64_t x_bs; const int32_t* x_len; /* (B, x_bs) float64 waveforms and their valid lengths */
  const double* f0; const double* t; int64_t f_bs;     /* (B, f_bs) F0 in Hz and temporal positions in seconds */
  const int32_t* n_frames;      /* (B,) */
  const double* twiddle;        /* fft_size/2 pairs (cos, -sin)(2 pi k / fft_size) */
  double q1, f0_floor;          /* cheaptrick: compensation-lifter q1 (-0.15); F0 <= f0_floor is analysed as 500 Hz */
  double threshold;             /* d4c: Love-Train voicing threshold (0.85) */
  double unvoiced_db;           /* d4c: what unvoiced / rejected frames hold, 20 log10(1 - 1e-12) */
  const double* band_window; int32_t band_window_len; /* d4c: Nuttall window over the group delay of one band */
  int32_t n_bands;              /* d4c: 3 kHz bands below min(15 kHz, fs/2 - 3 kHz): 3 at 24 kHz */
  double* out0; int64_t out0_bs; int32_t ld_out0; /* cheaptrick: spectral envelope (fft_size/2+1 per frame) or NULL;
                                                    * d4c: band aperiodicity in dB (n_bands per frame) */
  double* out1; int64_t out1_bs; int32_t ld_out1; /* cheaptrick: liftered cepstrum X (its c2r is log sp) or NULL */
} SrnWorldParams;
/* pw.cheaptrick: F0-adaptive Hanning window of 3 periods, power spectrum, DC correction, smoothing over 2 F0 / 3,
 * cepstral smoothing + q1 compensation lifter. */
int srn_world_cheaptrick(const SrnWorldParams* p, void* stream);
/* pw.d4c followed by pw.code_aperiodicity: Love-Train voicing check, static group delay, band aperiodicity in dB. */
int srn_world_d4c(const SrnWorldParams* p, void* stream);
/* out (rows, n_out) = g(in (rows, K)) @ mat_t (K, n_out), g = log (take_log) or identity, float64: pysptk.sp2mc as one
 * matrix (log -> irfft -> c0 / 2 -> SPTK freqt is linear in log sp), n_out <= 64. */
int srn_world_project(const double* in, int64_t rows, int K, int ld_in, const double* mat_t, int n_out, int take_log,
                      double* out, int ld_out, void* stream);
/* c (rows, ld_out) float32 = ([a | b] - mean) / scale (StandardScaler.transform :185-199, torch.FloatTensor :213);
 * mean = scale = NULL: plain concatenation. */
int srn_world_pack_features(const double* a, int na, const double* b, int nb, const double* mean, const double* scale,
                            float* out, int64_t rows, int ld_out, void* stream);
/* float32 waveform -> float64 samples; pcm16: through the PCM_16 file hop of the reference (decode writes
 * lrint(x * 32767), ssc_decode.py:449-455; post-processing reads int16 / 32768, ssc_postprocessing.py:143). */
int srn_wave_to_f64(const float* wave, double* out, int64_t n, int pcm16, void* stream);
/* np.maximum(np.interp(np.linspace(0, n_in - 1, n_out), arange(n_in), f0), 0); copy when n_in == n_out (:159-166). */
int srn_f0_match_length(const double* in, int64_t in_bs, const int32_t* n_in, double* out, int64_t out_bs,
                        const int32_t* n_out, int n_batch, int max_out, void* stream);
/* convert_continuos_f0 (:51-72): cf0 float64, uv float32 (both (B, bs)), ok[b] = 0 when an item has no voiced frame. */
int srn_cont_f0(const double* f0, int64_t bs, const int32_t* n_frames, double* cf0, float* uv, int32_t* ok,
                int n_batch, void* stream);
/* SignalGenerator(signal_types=["sine"]) and the dilated-factor tracks np.repeat(dilated_factor(f0, fs, dense), us). */
typedef struct SrnExcitationParams {
  int32_t n_batch, max_frames, fs, hop;
  const double* f0;        /* (B, f_bs) contour driving the sine (cf0 or f0, `sine_f0_type`) */
  const double* df_f0;     /* (B, f_bs) contour driving the dilated factors (`df_f0_type`) */
  int64_t f_bs;
  const int32_t* n_frames;
  double* phase_ws;        /* (B, f_bs) scratch: phase at every frame start */
  const float* noise;      /* (B, max_frames * hop) standard-normal draws standing in for torch.randn, or NULL */
  float* sine;             /* (B, max_frames * hop) */
  float sine_amp, noise_amp;
  int32_t n_df;            /* <= 4 */
  float* dfs[4];           /* track i: (B, max_frames * df_upsample[i]) */
  int32_t df_upsample[4];  /* np.cumprod(upsample_scales) */
  double dense_factors[4];
} SrnExcitationParams;
int srn_sifigan_excitation(const SrnExcitationParams* p, void* stream);

/*
 * Contractions over TIME of the training step (what `loss.backward()` of trainers/ssc.py:57-96 runs for the
 * Conv1d / Linear weights of matcha_components/decoder.py and for diffusers' attention), exact fp32 MFMA:
 *
 *   out[z, m, j * N + n] = alpha * sum_{item, t} a[z, item, t, m] * b[z, item, t * stride + shift[j], n]
 *
 * with rows of b outside [0, T_b) -- or [0, len_b[item]) -- read as zero.  z = zb * n_head + zh walks independent problems.
 *   weight gradient of a conv:  a = dY (B items of T_out rows, M = C_out), b = X (T_in rows, N = C_in), shift = taps
 *                               -> dW in the packed layout (C_out, taps * C_in) srn_conv_gemm reads;
 *   attention:  dV = P^T dO and dK = dS^T Q, one problem per (batch, head), n_items = 1, T_a = T_b = L.
 * Operands are used as they lie in memory (time-major): no transposes, no padded copies.  When the output has too
 * few tiles to fill the chip the time axis is sliced over extra workgroups; the slices go through `ws`
 * (srn_tn_gemm_workspace_bytes) and are added in slice order: results are bit-reproducible.
 */
typedef struct SrnTnGemmParams {
  int32_t n_batch, n_head;   /* problems */
  int32_t n_items, T_a, T_b; /* contraction: items x T_a rows of a, paired with rows of b in [0, T_b) */
  int32_t stride, n_shifts;
  int32_t shift[SRN_MAX_TAPS];
  int32_t M, N;              /* N % 4 == 0; M free with lda >= roundup(M, 4) */
  const float* a; int64_t a_bs, a_hs, a_is; int32_t lda;
  const float* b; int64_t b_bs, b_hs, b_is; int32_t ldb;
  float* out; int64_t out_bs, out_hs; int32_t ldc;  /* ldc >= n_shifts * N */
  float alpha;
  float* ws; int64_t ws_bytes;  /* or NULL: no slicing */
  int32_t n_inner;              /* > 1: item i = (i / n_inner, i % n_inner) with strides (x_is, x_is2) -- conv2d's */
  int64_t a_is2, b_is2;         /* (batch, output row) items; 0 / 1: one level */
  const int32_t* len_b;         /* or NULL; (n_batch, n_items), one-level items only: rows of b at or past len_b[zb, item]
                                 * read as zero -- the `x * mask` in front of the reference's convs (decoder.py:66-101),
                                 * as srn_conv_gemm's len_in does it in the forward */
  float* colsum;                /* or NULL; (M,), one problem, M % 4 == 0: alpha * sum_{item, t} a[item, t, m] -- a
                                 * conv's bias gradient (the column sums of dY), added in the same slice order */
  int32_t route;                /* 0 = automatic; SRN_TN_ROUTE_GENERAL: the general kernel only (testing / A-B timing) */
} SrnTnGemmParams;
enum { SRN_TN_ROUTE_GENERAL = 1 };
int srn_tn_gemm(const SrnTnGemmParams* p, void* stream);
int64_t srn_tn_gemm_workspace_bytes(const SrnTnGemmParams* p);
/* The kernel srn_tn_gemm runs for these params, from the very code its launch runs (pure host code, no launch):
 * out[0] = tile edge (64 or 128), out[1] = K slices (1: stored directly; without a workspace of
 * srn_tn_gemm_workspace_bytes at a 16-byte aligned address the launch falls back to 1), out[2] = 1 for the scalar-walk
 * kernel, 0 for the general one.  Returns the launch's validation error where the launch would. */
int srn_tn_gemm_route(const SrnTnGemmParams* p, int32_t out[3]);

/*
 * Training-mode pieces of the GST style encoder (serenade/modules/gst/style_encoder.py:171-191,235-252 under autograd;
 * SURVEY 8 f4).  Channels-last rows throughout.
 */
/* BatchNorm2d(training) + ReLU over `rows` x C: stats (2, C) = (batch mean, 1 / sqrt(biased var + eps)) kept for the
 * backward; running statistics updated like nn.BatchNorm2d (momentum, unbiased variance) when given.  rows == 1 (which
 * nn.BatchNorm2d refuses in training mode): the variance is 0, and so is the variance the running statistics take in.
 * The variance is formed from fp32 sums of x - x[0] (row 0 of each column as pivot), so a constant column gives exactly
 * 0 and a nearly constant one keeps its digits; it assumes row 0 is an ordinary sample of its column (a conv output):
 * a pivot many standard deviations from the column mean costs digits of mean and variance instead.
 * partial: srn_bn_chunks(rows) * 2 * C floats of scratch.  C % 4 == 0. */
int srn_bn_chunks(int64_t rows);
int srn_bn_relu_fwd(const float* x, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    float* partial, float* stats, float* y, int64_t rows, int C, float eps, float momentum, void* stream);
/* dx, and sums (2, C) = (dbeta, dgamma). */
int srn_bn_relu_bwd(const float* x, const float* y, const float* dy, const float* stats, const float* gamma,
                    float* partial, float* sums, float* dx, int64_t rows, int C, void* stream);
/* Conv2d(k 3, stride 2, pad 1) on channels-last (B, H, W, C) as a plain GEMM: col[(b, ho, wo), (kh, kw, c)] =
 * x[b, 2 ho + kh - 1, 2 wo + kw - 1, c] (zero outside), row stride ld >= 9 C (pad columns are not written).  The
 * per-(b, ho) form of the inference path leaves 64-row tiles mostly empty once Wo <= 20; flattened, every layer is
 * one well-shaped contraction per direction.  srn_col2im_s2 is the transpose of the gather (the dX side). */
int srn_im2col_s2(const float* x, float* col, int B, int H, int W, int C, int ld, void* stream);
int srn_col2im_s2(const float* col, float* dx, int B, int H, int W, int C, int ld, void* stream);
/* nn.GRU recurrence (gate order r, z, n) on gi = x W_ih^T + b_ih (B, T, 3H), zero initial state: hs (B, T+1, H) all
 * hidden states, gates (B, T, 4H) = [r | z | n | W_hn h + b_hn].  w_hh_t = W_hh transposed (H, 3H). */
int srn_gru_train_fwd(const float* gi, const float* w_hh_t, const float* b_hh, float* hs, float* gates, int B, int T,
                      int H, void* stream);
/* BPTT from dh_last (B, H): dgi, dgh (B, T, 3H); dW_hh = dgh^T hs[:, :T], db_hh = sum dgh are srn_tn_gemm / srn_colsum. */
int srn_gru_train_bwd(const float* dh_last, const float* w_hh, const float* hs, const float* gates, float* dgi,
                      float* dgh, int B, int T, int H, void* stream);
/* StyleTokenLayer's attention core: one query row q (B, F) per item over keys / values (n_tok, F), n_head heads:
 * p (B, n_head, n_tok) softmax weights, ctx (B, F). */
int srn_token_attn_fwd(const float* q, const float* k, const float* v, float* p, float* ctx, int B, int n_tok, int F,
                       int n_head, void* stream);
/* dq (B, F); dk_part, dv_part (B, n_tok, F): per-item terms, summed over items by the caller (srn_colsum). */
int srn_token_attn_bwd(const float* dctx, const float* q, const float* k, const float* v, const float* p, float* dq,
                       float* dk_part, float* dv_part, int B, int n_tok, int F, int n_head, void* stream);

/*
 * ContentVec / HuBERT content encoder (serenade_amd/contentvec.py; the `hubert` track of serenade/bin/preprocess.py:
 * 41-50,361-368,495-503, transformers HubertModel with the last feature-conv stride set to 1).  The rest of the encoder
 * is srn_conv_gemm (feature convs 1-6 and the feed-forward with SRN_POST_GELU), srn_layernorm and srn_softmax_rows.
 */
/* rows of the partial-sum chunks srn_cvec_conv0 writes per item for T0 frames */
int srn_frame_stats_chunks(int T);
/* Feature-conv layer 0 (Cin = 1, k <= 16, any stride, no bias): wave (B, n) at row stride wave_bs (samples at or past n
 * read as zero), w (C, k) -> out (B, T0, C) channels-last, out[b][t][c] = sum_j w[c][j] wave[b][t stride + j] for
 * t < lens[b] and 0 beyond.  partials (B, srn_frame_stats_chunks(T0), C, 2) float64: per chunk (sum, sumsq) of the
 * valid frames, for srn_channel_norm_gelu. */
int srn_cvec_conv0(const float* wave, int64_t wave_bs, int n, const int32_t* lens, const float* w, float* out,
                   double* partials, int B, int T0, int C, int k, int stride, void* stream);
/* GroupNorm(num_groups = C) over each item's valid frames t < lens[b] (statistics from srn_cvec_conv0's partials, fp64),
 * affine, GELU:  y = GELU((x - mean) / sqrt(var + eps) * gamma + beta) on valid rows, 0 on padded rows.  x, y (B, T, C)
 * (y may be x); stats (B, C, 2) receives (mean, rstd). */
int srn_channel_norm_gelu(const float* x, const double* partials, int n_chunks, const int32_t* lens,
                          const float* gamma, const float* beta, float* stats, float* y, int B, int T, int C, float eps,
                          void* stream);
/* Positional conv of the encoder (HubertPositionalConvEmbedding + HubertSamePadLayer) with its GELU and residual:
 *   y[b][t][n] = x[b][t][n] + GELU(bias[n] + sum_{j < k, c < Cg} w[g][j][c][n - g Cg] x[b][t + j - pad][g Cg + c])
 * g = n / Cg, Cg = C / groups (a multiple of 4, <= 64), k <= 128; rows outside [0, min(lens[b], T)) read as zero (lens
 * may be NULL).  w is packed [groups][k][Cg][Cg <= 32 ? 32 : 64] (zero columns past Cg).  x, y (B, T, C), y != x.
 * Exact fp32 (v_mfma_f32_32x32x2_f32). */
int srn_posconv_gelu_res(const float* x, const int32_t* lens, const float* w, const float* bias, float* y, int B,
                         int T, int C, int groups, int k, int pad, void* stream);

/*
 * Phoneme-informed MIDI note transcriber (serenade_amd/transcriber.py; the `est_lf0_score` track of
 * serenade/bin/preprocess.py:374-383,506-528, TranscriptionModel of serenade/modules/phoneme_midi/model.py).  Its STFT,
 * conv layers 1-2, flatten + Linear layers and LSTM input projections are srn_conv_gemm.  Every kernel takes per-item
 * lengths: each item of a padded batch gets what its own B = 1 call gets.
 */
/* nnAudio MelSpectrogram(center=True)'s nn.ReflectionPad1d(n_fft / 2) (feature.py:7-16) of each item on its own:
 * out (B, ld)[b][i] = x[b][reflect(i - pad)] mirrored at L = min(lens[b], n) for i < L + 2 pad, 0 beyond; x (B, n) at row
 * stride x_bs.  Needs lens[b] > pad (checked by the caller, as ReflectionPad1d does). */
int srn_pad_ragged(const float* x, int64_t x_bs, const int32_t* lens, float* out, int B, int n, int pad, int ld,
                   void* stream);
/* nnAudio mel power (mel_basis @ |X|^2) + torchaudio AmplitudeToDB("power", top_db) (feature.py:17-25):
 * spec (B, T, ld_spec) = [re | im] of n_bins bins, mel_t (n_bins, n_mels); out (B, T, ld_out) = 10 log10(max(mel, amin))
 * clamped below at (the item's maximum over its valid frames t < lens[b]) - top_db; frames t >= lens[b] are 0.
 * gmax_ws: B unsigned of scratch (zeroed here by a kernel). */
int srn_mel_db(const float* spec, int ld_spec, int n_bins, const float* mel_t, const int32_t* lens, unsigned* gmax_ws,
               float* out, int ld_out, int B, int T, int n_mels, float amin, float top_db, void* stream);
/* Conv-stack layer 0 (subnetworks.py:10-13,52-56): Conv2d(1 -> C, 3x3, padding (dilation, 1), dilation (dilation, 1))
 * with BatchNorm folded into w (C, 3, 3) and bias (C), then ReLU.  x (B, T, ld_x) at item stride x_bs, F valid columns;
 * out (B, T, F + 2, C) channels-last with a zero border column at each end of the frequency axis; frames
 * t >= lens[b] read and write as zero.  dilation 1 or 2. */
int srn_trans_conv0(const float* x, int64_t x_bs, int ld_x, const int32_t* lens, const float* w, const float* bias,
                    float* out, int B, int T, int F, int C, int dilation, void* stream);
/* MaxPool2d((1, 2)) (subnetworks.py:20,27) on in (B, T, F_in + 2, C) bordered.  flatten 0: out (B, T, F_in / 2 + 2, C)
 * with zero border columns; flatten 1: out (B, T, ld_out), column c (F_in / 2) + f for channels c < C_valid (the
 * transpose + flatten of subnetworks.py:36-37), zeros up to ld_out.  Frames t >= lens[b] are 0. */
int srn_trans_pool(const float* in, const int32_t* lens, float* out, int B, int T, int F_in, int C, int C_valid,
                   int flatten, int ld_out, void* stream);
/* K-slices per hidden unit srn_bilstm_recur uses for H (0: H unsupported) */
int srn_bilstm_slices(int H);
/* Bidirectional nn.LSTM recurrence (gate order i, f, g, o; zero initial state) of BiLSTM.forward (subnetworks.py:
 * 96-128: its 512-frame chunks with carried (h, c) equal one unchunked pass).  g (B, T, ld_g) at item stride g_bs is
 * the input projection x W_ih^T + b_ih + b_hh, columns [0, 4H) forward and [4H, 8H) reverse; w_hh_t (2, H, H, 4):
 * w_hh_t[d][k][j][q] = W_hh[d][q H + j][k].  The reverse direction of item b starts at t = min(lens[b], T) - 1.  out
 * (B, T, ld_out) at item stride out_bs: columns [0, H) forward h_t, [H, 2H) reverse; rows t >= lens[b] are 0.
 * 32 <= H <= 512, H % 8 == 0. */
int srn_bilstm_recur(const float* g, int64_t g_bs, int ld_g, const int32_t* lens, const float* w_hh_t, float* out,
                     int64_t out_bs, int ld_out, int B, int T, int H, void* stream);

/*
 * pYIN F0 estimation, librosa 0.10 `librosa.pyin` (serenade_amd/pitch.py): the f0 contour that the transcriber's
 * FramewiseDecoder.decode turns into note pitches (serenade/modules/phoneme_midi/decoding.py:36-45,
 * librosa.pyin(audio, fmin=65, fmax=2093, sr, frame_length=win_length, hop_length, center=True)).  fp64; the step
 * numbers are those of tests/_pyin_ref.py, the restatement both entry points are held to.  Every item of a padded
 * batch gets what its own B = 1 call gets.  Limits: frame_length <= SRN_PYIN_MAX_FRAME, 3 <= max_period - min_period
 * + 1 <= SRN_PYIN_MAX_PERIODS, 2 n_bins <= SRN_PYIN_MAX_STATES, n_thresholds <= SRN_PYIN_MAX_THRESHOLDS.
 */
#define SRN_PYIN_MAX_FRAME 4096
#define SRN_PYIN_MAX_PERIODS 1024
#define SRN_PYIN_MAX_STATES 4096
#define SRN_PYIN_MAX_THRESHOLDS 1024
/* Steps 1-5 (decoding.py:36-45 -> librosa.pyin up to the observation matrix), one workgroup per (item, frame).
 * x (B, N) float32 at row stride x_bs, lens[b] <= N valid samples, frames[b] <= T frames of item b (frame t starts at
 * sample t hop_length - pad; samples outside [0, lens[b]) read as zero).  Per frame: the cumulative mean normalised
 * difference over periods [min_period, max_period] (window win_length), parabolic shifts, troughs, their probabilities
 * (thresholds, beta_probs: n_thresholds; boltz_fact[c] = (1 - e^-l) / (1 - e^-l c) for c <= nf, boltz_exp[p] = e^-l p
 * for p < nf, no_trough[m] = no_trough_prob * sum(beta_probs[:m]) for m <= n_thresholds; nf = max_period - min_period
 * + 1), and the pitch bins round(bins_per_octave log2(sr / period / fmin)) clipped to [0, n_bins].  Writes obs
 * (B, T, n_bins): the voiced observation row (the larger period wins a shared bin) and voiced_prob (B, T), clipped to
 * [0, 1]; frames t >= frames[b] get voiced_prob 0 and leave obs untouched. */
int srn_pyin_observe(const float* x, int64_t x_bs, const int32_t* lens, const int32_t* frames, const double* thresholds,
                     const double* beta_probs, const double* boltz_fact, const double* boltz_exp,
                     const double* no_trough, double* obs, double* voiced_prob, int B, int N, int T, int frame_length,
                     int win_length, int hop_length, int pad, int min_period, int max_period, int n_thresholds,
                     double sr, double fmin, double bins_per_octave, int n_bins, void* stream);
/* Steps 6-8 (decoding.py:36-45 -> librosa.sequence.viterbi and pyin's state -> f0 map), one workgroup per item over
 * its own frames[b] frames.  States 0 .. n_bins - 1 voiced, n_bins .. 2 n_bins - 1 unvoiced; observations: obs (the
 * voiced row) and (1 - voiced_prob) / n_bins on every unvoiced state, log(p + tiny), log_tiny where p = 0.  log_band
 * (2, width, n_bins): [0][d + width / 2][q] = log((1 - switch) T[q + d][q] + tiny), [1] the same with the switch
 * probability (T = transition_local(n_bins, width, "triangle")); log(tiny) = log_tiny everywhere else, as the dense
 * matrix has it.  log_p_init (2 n_bins).  The argmax is the first maximal predecessor, as librosa's.  ptr_ws: B T 2 n_bins
 * uint16 of scratch.  Writes states (B, T) int32 (-1 past frames[b]), f0 (B, T): freqs[state] (freqs has 2 n_bins
 * entries, the unvoiced half repeating the voiced one), fill_na on unvoiced states when fill_unvoiced and on frames past
 * frames[b]; voiced_flag (B, T) 0/1. */
int srn_pyin_viterbi(const double* obs, const double* voiced_prob, const int32_t* frames, const double* log_band,
                     const double* log_p_init, const double* freqs, double log_tiny, double fill_na, int fill_unvoiced,
                     uint16_t* ptr_ws, int32_t* states, double* f0, uint8_t* voiced_flag, int B, int T, int n_bins,
                     int width, void* stream);

/*
 * WORLD Harvest F0 estimation (Morise 2017, harvest.cpp) as pyworld.harvest runs it on every utterance of
 * preprocessing (serenade/bin/preprocess.py:485-493: pyworld.harvest(audio, fs, f0_floor, f0_ceil, frame_period));
 * serenade_amd/harvest.py drives the five entry points in this order.  fp64; tests/_harvest_ref.py is the
 * restatement every one of them is held to.  Everything takes per-item lengths and frame counts: every item of a
 * padded batch gets what its own B = 1 call gets and samples past an item's length are never read.  The body always
 * works on 1 ms frames (frames[b] = int(1000 n / fs) + 1 of them, at most F1).  Limits: a channel's band-pass has
 * at most SRN_HARVEST_MAX_TAPS taps (2 matlab_round(2 actual_fs / (0.9 f0_floor 2^(1/40))) + 1), the refinement's
 * window 2 int(1.5 actual_fs / f0_floor + 1) + 1 at most SRN_HARVEST_MAX_WINDOW samples, at most
 * SRN_HARVEST_MAX_CAND candidates per frame (7 matlab_round(n_ch / 10)), decimation ratio <= SRN_HARVEST_MAX_RATIO.
 */
#define SRN_HARVEST_MAX_TAPS 1024
#define SRN_HARVEST_MAX_WINDOW 1536
#define SRN_HARVEST_MAX_CAND 256
#define SRN_HARVEST_MAX_RATIO 12
#define SRN_HARVEST_SMOOTH_PAD 300
/* preprocess.py:485-493 -> Harvest's GetWaveformAndSpectrum + decimate, one wave per item.  x (B, N) float32
 * (x_is_f64 0) or float64 (1) at row stride x_bs, lens[b] <= N samples.  ratio > 1: the item extended by lag
 * (a multiple of ratio, >= 10) copies of each edge sample, MATLAB-style zero-phase decimate (9 reflected samples, the
 * order-3 filter coef = b[0..3], a[0..3] in direct form II from zero state, forwards then backwards), every ratio-th
 * sample, the first lag / ratio dropped; ratio 1: a copy.  Then the mean over the item's ceil(lens[b] / ratio)
 * samples is removed.  ws: B x ws_stride doubles of scratch, ws_stride >= N + 2 lag + 18 (unused for ratio 1).
 * y (B, y_bs), y_bs >= ceil(N / ratio). */
int srn_harvest_decimate(const void* x, int x_is_f64, int64_t x_bs, const int32_t* lens, const double* coef, double* ws,
                         int64_t ws_stride, double* y, int64_t y_bs, int B, int N, int ratio, int lag, void* stream);
/* preprocess.py:485-493 -> Harvest's GetRawF0Candidates (GetFilteredSignal, ZeroCrossingEngine x 4,
 * GetF0CandidateContour), one workgroup per (channel, item) for the channels ch0 .. ch0 + n_launch - 1 of n_ch.
 * y (B, y_bs): item b has ylens[b] <= max_ylen samples at fs (the decimated rate) and frames[b] 1 ms frames.  Channel
 * c: taps[tap_off[c] .. + 2 half_len[c]] (Nuttall window x cosine at boundary[c], built on the host), max_half_len
 * the largest half length.  The band-pass is the linear convolution taken at index bias half_len + 1, zeros outside
 * the item.  events: B x n_launch x 4 x ev_cap doubles of scratch, ev_cap >= max_ylen / 2 (an edge needs two
 * samples, so no kind of event can have more).  raw (B, n_ch, F1): the channel's candidate at every frame, 0 where
 * any kind of event has fewer than 3 intervals, where the average of the four interpolated contours is outside
 * [0.9, 1.1] boundary[c] or [f0_floor, f0_ceil], and on frames past frames[b]. */
int srn_harvest_channels(const double* y, int64_t y_bs, const int32_t* ylens, const int32_t* frames, const double* taps,
                         const int32_t* tap_off, const int32_t* half_len, const double* boundary, int max_half_len,
                         double* events, int64_t ev_cap, double* raw, int B, int ch0, int n_launch, int n_ch, int F1,
                         int max_ylen, double fs, double f0_floor, double f0_ceil, void* stream);
/* preprocess.py:485-493 -> Harvest's DetectOfficialF0Candidates + OverlapF0Candidates, one thread per (item, frame).
 * official (B, F1, n_base): the means of raw over every run of >= 10 channels with a candidate (first and last channel
 * ignored), in channel order, zero-filled.  cand (B, F1, 7 n_base): block 0 the frame's own, blocks 1-3 those of the
 * frames 1-3 before, blocks 4-6 those of the frames 1-3 after; a missing neighbour gives 0. */
int srn_harvest_candidates(const double* raw, const int32_t* frames, double* official, double* cand, int B, int n_ch,
                           int F1, int n_base, void* stream);
/* preprocess.py:485-493 -> Harvest's RefineF0Candidates (GetRefinedF0), one wave per (item, frame) over the frame's
 * non-zero candidates: Blackman-type window of 2 int(1.5 fs / f0 + 1) + 1 samples centred on the frame's time and its
 * central-difference derivative, sample indices clamped into the item, a direct DFT at the bins of the first
 * min(int(fs / 2 / f0), 6) harmonics, the instantaneous frequency of each, refined (B, F1, n_cand) = their
 * amplitude-weighted F0 and score = 1 / (1e-12 + mean relative deviation); both 0 where refined is outside
 * [f0_floor, f0_ceil] or score < 2.5. */
int srn_harvest_refine(const double* y, int64_t y_bs, const int32_t* ylens, const int32_t* frames, const double* cand,
                       double* refined, double* score, int B, int F1, int n_cand, double fs, double f0_floor,
                       double f0_ceil, void* stream);
/* preprocess.py:485-493 -> Harvest's RemoveUnreliableCandidates (one thread per candidate, into cand2 / score2
 * (B, F1, n_cand)), then one workgroup per item: SearchF0Base, FixStep1-4 (Extend runs one wave per voiced section),
 * SmoothF0Contour (one lane per section, smooth_coef = b[0..2], a[0..2], SRN_HARVEST_SMOOTH_PAD frames of padding) and
 * the pick f0_out[b][i] = smoothed[min(frames[b] - 1, matlab_round(i frame_period))] for i < out_frames[b], 0 up to
 * F_out.  fbuf (B, 6, F1): [0] the best candidates, [3] the contour before smoothing, [4] the smoothed 1 ms contour.
 * pool: B x pool_stride doubles, sections: B x 7 x sec_cap int32 of scratch; status[b] != 0 reports that item b had
 * more voiced sections than sec_cap or pool_stride hold (sec_cap >= F1 / min(voice_range_minimum + 2, 10) + 4 and
 * pool_stride >= F1 + 600 sec_cap always suffice). */
int srn_harvest_contour(const double* refined, const double* score, const int32_t* frames, const int32_t* out_frames,
                        const double* smooth_coef, double* cand2, double* score2, double* fbuf, double* pool,
                        int64_t pool_stride, int32_t* sections, int sec_cap, int32_t* status, double* f0_out,
                        int64_t out_stride, int B, int F1, int n_cand, int F_out, int voice_range_minimum,
                        double frame_period, void* stream);

/*
 * The waveform arithmetic between the file on disk and the feature front-ends (serenade_amd/audio.py drives it,
 * tests/_audio_ref.py is the restatement): resampling, silence trimming and the reflect tail pad of
 * serenade/bin/preprocess.py:405-432 and the resampling of ssc_postprocessing.py:146.  All three are ragged: x (B, N)
 * float32 (x_is_f64 0) or float64 (1) at row stride x_bs, item b has its own sample count and nothing past it is read;
 * every sum is fp64 in an order that depends on the item alone, so each item gets bit for bit what its B = 1 call
 * gets; y has x's dtype (the fp64 result rounded once for float32).
 */
#define SRN_RESAMPLE_TILE 256      /* outputs per workgroup */
#define SRN_RESAMPLE_MAX_SPAN 8192 /* inputs one tile may touch (64 KiB of LDS): ceil(255 M / L) + K */
/* preprocess.py:405-412, :428-432 and ssc_postprocessing.py:146 -> librosa.resample as a polyphase Kaiser-windowed
 * sinc (the filter is specified in audio.py / DESIGN.md 7e; soxr itself is not restated).  L = target / g,
 * M = orig / g: y[b][m] = sum_j x[b][j] h[m M - j L] over 0 <= j < lens[b], j ascending, for m < out_lens[b]
 * (<= n_out_max), zeros up to n_out_max.  table (K, L) float64, tap-major: table[k][p] = h[p - (k - q_lo) L], 0 where
 * the argument lies beyond the filter's half length; output m uses phase p = m M mod L on the inputs
 * floor(m M / L) - q_lo + k, k = 0 .. K - 1. */
int srn_resample(const void* x, int x_is_f64, int64_t x_bs, const int32_t* lens, const int32_t* out_lens,
                 const double* table, void* y, int64_t y_bs, int B, int N, int n_out_max, int L, int M, int K,
                 int q_lo, void* stream);
/* preprocess.py:416-422 -> the frame decisions of librosa.effects.trim.  Item b has 1 + lens[b] / hop frames (at most
 * T_max), frame t the samples [t hop - frame_length / 2, + frame_length) with zeros outside the item; ms (B, T_max)
 * float64 scratch receives the mean of squares of each.  Frame t is non-silent iff
 * max(1e-10, ms_t) > factor max(1e-10, max_t ms_t), factor = 10^(-top_db / 10).  bounds (B, 2) int32:
 * (first hop, min(lens[b], (last + 1) hop)) over the non-silent frames, (0, 0) when there is none. */
int srn_trim_bounds(const void* x, int x_is_f64, int64_t x_bs, const int32_t* lens, double* ms, int32_t* bounds, int B,
                    int N, int T_max, int frame_length, int hop, double factor, void* stream);
/* preprocess.py:416-426 -> the trimmed slice and np.pad(audio, (0, pad), mode="reflect") in one pass:
 * y[b][i] = x[b][starts[b] + i] for i < counts[b], x[b][starts[b] + counts[b] - 2 - (i - counts[b])] for the next pad
 * samples (pad < counts[b]: one reflection), zeros up to width.  starts[b] + counts[b] must lie within the item. */
int srn_wave_window(const void* x, int x_is_f64, int64_t x_bs, const int32_t* starts, const int32_t* counts, int pad,
                    void* y, int64_t y_bs, int B, int width, void* stream);

/*
 * Stage 2 of the recipe and the batch the training step eats (serenade_amd/stats.py drives both, tests/_stats_ref.py is
 * the restatement): the per-utterance sums behind sklearn's StandardScaler / MinMaxScaler.partial_fit of
 * serenade/bin/compute_statistics.py:121-144, and FeatsDataset's normalisation (serenade/datasets/
 * audio_mel_dataset.py:96-110) followed by SSCCollater's sort, drop and zero padding (serenade/collaters/ssc.py:50-77).
 * Input is PACKED: x (R, C) float32 row-major, the rows of all B items one after another; row_off [B + 1] int64 on the
 * device, item b the rows [row_off[b], row_off[b + 1]).  Nothing outside an item is read (offsets are clamped to
 * [0, R]).  Every sum is fp64, contraction off, in an order that depends on the item's row count alone, so a batched
 * call is bit for bit its B = 1 calls.
 */
#define SRN_STATS_COL_TILE 64 /* columns per workgroup of srn_col_moments */
/* compute_statistics.py:138-141 -> what one partial_fit needs of one utterance.  Per item b and column c, with
 * n = the item's rows: sum (B, C) float64 = sum_r x; m2 (B, C) float64 = sum_r d^2 - (sum_r d)^2 / n with
 * d = (double)x - sum / n (sklearn.utils.extmath._incremental_mean_and_var's new_unnormalized_variance); mn / mx (B, C)
 * float32, the input's own values; nonfinite (B) int32, the item's count of NaN / +-inf (zeroed here by a kernel).
 * Order of every sum: wave w = 0 .. 3 adds the rows w, w + 4, ... in turn, then (s0 + s1) + s2 + s3. */
int srn_col_moments(const float* x, const int64_t* row_off, int64_t R, double* sum, double* m2, float* mn, float* mx,
                    int32_t* nonfinite, int B, int C, void* stream);
/* audio_mel_dataset.py:96-110 + collaters/ssc.py:50-77 for one track: out (Bout, Tmax, C) float32,
 * out[b][t][c] = (x[row_off[order[b]] + t][c] - sub[c]) / div[c] for t < the item's rows, exact +0.0 for the rest up
 * to Tmax; every element of out is written.  order (Bout) int32 on the device picks and sorts the items (an index
 * outside [0, B) reads as an empty item).  wide 1: sub / div (C) float64, both operations fp64, one rounding to
 * float32 (numpy's float32 - float64, / float64, then .float()); wide 0: sub / div (C) float32, both operations
 * float32 (numpy's float32 track against MinMaxScaler's float32 data_min_ / span).  Tmax C < 2^31. */
int srn_scale_collate(const float* x, const int64_t* row_off, int64_t R, const int32_t* order, const void* sub,
                      const void* div, int wide, float* out, int Tmax, int B, int Bout, int C, void* stream);

/*
 * The host loop behind the note transcriber (serenade_amd/transcriber.py drives both, tests/_notes_ref.py is the
 * restatement; notes.hip states the semantics once).  Ragged batches: padded arrays plus per-item counts, clamped
 * against the padded extents passed alongside; one workgroup per item, so an item inside a batch gets the bits of its
 * own B = 1 call.
 */
#define SRN_NOTE_MAX_FRAMES 8192 /* frames per item (Tmax) of srn_note_decode; the host raises beyond it */
/* serenade/modules/phoneme_midi/decoding.py:22-159 (FramewiseDecoder.decode with f0 given, _peak_selector,
 * _decode_notes): logits (B, Tmax, 3) float32 contiguous (onset, offset, frame), frames (B) valid frames per item;
 * f0 (B, Fmax) float64 pYIN contour in Hz (NaN = unvoiced), f0_frames (B) its frames per item; pitch_sum 0 median,
 * 1 weighted_mean, 2 weighted_median; log2_a4 = log2(440) as the host computes it.  Out: counts (B) notes per item,
 * intervals (B, Tmax, 2) int32 (onset, offset + 1), pitches (B, Tmax) float64 MIDI pitch per note; entries past an
 * item's count are 0.  Scratch: ws_f (B, 5, Tmax) float32, ws_d (B, 4, Tmax) float64, ws_i (B, 2, Tmax) int32. */
int srn_note_decode(const float* logits, const int32_t* frames, const double* f0, const int32_t* f0_frames, int B,
                    int Tmax, int Fmax, float onset_threshold, float offset_threshold, int pitch_sum, double log2_a4,
                    float* ws_f, double* ws_d, int32_t* ws_i, int32_t* counts, int32_t* intervals, double* pitches,
                    void* stream);
/* serenade/bin/preprocess.py:237-259 (midi_to_frames), :117-123 (_midi_to_hz(log_f0=True)) and the arithmetic of
 * :510-528: counts (B), intervals (B, cap, 2) int32 >= 0 and pitches (B, cap) float64 as srn_note_decode leaves them;
 * n_samples (B) samples per item at the acoustic rate; scale = hop_length / sample_rate of the transcriber,
 * shift = shiftms / 1000, sampling_rate the acoustic rate, all float64 from the host; table (128) int32 the log-Hz
 * value per MIDI number.  Per item n = ceil((n_samples / sampling_rate) / shift) frames (clamped to Nmax, written to
 * n_frames (B)); note k covers the frames floor((onset scale) / shift) .. min(ceil((end scale) / shift), n) with its
 * pitch rounded half to even, the last note covering a frame wins, frames of no note are 0: midi (B, Nmax) int32 and
 * lf0 (B, Nmax) int32 = table[midi]; every element is written.  bad (1) int32 is set when a rounded pitch lies
 * outside 0 .. 127 or an interval is negative (such a note is left out).  Scratch: ws (B, cap, 3) int32. */
int srn_note_frames(const int32_t* counts, const int32_t* intervals, const double* pitches, int B, int cap,
                    const int32_t* n_samples, double scale, double shift, double sampling_rate, const int32_t* table,
                    int32_t* ws, int32_t* midi, int32_t* lf0, int Nmax, int32_t* n_frames, int32_t* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
