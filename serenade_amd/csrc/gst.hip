// gst.hip — the tail of the GST style encoder (run once per utterance): the GRU recurrence on a precomputed input
// projection and the style-token multi-head attention on precomputed keys / values.  (The Conv2d + BatchNorm + ReLU
// layers are srn_conv_gemm launches, one per kernel row: models.StyleEncoder.build_ops.)  Reference: serenade/modules/gst/style_encoder.py:142-191,235-252 and
// serenade/modules/gst/attention.py:110-184,298-300.
#include "common.h"
#include "conv_common.h"  // SrnLens, srn_first
#include "row_common.h"

namespace {

// GRU recurrence on a PRECOMPUTED input projection gi = x W_ih^T + b_ih (one srn_conv_gemm over all (b, t) rows,
// spread over the chip) -- the part that is inherently sequential is only h -> W_hh h, done by one workgroup per
// batch item: row_common.h's gru_forward, which gst_train.hip's forward runs too (keeping every step).
// Lens: empty in the dense instance, whose arguments and code are what they were before the pack existed; one SrnLens
// in the ragged one (conv_common.h), where item b's recurrence ends after n_b = min(lens[b], T) steps of its T rows.
template <class... Lens>
__global__ void gru_recur_last_kernel(const float* __restrict__ gi_all, const float* __restrict__ w_hh_t,
                                      const float* __restrict__ b_hh, float* __restrict__ hout, int T, int H,
                                      const Lens... lens) {
  static_assert(sizeof...(Lens) <= 1, "the ragged instance takes the step counts, the dense one nothing");
  extern __shared__ float sm[];  // h[H] | gh[3H]
  if constexpr (sizeof...(Lens) == 0) {
    gru_forward<false>(sm, gi_all, w_hh_t, b_hh, hout, nullptr, nullptr, T, H);
  } else {
    const int n = max(min(srn_first(lens...)[blockIdx.x], T), 1);  // one scalar load, uniform over the workgroup
    // gru_forward finds step t of item b at row b * n + t of the pointer it is given.  Item b's rows start at row
    // b * T of gi_all, so the pointer is moved on by b * (T - n) rows: row b * n + t of it is row b * T + t of gi_all,
    // and the rows read are the item's first n.  The arithmetic is gru_forward's own, the dense kernel's at T = n.
    gru_forward<false>(sm, gi_all + (int64_t)blockIdx.x * (T - n) * 3 * H, w_hh_t, b_hh, hout, nullptr, nullptr, n, H);
  }
}

// +0.0 into rows [n_rows[b], rows_cap) of item b (rows of n_cols contiguous floats, rows back to back): the span is
// ONE contiguous run of floats, [n_rows[b] * n_cols, rows_cap * n_cols) behind x + b * bs.  Grid (chunks, B), a
// workgroup owns ZR_CHUNK floats of the item, a thread four consecutive ones: a 16-byte store where all four are past
// the item's end and the address is aligned (n_cols % 4 == 0 and an aligned base make every quad so), single stores
// for the quad that holds the edge, for the tail, and for every quad of a misaligned base.
constexpr int ZR_THREADS = 256;
constexpr int ZR_CHUNK = 4 * ZR_THREADS;

__global__ __launch_bounds__(ZR_THREADS) void zero_rows_ragged_kernel(float* __restrict__ x, int64_t bs, int n_cols,
                                                                      SrnLens n_rows, int rows_cap) {
  const int b = blockIdx.y;
  const int64_t total = (int64_t)rows_cap * n_cols;
  const int64_t start = (int64_t)max(n_rows[b], 0) * n_cols;  // one scalar load, uniform over the workgroup
  const int64_t e0 = (int64_t)blockIdx.x * ZR_CHUNK;
  if (e0 + ZR_CHUNK <= start) return;  // uniform: the whole chunk lies before the item's end (or the item is full)
  float* xb = x + (int64_t)b * bs;
  const int64_t q = e0 + 4 * (int64_t)threadIdx.x;
  if (q >= start && q + 4 <= total && (reinterpret_cast<uintptr_t>(xb + q) & 15) == 0) {
    *reinterpret_cast<float4*>(xb + q) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q + j >= start && q + j < total) xb[q + j] = 0.f;
  }
}

// ReplicationPad1d((1, 0)) of a stream's first chunk, keyed on device data: where lead[b] <= 0, row 0 of item b becomes a
// copy of its row 1 (rows of n_cols contiguous floats, back to back).  Grid (chunks of 256 floats, B); lead[b] is one
// scalar load, uniform over the workgroup, and an item in mid-stream costs that load only.
__global__ __launch_bounds__(256) void replicate_first_row_kernel(float* __restrict__ x, int64_t bs, int n_cols,
                                                                  SrnLens lead) {
  const int b = blockIdx.y;
  if (lead[b] > 0) return;  // uniform: row 0 holds the previous chunk's last row
  const int c = blockIdx.x * 256 + threadIdx.x;
  float* xb = x + (int64_t)b * bs;
  if (c < n_cols) xb[c] = xb[n_cols + c];
}

// Style-token attention on PRECOMPUTED keys / values: K = tanh(embs) W_k^T + b_k and V likewise do not depend on the
// input, so they are formed once at weight-packing time ((n_tok, F) each); the query / output projections read
// TRANSPOSED weights (wq_t [Dq][F], wo_t [F][F]) so lanes read consecutive addresses.  One workgroup per batch item.
__global__ __launch_bounds__(256) void style_token_attention_kv_kernel(
    const float* __restrict__ ref, const float* __restrict__ wq_t, const float* __restrict__ bq,
    const float* __restrict__ kk, const float* __restrict__ vv, const float* __restrict__ wo_t,
    const float* __restrict__ bo, float* __restrict__ out, int Dq, int n_tok, int F, int n_head) {
  extern __shared__ float sm[];
  float* q = sm;                       // [F]
  float* sc = q + F;                   // [n_head][n_tok]
  float* ctx = sc + n_head * n_tok;    // [F]
  float* sref = ctx + F;               // [Dq]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int dk = F / n_head;
  for (int i = tid; i < Dq; i += 256) sref[i] = ref[(int64_t)b * Dq + i];
  __syncthreads();
  for (int f = tid; f < F; f += 256) {
    float a = 0.f;
    for (int i = 0; i < Dq; ++i) a = fmaf(sref[i], wq_t[(int64_t)i * F + f], a);
    q[f] = a + bq[f];
  }
  __syncthreads();
  token_scores_softmax(q, kk, sc, n_tok, F, n_head);
  for (int f = tid; f < F; f += 256) {
    const int h = f / dk;
    float a = 0.f;
    for (int t = 0; t < n_tok; ++t) a = fmaf(sc[h * n_tok + t], vv[t * F + f], a);
    ctx[f] = a;
  }
  __syncthreads();
  for (int f = tid; f < F; f += 256) {
    float a = 0.f;
    for (int i = 0; i < F; ++i) a = fmaf(ctx[i], wo_t[(int64_t)i * F + f], a);
    out[(int64_t)b * F + f] = a + bo[f];
  }
}

}  // namespace

extern "C" int srn_gru_recur_last(const float* gi, const float* w_hh_t, const float* b_hh, float* h, int B, int T,
                                  int H, void* stream) {
  SRN_CHECK_ARG(gi && w_hh_t && b_hh && h && B > 0 && T > 0 && H > 0 && 3 * H <= 1024, "gru_recur_last: bad args");
  const int threads = ((3 * H + 63) / 64) * 64;
  hipLaunchKernelGGL((gru_recur_last_kernel<>), dim3(B), dim3(threads), (size_t)(4 * H) * sizeof(float),
                     (hipStream_t)stream, gi, w_hh_t, b_hh, h, T, H);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_gru_recur_last_ragged(const float* gi, const float* w_hh_t, const float* b_hh, float* h,
                                         const int32_t* n_steps, int B, int T_cap, int H, void* stream) {
  SRN_CHECK_ARG(gi && w_hh_t && b_hh && h && n_steps && B > 0 && T_cap > 0 && H > 0 && 3 * H <= 1024,
                "gru_recur_last_ragged: bad args");
  const int threads = ((3 * H + 63) / 64) * 64;
  hipLaunchKernelGGL((gru_recur_last_kernel<SrnLens>), dim3(B), dim3(threads), (size_t)(4 * H) * sizeof(float),
                     (hipStream_t)stream, gi, w_hh_t, b_hh, h, T_cap, H, n_steps);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_zero_rows_ragged(float* x, int64_t bs, int n_cols, const int32_t* n_rows, int B, int rows_cap,
                                    void* stream) {
  SRN_CHECK_ARG(x && n_rows, "zero_rows_ragged: null");
  SRN_CHECK_ARG(n_cols > 0 && B > 0 && B <= 65535 && rows_cap > 0, "zero_rows_ragged: bad sizes");
  const int64_t total = (int64_t)rows_cap * n_cols;
  SRN_CHECK_ARG(B == 1 || bs >= total, "zero_rows_ragged: items of %lld floats overlap at a batch stride of %lld",
                (long long)total, (long long)bs);
  const int64_t chunks = (total + ZR_CHUNK - 1) / ZR_CHUNK;
  SRN_CHECK_ARG(chunks <= 0x7fffffff, "zero_rows_ragged: too large");
  hipLaunchKernelGGL(zero_rows_ragged_kernel, dim3((unsigned)chunks, B), dim3(ZR_THREADS), 0, (hipStream_t)stream, x,
                     bs, n_cols, n_rows, rows_cap);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_replicate_first_row(float* x, int64_t bs, int n_cols, const int32_t* lead, int B, void* stream) {
  SRN_CHECK_ARG(x && lead, "replicate_first_row: null");
  SRN_CHECK_ARG(n_cols > 0 && B > 0 && B <= 65535, "replicate_first_row: bad sizes");
  SRN_CHECK_ARG(B == 1 || bs >= 2 * (int64_t)n_cols, "replicate_first_row: items of two rows overlap at a batch stride of %lld",
                (long long)bs);
  hipLaunchKernelGGL(replicate_first_row_kernel, dim3((unsigned)((n_cols + 255) / 256), B), dim3(256), 0,
                     (hipStream_t)stream, x, bs, n_cols, lead);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_style_token_attention_kv(const float* ref, const float* wq_t, const float* bq, const float* k,
                                            const float* v, const float* wo_t, const float* bo, float* out, int B,
                                            int Dq, int n_tok, int F, int n_head, void* stream) {
  SRN_CHECK_ARG(ref && wq_t && bq && k && v && wo_t && bo && out, "style_token_attention_kv: null");
  SRN_CHECK_ARG(B > 0 && F > 0 && n_head > 0 && F % n_head == 0 && n_tok > 0 && Dq > 0,
                "style_token_attention_kv: bad sizes");
  // token_scores_softmax normalises head h in thread h of the workgroup of 256
  SRN_CHECK_ARG(n_head <= 256, "style_token_attention_kv: n_head %d is above the limit of 256", n_head);
  const size_t smem = (size_t)(2 * F + n_head * n_tok + Dq) * sizeof(float);
  SRN_CHECK_ARG(smem <= 64 * 1024, "style_token_attention_kv: too large for LDS");
  hipLaunchKernelGGL(style_token_attention_kv_kernel, dim3(B), dim3(256), smem, (hipStream_t)stream, ref, wq_t, bq, k,
                     v, wo_t, bo, out, Dq, n_tok, F, n_head);
  SRN_CHECK_LAUNCH();
  return 0;
}
