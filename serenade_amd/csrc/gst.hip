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

// The carry of a causal stream with the pushed counts as device data (srn_history_carry_ragged).  Grid (entries, B):
// ONE workgroup owns a (buffer, item) pair, so nothing it reads is written by another workgroup, and the table travels
// in the kernel arguments (the call can sit inside a captured hipGraph).  n[b] is one scalar load, uniform over the
// workgroup; an idle item (n[b] == 0) costs that load only.  With m = min(n[b], T / scale) * scale rows pushed, floats
// [m C, (m + H) C) of the item move to [0, H C): the destination lies below the source, so the copy runs upwards in
// blocks of HC_BLOCK floats, each block read into registers by all threads BEFORE any of them stores it (one barrier
// per block).  That is the snapshot (memmove) result for every m >= 1 without a scratch pass: block j's stores end
// where its loads begin or before, later blocks read only above them, and no thread stores block j + 1 before every
// thread has passed the barrier behind block j's loads.
constexpr int HC_THREADS = 256;
constexpr int HC_PER_THREAD = 8;
constexpr int HC_BLOCK = HC_THREADS * HC_PER_THREAD;

__global__ __launch_bounds__(HC_THREADS) void history_carry_ragged_kernel(float* __restrict__ arena,
                                                                          const SrnCarryTable table, SrnLens n) {
  const SrnCarryEntry e = table.e[blockIdx.x];
  const int b = blockIdx.y;
  const int nb = n[b];  // one scalar load, uniform over the workgroup
  const int64_t total = (int64_t)e.H * e.C;
  if (nb == 0 || total == 0) return;  // uniform: the item was idle, its state stays
  float* x = arena + e.off + (int64_t)b * e.bs;
  if (nb < 0) {  // a restart: zero history is the causal padding
    for (int64_t i = threadIdx.x; i < total; i += HC_THREADS) x[i] = 0.f;
    return;
  }
  const int64_t shift = (int64_t)min(nb, e.T / e.scale) * e.scale * e.C;  // m C, with m <= T
  if (shift == 0) return;  // uniform: T < scale, no whole frame fits
  for (int64_t i0 = 0; i0 < total; i0 += HC_BLOCK) {  // the bounds are uniform: every thread meets every barrier
    float v[HC_PER_THREAD];
#pragma unroll
    for (int u = 0; u < HC_PER_THREAD; ++u) {
      const int64_t i = i0 + u * HC_THREADS + threadIdx.x;
      v[u] = i < total ? x[shift + i] : 0.f;
    }
    // the loads have RETURNED before any wave stores: __syncthreads alone leaves them in flight across the barrier
    // (its workgroup-scope fence counts on the CU's in-order memory path), and this kernel should not lean on that
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt and lgkmcnt not waited for (gfx9 encoding)
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HC_PER_THREAD; ++u) {
      const int64_t i = i0 + u * HC_THREADS + threadIdx.x;
      if (i < total) x[i] = v[u];
    }
  }
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

extern "C" int srn_history_carry_ragged(float* arena, const SrnCarryTable* table, const int32_t* n, int B,
                                        void* stream) {
  SRN_CHECK_ARG(arena && table && n, "history_carry_ragged: null");
  SRN_CHECK_ARG(B > 0 && B <= 65535, "history_carry_ragged: bad batch %d", B);
  SRN_CHECK_ARG(table->n > 0 && table->n <= SRN_CARRY_MAX, "history_carry_ragged: %d entries, 1 to %d are taken",
                table->n, SRN_CARRY_MAX);
  for (int i = 0; i < table->n; ++i) {
    const SrnCarryEntry& e = table->e[i];
    SRN_CHECK_ARG(e.off >= 0 && e.H >= 0 && e.T >= 0 && e.C >= 1 && e.scale >= 1,
                  "history_carry_ragged: entry %d: off %lld, H %d, T %d, C %d, scale %d", i, (long long)e.off, e.H, e.T,
                  e.C, e.scale);
    SRN_CHECK_ARG(B == 1 || e.bs >= ((int64_t)e.H + e.T) * e.C,
                  "history_carry_ragged: entry %d: items of %lld floats overlap at a batch stride of %lld", i,
                  (long long)(((int64_t)e.H + e.T) * e.C), (long long)e.bs);
  }
  hipLaunchKernelGGL(history_carry_ragged_kernel, dim3((unsigned)table->n, B), dim3(HC_THREADS), 0,
                     (hipStream_t)stream, arena, *table, n);
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
