// row_common.h -- the arithmetic the row kernels of norm_act.hip, train.hip, gst.hip and gst_train.hip share, stated once:
// LayerNorm of a wave-owned row, GroupNorm statistics, GroupNorm + Mish and its gradient, the AdamW update, the GRU
// forward recurrence and the style-token scores + softmax.  Device functions only (every file that includes a
// __global__ function would emit its own copy); the kernels keep their own launch geometry, prefetch and stores.
#pragma once
#include "common.h"

// ---- float4 lane helpers -----------------------------------------------------------------------
template <class F>
__device__ __forceinline__ float4 map4(float4 v, F f) {
  return make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
}
__device__ __forceinline__ float hsum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
// sum of squares about mean
__device__ __forceinline__ float sqdev4(float4 v, float mean) {
  const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
  return (dx * dx + dy * dy) + (dz * dz + dw * dw);
}
// (v - mean) * s; DIV: (v - mean) / s -- the SpeakerAdapter divides by the standard deviation (decoder.py:34-45),
// nn.LayerNorm and GroupNorm multiply by its reciprocal, and the two round differently
template <bool DIV = false>
__device__ __forceinline__ float4 xhat4(float4 v, float mean, float s) {
  return map4(v, [=](float t) { return DIV ? (t - mean) / s : (t - mean) * s; });
}
__device__ __forceinline__ float4 affine4(float4 h, float4 g, float4 b) {
  return make_float4(h.x * g.x + b.x, h.y * g.y + b.y, h.z * g.z + b.z, h.w * g.w + b.w);
}
template <bool DIV = false>
__device__ __forceinline__ float4 norm_affine4(float4 v, float mean, float s, float4 g, float4 b) {
  return affine4(xhat4<DIV>(v, mean, s), g, b);
}

// ---- LayerNorm of a wave-owned row -------------------------------------------------------------
// One wavefront per row of C = 4 c4n <= 1024 channels: lane l holds float4 l, l + 64, .. (up to MAXV of them).
constexpr int MAXV = 4;

__device__ __forceinline__ void row_load(const float* __restrict__ x, float4 (&v)[MAXV], int lane, int c4n) {
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c4 = lane + 64 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < c4n) v[i] = *reinterpret_cast<const float4*>(x + c4 * 4);
  }
}
__device__ __forceinline__ float row_sum(const float4 (&v)[MAXV], int lane, int c4n) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + 64 * i < c4n) sum += hsum4(v[i]);
  return wave_sum(sum);
}
__device__ __forceinline__ float row_sqdev(const float4 (&v)[MAXV], float mean, int lane, int c4n) {
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + 64 * i < c4n) sq += sqdev4(v[i], mean);
  return wave_sum(sq);
}
// y = v <- (v - mean) * s * g + b  (DIV: / s); g, b, y point at the row's channel 0
template <bool DIV = false>
__device__ __forceinline__ void row_norm_affine_store(float4 (&v)[MAXV], float mean, float s, const float* __restrict__ g,
                                                      const float* __restrict__ b, float* __restrict__ y, int lane,
                                                      int c4n) {
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < c4n * 4) {
      v[i] = norm_affine4<DIV>(v[i], mean, s, *reinterpret_cast<const float4*>(g + c),
                               *reinterpret_cast<const float4*>(b + c));
      *reinterpret_cast<float4*>(y + c) = v[i];
    }
  }
}
// nn.LayerNorm of the row in v: the whole of layernorm_kernel and rowln_fwd_kernel per row, and the y2 output of
// resblock_tail_kernel on the row it has just produced
__device__ __forceinline__ void row_layernorm_store(float4 (&v)[MAXV], float eps, const float* __restrict__ g,
                                                    const float* __restrict__ b, float* __restrict__ y, int lane,
                                                    int c4n, float inv_c) {
  const float mean = row_sum(v, lane, c4n) * inv_c;
  const float rstd = 1.0f / sqrtf(row_sqdev(v, mean, lane, c4n) * inv_c + eps);
  row_norm_affine_store(v, mean, rstd, g, b, y, lane, c4n);
}

// ---- GroupNorm ---------------------------------------------------------------------------------
// Statistics from the per-(32 rows x 32 cols) partials the conv epilogue wrote, partials: [b][gn_mt][gn_nt][2], summed in
// fp64: wave w of the 256 threads reduces groups w, w + 4, .. and its lane 0 calls store(g, mean, rstd).
// n_rows: rows the statistics run over (T, or an item's own length when its padded rows are zero).
template <class Store>
__device__ __forceinline__ void gn_group_stats(const float* __restrict__ partials, int b, int T, int C, int groups,
                                               float eps, int n_rows, Store store) {
  const int gn_mt = (T + 31) / 32;
  const int gn_nt = C / 32;
  const int nt_per_g = (C / groups) / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* base = partials + (int64_t)b * gn_mt * gn_nt * 2;
  const int per_g = gn_mt * nt_per_g;
  for (int g = wave; g < groups; g += 4) {
    double s1 = 0.0, s2 = 0.0;
    for (int e = lane; e < per_g; e += 64) {
      const int mt = e / nt_per_g;
      const int nt = g * nt_per_g + (e - mt * nt_per_g);
      const float2 v = *reinterpret_cast<const float2*>(base + ((int64_t)mt * gn_nt + nt) * 2);
      s1 += (double)v.x;
      s2 += (double)v.y;
    }
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    if (lane == 0) {
      const double cnt = (double)max(n_rows, 1) * (double)(C / groups);
      const double mean = s1 / cnt;
      double var = s2 / cnt - mean * mean;
      if (var < 0.0) var = 0.0;
      store(g, (float)mean, (float)(1.0 / sqrt(var + (double)eps)));
    }
  }
}
// mish((x - m) * rs * gamma + beta)
__device__ __forceinline__ float4 gn_mish4(float4 x, float m, float rs, float4 ga, float4 be) {
  return map4(norm_affine4(x, m, rs, ga, be), [](float t) { return srn_mish(t); });
}
// dy * mish'(xhat * gamma + beta): the gradient at the GroupNorm's affine output
__device__ __forceinline__ float4 gn_mish_dg4(float4 dy, float4 xh, float4 ga, float4 be) {
  return mul4(dy, map4(affine4(xh, ga, be), [](float t) { return srn_mish_grad(t); }));
}

// ---- torch.optim.AdamW (decoupled weight decay) on a flat buffer, grid-stride; g is multiplied by gscale first
// (gradient clipping).  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step.
__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, int64_t n, float lr, float beta1, float beta2,
                                             float eps, float wd, float bc1, float bc2, float gscale) {
  const float step = lr / bc1;
  const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gi = g[i] * gscale;
    float pi = p[i] * (1.0f - lr * wd);
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    pi -= step * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    p[i] = pi, m[i] = mi, v[i] = vi;
  }
}

// ---- GRU recurrence on a PRECOMPUTED input projection gi = x W_ih^T + b_ih (B, T, 3H), one workgroup of >= 3H threads
// per batch item, W_hh TRANSPOSED (w_hh_t [H][3H]) so that gate row tid reads consecutive addresses across lanes.
// sm: h[H] | gh[3H] in LDS.  hout (B, H) gets h_T.  KEEP (training): hs (B, T+1, H) keeps h_0..h_T and gates (B, T, 4H)
// per step [r | z | n | W_hn h + b_hn].
template <bool KEEP>
__device__ __forceinline__ void gru_forward(float* sm, const float* __restrict__ gi_all, const float* __restrict__ w_hh_t,
                                            const float* __restrict__ b_hh, float* __restrict__ hout,
                                            float* __restrict__ hs, float* __restrict__ gates, int T, int H) {
  float* sh = sm;
  float* gh = sh + H;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G = 3 * H;
  for (int i = tid; i < H; i += blockDim.x) {
    sh[i] = 0.f;
    if (KEEP) hs[(int64_t)b * (T + 1) * H + i] = 0.f;
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    if (tid < G) {
      float c = 0.f;
      for (int i = 0; i < H; ++i) c = fmaf(w_hh_t[(int64_t)i * G + tid], sh[i], c);
      gh[tid] = c + b_hh[tid];
    }
    __syncthreads();
    if (tid < H) {
      const float* gi = gi_all + ((int64_t)b * T + t) * G;
      const float r = 1.0f / (1.0f + expf(-(gi[tid] + gh[tid])));
      const float z = 1.0f / (1.0f + expf(-(gi[H + tid] + gh[H + tid])));
      const float ghn = gh[2 * H + tid];
      const float n = tanhf(gi[2 * H + tid] + r * ghn);
      // fused by hand: left to the compiler, one instantiation contracted this sum and the other formed both products
      // with a packed multiply, so inference and training disagreed in the last bit of h
      const float h = fmaf(1.0f - z, n, z * sh[tid]);
      sh[tid] = h;
      if (KEEP) {
        float* gt = gates + ((int64_t)b * T + t) * 4 * H;
        gt[tid] = r, gt[H + tid] = z, gt[2 * H + tid] = n, gt[3 * H + tid] = ghn;
        hs[((int64_t)b * (T + 1) + t + 1) * H + tid] = h;
      }
    }
    __syncthreads();
  }
  if (!KEEP)
    for (int i = tid; i < H; i += blockDim.x) hout[(int64_t)b * H + i] = sh[i];
}

// ---- style-token attention: one query (sq [F], LDS) against n_tok keys k (n_tok, F), n_head heads of dk = F / n_head:
// sc[h][t] = softmax_t(q_h . k_h[t] / sqrt(dk)) in LDS.  Called by all 256 threads after sq is visible; sc is visible
// to all on return.
__device__ __forceinline__ void token_scores_softmax(const float* sq, const float* __restrict__ k, float* sc, int n_tok,
                                                     int F, int n_head) {
  const int tid = threadIdx.x, dk = F / n_head;
  const float scale = 1.0f / sqrtf((float)dk);
  for (int i = tid; i < n_head * n_tok; i += 256) {
    const int h = i / n_tok, t = i - h * n_tok;
    float a = 0.f;
    for (int d = 0; d < dk; ++d) a = fmaf(sq[h * dk + d], k[(int64_t)t * F + h * dk + d], a);
    sc[i] = a * scale;
  }
  __syncthreads();
  if (tid < n_head) {
    float m = -INFINITY;
    for (int t = 0; t < n_tok; ++t) m = fmaxf(m, sc[tid * n_tok + t]);
    float s = 0.f;
    for (int t = 0; t < n_tok; ++t) {
      const float e = expf(sc[tid * n_tok + t] - m);
      sc[tid * n_tok + t] = e;
      s += e;
    }
    for (int t = 0; t < n_tok; ++t) sc[tid * n_tok + t] /= s;
  }
  __syncthreads();
}
