// contentvec.hip -- the ContentVec / HuBERT content encoder's own kernels (serenade_amd/contentvec.py; the `hubert`
// track of serenade/bin/preprocess.py:41-50,361-368,495-503, transformers' HubertModel).  Everything else of the
// encoder is srn_conv_gemm (feature convs 1-6 with SRN_POST_GELU, projections, Q K^T / P V), srn_layernorm and
// srn_softmax_rows.  Here:
//   srn_cvec_conv0         layer 0 (Cin = 1, k <= 16, any stride), channels-last, with fp64 (sum, sumsq) partials per
//                          (item, 64-frame chunk, channel) over the item's valid frames
//   srn_channel_norm_gelu  GroupNorm(groups = C) from those partials + affine + GELU (HBM-bound)
//   srn_posconv_gelu_res   y = x + GELU(grouped conv(x) + bias): the positional conv (k up to 128, zero padding, rows
//                          at or past the item's length read as zero), exact fp32 on v_mfma_f32_32x32x2_f32
#include <hip/hip_runtime.h>

#include "common.h"
#include "conv_common.h"
#include "serenade_hip.h"

namespace {

constexpr int C0_FRAMES = 64;  // layer-0 frames per workgroup = rows of one partial-sum chunk
constexpr int C0_MAX_K = 16;

// out[b][t][c] = sum_j w[c][j] wave[b][t * stride + j] for t < lens[b], 0 beyond; samples at or past n read as 0.
// partials[b][chunk][c] = (sum, sumsq) in fp64 of the chunk's valid frames (T0 reaches ~1e5 frames for 30 s of audio:
// an fp32 sum of squares would lose digits).
__global__ __launch_bounds__(256) void cvec_conv0_kernel(const float* __restrict__ wave, const int64_t wave_bs,
                                                         const int n, const int32_t* __restrict__ lens,
                                                         const float* __restrict__ w, float* __restrict__ out,
                                                         double* __restrict__ partials, const int T0, const int C,
                                                         const int k, const int stride) {
  extern __shared__ float sig[];  // C0_FRAMES * stride + C0_MAX_K samples
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * C0_FRAMES;
  const int len = min(lens[b], T0);
  const int nf = min(C0_FRAMES, T0 - t0);
  const int ns = C0_FRAMES * stride + C0_MAX_K;
  const float* x = wave + (int64_t)b * wave_bs;
  const int64_t s0 = (int64_t)t0 * stride;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const int64_t s = s0 + i;
    sig[i] = s < n ? x[s] : 0.f;
  }
  __syncthreads();
  double* part = partials + ((int64_t)b * gridDim.x + blockIdx.x) * C * 2;
  for (int c = threadIdx.x; c < C; c += 256) {
    float wr[C0_MAX_K];
#pragma unroll
    for (int j = 0; j < C0_MAX_K; ++j) wr[j] = j < k ? w[c * k + j] : 0.f;
    double s1 = 0.0, s2 = 0.0;
    float* o = out + ((int64_t)b * T0 + t0) * C + c;
    for (int f = 0; f < nf; ++f) {
      const float* sp = sig + f * stride;
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < C0_MAX_K; ++j)
        if (j < k) v = fmaf(wr[j], sp[j], v);
      const bool live = t0 + f < len;
      v = live ? v : 0.f;
      o[(int64_t)f * C] = v;
      if (live) {
        s1 += (double)v;
        s2 += (double)v * (double)v;
      }
    }
    part[2 * c] = s1;
    part[2 * c + 1] = s2;
  }
}

// per (item, channel): mean and 1 / sqrt(var + eps) over the item's valid frames, from the chunk partials in fp64
__global__ __launch_bounds__(256) void channel_stats_kernel(const double* __restrict__ partials, const int n_chunks,
                                                            const int32_t* __restrict__ lens, const int T,
                                                            float* __restrict__ stats, const int C, const float eps) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double* p = partials + (int64_t)b * n_chunks * C * 2 + 2 * c;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < n_chunks; ++i) {
    s1 += p[(int64_t)i * C * 2];
    s2 += p[(int64_t)i * C * 2 + 1];
  }
  const int nv = max(min(lens[b], T), 1);
  const double mean = s1 / nv;
  const double var = fmax(s2 / nv - mean * mean, 0.0);
  stats[((int64_t)b * C + c) * 2] = (float)mean;
  stats[((int64_t)b * C + c) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// y = GELU((x - mean) * rstd * gamma + beta) on valid rows, 0 on padded rows; 16 B per lane along the channels
__global__ __launch_bounds__(256) void channel_norm_gelu_kernel(const float* x, const float* __restrict__ stats,
                                                                const int32_t* __restrict__ lens,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* y, const int T,
                                                                const int C) {
  const int b = blockIdx.y;
  const int len = min(lens[b], T);
  const int cq = C / 4;
  const int64_t nq = (int64_t)T * cq;
  const float4* xb = reinterpret_cast<const float4*>(x + (int64_t)b * T * C);
  float4* yb = reinterpret_cast<float4*>(y + (int64_t)b * T * C);
  const float* st = stats + (int64_t)b * C * 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / cq);
    const int c = (int)(i - (int64_t)t * cq) * 4;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < len) {
      const float4 v = xb[i];
      const float4 s01 = *reinterpret_cast<const float4*>(st + 2 * c);
      const float4 s23 = *reinterpret_cast<const float4*>(st + 2 * c + 4);
      const float4 g = *reinterpret_cast<const float4*>(gamma + c);
      const float4 be = *reinterpret_cast<const float4*>(beta + c);
      o.x = srn_gelu_erf((v.x - s01.x) * s01.y * g.x + be.x);
      o.y = srn_gelu_erf((v.y - s01.z) * s01.w * g.y + be.y);
      o.z = srn_gelu_erf((v.z - s23.x) * s23.y * g.z + be.z);
      o.w = srn_gelu_erf((v.w - s23.z) * s23.w * g.w + be.w);
    }
    yb[i] = o;
  }
}

constexpr int PC_BM = 128;     // output rows per workgroup: 4 waves x 32
constexpr int PC_MAX_K = 128;  // taps
constexpr int PC_MAX_CG = 64;  // channels per group
constexpr int PC_LDS_MAX = (PC_BM + PC_MAX_K - 1) * (PC_MAX_CG + 1) * 4;

// y[b][t][g Cg + n] = x[b][t][g Cg + n] + GELU(bias[g Cg + n] + sum_{j, c} w[g][j][c][n] xz[b][t + j - pad][g Cg + c])
// xz: x with rows outside [0, min(lens[b], T)) read as zero.  One workgroup = 128 output rows of one group of one item;
// the input window (128 + k - 1 rows x Cg channels, row stride Cg + 1: conflict-free column reads) sits in LDS.  Wave w
// owns rows [32 w, 32 w + 32) and NB 32-column blocks; A (rows x channels) comes from LDS, B from the packed weights
// w[g][j][c][NB * 32] (zero columns past Cg), one k-ordered exact-fp32 fma chain per output.
template <int NB>
__global__ __launch_bounds__(256) void posconv_gelu_res_kernel(const float* __restrict__ x,
                                                               const int32_t* __restrict__ lens,
                                                               const float* __restrict__ wp,
                                                               const float* __restrict__ bias, float* __restrict__ y,
                                                               const int T, const int C, const int Cg, const int k,
                                                               const int pad) {
  extern __shared__ float tile[];
  const int g = blockIdx.y, b = blockIdx.z;
  const int t0 = blockIdx.x * PC_BM;
  const int len = lens ? min(lens[b], T) : T;
  const int S = Cg + 1;
  const int rows = PC_BM + k - 1;
  const float* xb = x + (int64_t)b * T * C + g * Cg;
  for (int i = threadIdx.x; i < rows * Cg; i += 256) {
    const int r = i / Cg, c = i - r * Cg;
    const int src = t0 - pad + r;
    tile[r * S + c] = (src >= 0 && src < len) ? xb[(int64_t)src * C + c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, kh = lane >> 5;
  constexpr int NP = NB * 32;
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
  const float* wg = wp + (int64_t)g * k * Cg * NP + kh * NP + li;
  const float* arow = tile + (wave * 32 + li) * S + kh;
  for (int j = 0; j < k; ++j) {
    const float* wj = wg + (int64_t)j * Cg * NP;
    const float* aj = arow + j * S;
#pragma unroll 8
    for (int c = 0; c < Cg; c += 2) {
      const float a = aj[c];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wj[c * NP + nb * 32], acc[nb], 0, 0, 0);
    }
  }
  const float* xo = x + (int64_t)b * T * C + g * Cg;
  float* yo = y + (int64_t)b * T * C + g * Cg;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = nb * 32 + li;
    if (col >= Cg) continue;
    const float bv = bias[g * Cg + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = t0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (row < T) {
        const int64_t e = (int64_t)row * C + col;
        yo[e] = xo[e] + srn_gelu_erf(acc[nb][r] + bv);
      }
    }
  }
}

}  // namespace

extern "C" int srn_frame_stats_chunks(int T) { return (T + C0_FRAMES - 1) / C0_FRAMES; }

extern "C" int srn_cvec_conv0(const float* wave, int64_t wave_bs, int n, const int32_t* lens, const float* w,
                              float* out, double* partials, int B, int T0, int C, int k, int stride, void* stream) {
  SRN_CHECK_ARG(wave && lens && w && out && partials, "cvec_conv0: null pointer");
  SRN_CHECK_ARG(B > 0 && T0 > 0 && C > 0 && n > 0 && k >= 1 && k <= C0_MAX_K && stride >= 1 && stride <= 64,
                "cvec_conv0: bad sizes (B %d, T0 %d, C %d, n %d, k %d, stride %d)", B, T0, C, n, k, stride);
  SRN_CHECK_ARG(wave_bs >= n, "cvec_conv0: wave_bs %lld < n %d", (long long)wave_bs, n);
  const int chunks = srn_frame_stats_chunks(T0);
  const int smem = (C0_FRAMES * stride + C0_MAX_K) * 4;
  hipLaunchKernelGGL(cvec_conv0_kernel, dim3(chunks, B), dim3(256), smem, (hipStream_t)stream, wave, wave_bs, n, lens,
                     w, out, partials, T0, C, k, stride);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_channel_norm_gelu(const float* x, const double* partials, int n_chunks, const int32_t* lens,
                                     const float* gamma, const float* beta, float* stats, float* y, int B, int T, int C,
                                     float eps, void* stream) {
  SRN_CHECK_ARG(x && partials && lens && gamma && beta && stats && y, "channel_norm_gelu: null pointer");
  SRN_CHECK_ARG(B > 0 && T > 0 && C > 0 && C % 4 == 0 && n_chunks == srn_frame_stats_chunks(T),
                "channel_norm_gelu: bad sizes (B %d, T %d, C %d, n_chunks %d)", B, T, C, n_chunks);
  SRN_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(stats) |
                  reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta)) & 15) == 0,
                "channel_norm_gelu: x, y, stats, gamma, beta must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(channel_stats_kernel, dim3((C + 255) / 256, B), dim3(256), 0, st, partials, n_chunks, lens, T,
                     stats, C, eps);
  SRN_CHECK_LAUNCH();
  const int64_t nq = (int64_t)T * (C / 4);
  const int blocks = (int)((nq + 255) / 256 < 2048 ? (nq + 255) / 256 : 2048);
  hipLaunchKernelGGL(channel_norm_gelu_kernel, dim3(blocks, B), dim3(256), 0, st, x, stats, lens, gamma, beta, y, T, C);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_posconv_gelu_res(const float* x, const int32_t* lens, const float* w, const float* bias, float* y,
                                    int B, int T, int C, int groups, int k, int pad, void* stream) {
  SRN_CHECK_ARG(x && w && bias && y && x != y, "posconv_gelu_res: null pointer, or y aliases x");
  SRN_CHECK_ARG(B > 0 && T > 0 && groups > 0 && C % groups == 0, "posconv_gelu_res: bad sizes");
  const int Cg = C / groups;
  SRN_CHECK_ARG(Cg % 4 == 0 && Cg <= PC_MAX_CG && k >= 1 && k <= PC_MAX_K && pad >= 0 && pad < k,
                "posconv_gelu_res: needs channels per group %% 4 == 0 and <= %d, 1 <= k <= %d, 0 <= pad < k (got %d, %d, %d)",
                PC_MAX_CG, PC_MAX_K, Cg, k, pad);
  const int smem = (PC_BM + k - 1) * (Cg + 1) * 4;
  const dim3 grid((T + PC_BM - 1) / PC_BM, groups, B);
  hipStream_t st = (hipStream_t)stream;
  if (Cg <= 32) {
    static SrnSmemAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(posconv_gelu_res_kernel<1>), PC_LDS_MAX)) return e;
    hipLaunchKernelGGL(posconv_gelu_res_kernel<1>, grid, dim3(256), smem, st, x, lens, w, bias, y, T, C, Cg, k, pad);
  } else {
    static SrnSmemAttr attr;
    if (const int e = attr.ensure(reinterpret_cast<const void*>(posconv_gelu_res_kernel<2>), PC_LDS_MAX)) return e;
    hipLaunchKernelGGL(posconv_gelu_res_kernel<2>, grid, dim3(256), smem, st, x, lens, w, bias, y, T, C, Cg, k, pad);
  }
  SRN_CHECK_LAUNCH();
  return 0;
}
