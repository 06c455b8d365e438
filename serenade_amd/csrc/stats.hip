// stats.hip -- stage 2 of the recipe and the batch the training step eats: what
// serenade/bin/compute_statistics.py:121-144 asks of sklearn's StandardScaler / MinMaxScaler per utterance, and
// FeatsDataset's normalisation (audio_mel_dataset.py:96-110) followed by SSCCollater's padding
// (collaters/ssc.py:50-77).  serenade_amd/stats.py drives it; tests/_stats_ref.py is the float64 restatement it is
// held to.
//   srn_col_moments     per item and column: sum, corrected sum of squared deviations, min, max; per item: the count
//                       of non-finite values
//   srn_scale_collate   (x - sub) / div of the chosen items in the chosen order, padded with +0.0 to (Bout, Tmax, C)
//
// Both read PACKED input: x (R, C) float32, the rows of all items one after another, row_off [B + 1] int64 on the
// device; nothing outside an item is read.  Numerics: every sum is fp64 with contraction off, in an order that depends
// on the item's row count alone (never on B, on where the item lies in the buffer, or on the grid), so a batched call
// is bit for bit its B = 1 calls.  The scaling is one IEEE subtraction and one IEEE division.
#include <hip/hip_runtime.h>

#include "common.h"
#include "serenade_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int COLS = SRN_STATS_COL_TILE;  // columns per workgroup = lanes of a wave
constexpr int PER_THREAD = 4;             // outputs per thread of the collate kernel

// (s[0] + s[1]) + s[2] + s[3] of one column: the waves' partial sums in wave order
__device__ __forceinline__ double combine(const double (*s)[COLS], const int lane) {
  double v = s[0][lane];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) v = v + s[w][lane];
  return v;
}

// One workgroup per (64-column tile, item).  Lane l owns column tile * 64 + l, so a wave reads 256 contiguous bytes
// of a row; wave w takes the item's rows w, w + 4, w + 8, ... in turn.  Two passes over the item: the sums, then the
// deviations from T = sum / n (the corrected two-pass algorithm of Chan, Golub and LeVeque as sklearn states it).
__global__ __launch_bounds__(NT) void col_moments_kernel(const float* __restrict__ x,
                                                         const int64_t* __restrict__ row_off, const int64_t R,
                                                         double* __restrict__ sum, double* __restrict__ m2,
                                                         float* __restrict__ mn, float* __restrict__ mx,
                                                         int32_t* __restrict__ nonfinite, const int C) {
  __shared__ double s_a[WAVES][COLS], s_b[WAVES][COLS];
  __shared__ float s_mn[WAVES][COLS], s_mx[WAVES][COLS];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * COLS + lane;
  const bool live = c < C;
  const int64_t r0 = max(row_off[b], (int64_t)0), r1 = min(row_off[b + 1], R);
  const int64_t n = r1 - r0;
  const float* xc = x + (live ? c : 0);

  double acc = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  if (live)
#pragma unroll 4  // four rows' loads in flight; the additions keep their order
    for (int64_t r = r0 + wave; r < r1; r += WAVES) {
      const float v = xc[r * C];
      acc = acc + (double)v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
      bad += !isfinite(v);
    }
  s_a[wave][lane] = acc;
  s_mn[wave][lane] = lo;
  s_mx[wave][lane] = hi;
  if (bad) atomicAdd(nonfinite + b, bad);
  __syncthreads();
  const double total = combine(s_a, lane);
  const double T = total / (double)n;
  if (wave == 0 && live) {
    for (int w = 1; w < WAVES; ++w) {
      lo = fminf(lo, s_mn[w][lane]);
      hi = fmaxf(hi, s_mx[w][lane]);
    }
    sum[(int64_t)b * C + c] = total;
    mn[(int64_t)b * C + c] = lo;
    mx[(int64_t)b * C + c] = hi;
  }
  __syncthreads();  // s_a is read above and written below

  double sd = 0.0, sd2 = 0.0;
  if (live)
#pragma unroll 4
    for (int64_t r = r0 + wave; r < r1; r += WAVES) {
      const double d = (double)xc[r * C] - T;
      sd = sd + d;
      sd2 = sd2 + d * d;
    }
  s_a[wave][lane] = sd;
  s_b[wave][lane] = sd2;
  __syncthreads();
  if (wave == 0 && live) {
    const double corr = combine(s_a, lane);
    m2[(int64_t)b * C + c] = combine(s_b, lane) - corr * corr / (double)n;
  }
}

// One workgroup per (NT * PER_THREAD consecutive elements of an output item, output item): element i of the item is
// row i / C, column i % C.  Writes every element of out.
template <typename S>
__global__ __launch_bounds__(NT) void scale_collate_kernel(const float* __restrict__ x,
                                                           const int64_t* __restrict__ row_off, const int64_t R,
                                                           const int32_t* __restrict__ order,
                                                           const S* __restrict__ sub, const S* __restrict__ div,
                                                           float* __restrict__ out, const int Tmax, const int B,
                                                           const int C) {
  const int b = blockIdx.y, item = order[b];
  const bool known = item >= 0 && item < B;  // anything else reads as an empty item
  const int64_t r0 = known ? max(row_off[item], (int64_t)0) : 0, r1 = known ? min(row_off[item + 1], R) : 0;
  const int width = Tmax * C;
  const int valid = (int)min(max(r1 - r0, (int64_t)0), (int64_t)Tmax) * C;
  const float* xi = x + r0 * C;
  float* oi = out + (int64_t)b * width;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const int i = (blockIdx.x * PER_THREAD + k) * NT + threadIdx.x;
    if (i >= width) break;
    float y = 0.0f;
    if (i < valid) {
      const int c = i % C;
      y = (float)(((S)xi[i] - sub[c]) / div[c]);
    }
    oi[i] = y;
  }
}

}  // namespace

extern "C" int srn_col_moments(const float* x, const int64_t* row_off, int64_t R, double* sum, double* m2, float* mn,
                               float* mx, int32_t* nonfinite, int B, int C, void* stream) {
  SRN_CHECK_ARG(x && row_off && sum && m2 && mn && mx && nonfinite, "col_moments: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && R > 0, "col_moments: bad sizes (B %d, C %d, R %lld)", B, C,
                (long long)R);
  srn_zero_u32((unsigned*)nonfinite, B, (hipStream_t)stream);
  hipLaunchKernelGGL(col_moments_kernel, dim3((C + COLS - 1) / COLS, B), dim3(NT), 0, (hipStream_t)stream, x, row_off,
                     R, sum, m2, mn, mx, nonfinite, C);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_scale_collate(const float* x, const int64_t* row_off, int64_t R, const int32_t* order,
                                 const void* sub, const void* div, int wide, float* out, int Tmax, int B, int Bout,
                                 int C, void* stream) {
  SRN_CHECK_ARG(x && row_off && order && sub && div && out, "scale_collate: null pointer");
  SRN_CHECK_ARG(B > 0 && Bout > 0 && Bout <= 65535 && C > 0 && Tmax > 0 && R > 0 &&
                    (int64_t)Tmax * C < (1ll << 31) - NT * PER_THREAD,
                "scale_collate: bad sizes (B %d, Bout %d, Tmax %d, C %d, R %lld)", B, Bout, Tmax, C, (long long)R);
  const int per_block = NT * PER_THREAD;
  const dim3 grid((Tmax * C + per_block - 1) / per_block, Bout);
  if (wide)
    hipLaunchKernelGGL(scale_collate_kernel<double>, grid, dim3(NT), 0, (hipStream_t)stream, x, row_off, R, order,
                       (const double*)sub, (const double*)div, out, Tmax, B, C);
  else
    hipLaunchKernelGGL(scale_collate_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, x, row_off, R, order,
                       (const float*)sub, (const float*)div, out, Tmax, B, C);
  SRN_CHECK_LAUNCH();
  return 0;
}
