// audio.hip -- the arithmetic between the file on disk and the feature front-ends of preprocessing
// (serenade/bin/preprocess.py:405-432) and stage 9's resampling (ssc_postprocessing.py:146).  serenade_amd/audio.py
// drives it; tests/_audio_ref.py is the float64 restatement it is held to.
//   srn_resample      librosa.resample: band-limited rational resampling, polyphase Kaiser-windowed sinc
//   srn_trim_bounds   librosa.effects.trim's frame decisions: one (start, end) per item
//   srn_wave_window   the slice [start, start + n) of every item and np.pad(..., (0, pad), "reflect") in one pass
//
// Numerics: every sum is fp64 in a fixed order that depends on the item alone (never on the batch, the grid or what
// the padding holds), so a batched call is bit for bit its B = 1 calls.  float32 input is widened exactly, float32
// output is the fp64 result rounded once.  Nothing past an item's own samples is ever read.
#include <hip/hip_runtime.h>

#include "common.h"
#include "serenade_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS_TILE = SRN_RESAMPLE_TILE;  // outputs = threads per workgroup of the resampler
constexpr int NT = 256;
constexpr double AMIN2 = 1e-5 * 1e-5;  // librosa's amin = 1e-5 on the rms, squared for the power domain

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {  // b > 0
  const int64_t q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// ------------------------------------------------------------------------------------------------ resampling
// One workgroup per (tile of RS_TILE outputs, item).  Output m reads the inputs j0 - q_lo .. j0 + q_hi around
// j0 = floor(m M / L) against the taps of its phase p = m M mod L; table (K, L) is tap-major, table[k][p] =
// h[p - (k - q_lo) L] (0 beyond the filter), so ascending k is ascending j: the restatement's order.  The tile's input
// span is staged in LDS as fp64 with exact zeros outside the item (a zero term leaves a sum unchanged).
template <typename T>
__global__ __launch_bounds__(RS_TILE) void resample_kernel(const T* __restrict__ x, const int64_t x_bs,
                                                           const int32_t* __restrict__ lens,
                                                           const int32_t* __restrict__ out_lens,
                                                           const double* __restrict__ table, T* __restrict__ y,
                                                           const int64_t y_bs, const int n_out_max, const int L,
                                                           const int M, const int K, const int q_lo, const int span) {
  extern __shared__ double s_x[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = lens[b], n_out = out_lens[b];
  const int64_t m0 = (int64_t)blockIdx.x * RS_TILE, m = m0 + tid;
  T* yb = y + (int64_t)b * y_bs;
  if (m0 >= n_out) {  // a tile past the item: the row's zero tail
    if (m < n_out_max) yb[m] = (T)0;
    return;
  }
  const T* xb = x + (int64_t)b * x_bs;
  const int64_t j_first = floor_div(m0 * M, L) - q_lo;
  for (int i = tid; i < span; i += RS_TILE) {
    const int64_t j = j_first + i;
    s_x[i] = (j >= 0 && j < n) ? (double)xb[j] : 0.0;
  }
  __syncthreads();
  if (m >= n_out_max) return;
  if (m >= n_out) {
    yb[m] = (T)0;
    return;
  }
  const int64_t pos = m * M;
  const int64_t j0 = pos / L;
  const int p = (int)(pos - j0 * L);
  const double* sx = s_x + (int)(j0 - q_lo - j_first);
  const double* tp = table + p;
  double acc = 0.0;
  for (int k = 0; k < K; ++k) acc = acc + sx[k] * tp[(int64_t)k * L];
  yb[m] = (T)acc;
}

// ------------------------------------------------------------------------------------------------ trim
// Mean of squares of every centred frame, one wave per (item, frame): lane l takes the frame's samples l, l + 64, ...
// in turn, then a shuffle tree.  Frame t covers the samples [t hop - frame_length / 2, + frame_length) of the item,
// zeros outside it.
template <typename T>
__global__ __launch_bounds__(NT) void trim_ms_kernel(const T* __restrict__ x, const int64_t x_bs,
                                                     const int32_t* __restrict__ lens, double* __restrict__ ms,
                                                     const int T_max, const int frame_length, const int hop) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const int n = lens[b];
  if (t >= 1 + n / hop) return;  // wave-uniform
  const T* xb = x + (int64_t)b * x_bs;
  const int64_t first = (int64_t)t * hop - frame_length / 2;
  double acc = 0.0;
  for (int i = lane; i < frame_length; i += 64) {
    const int64_t j = first + i;
    const double v = (j >= 0 && j < n) ? (double)xb[j] : 0.0;
    acc = acc + v * v;
  }
  acc = wave_sum_d(acc);
  if (lane == 0) ms[(int64_t)b * T_max + t] = acc / (double)frame_length;
}

// One workgroup per item: the largest frame power, then the first and last frame above the threshold.
__global__ __launch_bounds__(NT) void trim_bounds_kernel(const double* __restrict__ ms,
                                                         const int32_t* __restrict__ lens,
                                                         int32_t* __restrict__ bounds, const int T_max, const int hop,
                                                         const double factor) {
  __shared__ double s_max[NT];
  __shared__ int s_first[NT], s_last[NT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = lens[b], frames = 1 + n / hop;
  const double* row = ms + (int64_t)b * T_max;
  double mx = 0.0;
  for (int t = tid; t < frames; t += NT) mx = fmax(mx, row[t]);
  s_max[tid] = mx;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = fmax(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  const double threshold = factor * fmax(AMIN2, s_max[0]);
  int first = frames, last = -1;
  for (int t = tid; t < frames; t += NT)
    if (fmax(AMIN2, row[t]) > threshold) {
      first = min(first, t);
      last = max(last, t);
    }
  s_first[tid] = first;
  s_last[tid] = last;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_first[tid] = min(s_first[tid], s_first[tid + o]);
      s_last[tid] = max(s_last[tid], s_last[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool any = s_last[0] >= 0;
    bounds[2 * b] = any ? s_first[0] * hop : 0;
    bounds[2 * b + 1] = any ? (int)min((int64_t)n, ((int64_t)s_last[0] + 1) * hop) : 0;
  }
}

// ------------------------------------------------------------------------------------------------ window
template <typename T>
__global__ __launch_bounds__(NT) void wave_window_kernel(const T* __restrict__ x, const int64_t x_bs,
                                                         const int32_t* __restrict__ starts,
                                                         const int32_t* __restrict__ counts, const int pad,
                                                         T* __restrict__ y, const int64_t y_bs, const int width) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= width) return;
  const int n = counts[b];
  int64_t j = -1;  // offset into the item's window [0, n)
  if (i < n)
    j = i;
  else if (i < (int64_t)n + pad)
    j = (int64_t)n - 2 - (i - n);
  y[(int64_t)b * y_bs + i] = (j >= 0 && j < n) ? x[(int64_t)b * x_bs + starts[b] + j] : (T)0;
}

}  // namespace

extern "C" int srn_resample(const void* x, int x_is_f64, int64_t x_bs, const int32_t* lens, const int32_t* out_lens,
                            const double* table, void* y, int64_t y_bs, int B, int N, int n_out_max, int L, int M,
                            int K, int q_lo, void* stream) {
  SRN_CHECK_ARG(x && lens && out_lens && table && y, "resample: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && x_bs >= N && n_out_max > 0 && y_bs >= n_out_max,
                "resample: bad sizes (B %d, N %d, x_bs %lld, n_out_max %d, y_bs %lld)", B, N, (long long)x_bs,
                n_out_max, (long long)y_bs);
  SRN_CHECK_ARG(L >= 1 && M >= 1 && K >= 1 && q_lo >= 0 && q_lo < K, "resample: bad filter (L %d, M %d, K %d, q_lo %d)",
                L, M, K, q_lo);
  // inputs a tile can touch: floor((m0 + TILE - 1) M / L) - floor(m0 M / L) <= ceil((TILE - 1) M / L), plus K taps
  const int64_t span = ((int64_t)(RS_TILE - 1) * M + L - 1) / L + K;
  SRN_CHECK_ARG(span <= SRN_RESAMPLE_MAX_SPAN, "resample: a tile of %d outputs spans %lld inputs, above %d", RS_TILE,
                (long long)span, SRN_RESAMPLE_MAX_SPAN);
  const dim3 grid((n_out_max + RS_TILE - 1) / RS_TILE, B);
  const size_t lds = (size_t)span * sizeof(double);
  if (x_is_f64)
    hipLaunchKernelGGL(resample_kernel<double>, grid, dim3(RS_TILE), lds, (hipStream_t)stream, (const double*)x, x_bs,
                       lens, out_lens, table, (double*)y, y_bs, n_out_max, L, M, K, q_lo, (int)span);
  else
    hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(RS_TILE), lds, (hipStream_t)stream, (const float*)x, x_bs,
                       lens, out_lens, table, (float*)y, y_bs, n_out_max, L, M, K, q_lo, (int)span);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_trim_bounds(const void* x, int x_is_f64, int64_t x_bs, const int32_t* lens, double* ms,
                               int32_t* bounds, int B, int N, int T_max, int frame_length, int hop, double factor,
                               void* stream) {
  SRN_CHECK_ARG(x && lens && ms && bounds, "trim_bounds: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && x_bs >= N && frame_length >= 1 && hop >= 1 && T_max >= 1 + N / hop,
                "trim_bounds: bad sizes (B %d, N %d, x_bs %lld, frame_length %d, hop %d, T_max %d)", B, N,
                (long long)x_bs, frame_length, hop, T_max);
  const dim3 grid((T_max + NT / 64 - 1) / (NT / 64), B);
  if (x_is_f64)
    hipLaunchKernelGGL(trim_ms_kernel<double>, grid, dim3(NT), 0, (hipStream_t)stream, (const double*)x, x_bs, lens,
                       ms, T_max, frame_length, hop);
  else
    hipLaunchKernelGGL(trim_ms_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)x, x_bs, lens, ms,
                       T_max, frame_length, hop);
  SRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, ms, lens, bounds, T_max, hop,
                     factor);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_wave_window(const void* x, int x_is_f64, int64_t x_bs, const int32_t* starts, const int32_t* counts,
                               int pad, void* y, int64_t y_bs, int B, int width, void* stream) {
  SRN_CHECK_ARG(x && starts && counts && y, "wave_window: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && width > 0 && y_bs >= width && pad >= 0 && x_bs > 0,
                "wave_window: bad sizes (B %d, width %d, y_bs %lld, pad %d, x_bs %lld)", B, width, (long long)y_bs, pad,
                (long long)x_bs);
  const dim3 grid((width + NT - 1) / NT, B);
  if (x_is_f64)
    hipLaunchKernelGGL(wave_window_kernel<double>, grid, dim3(NT), 0, (hipStream_t)stream, (const double*)x, x_bs,
                       starts, counts, pad, (double*)y, y_bs, width);
  else
    hipLaunchKernelGGL(wave_window_kernel<float>, grid, dim3(NT), 0, (hipStream_t)stream, (const float*)x, x_bs,
                       starts, counts, pad, (float*)y, y_bs, width);
  SRN_CHECK_LAUNCH();
  return 0;
}
