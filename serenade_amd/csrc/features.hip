// features.hip -- the feature front-end in front of the hot path: log-mel spectrogram and
// A-weighted loudness of serenade/bin/preprocess.py:126-203 (librosa stft / filters.mel / perceptual_weighting there).
//
// The STFT itself is one strided implicit-GEMM through srn_conv_gemm (the signal viewed as rows of 16 samples, a frame
// = n_fft / 16 taps, hop / 16 rows of stride, weights = window x DFT basis, [re | im] output columns); this file holds
// the byte-moving and elementwise ends: reflection padding, magnitude -> mel -> log, and power -> dB (with the
// per-utterance top_db floor) -> A-weighting -> amplitude -> frame mean -> log.  All HBM-bound and tiny next to the
// model (8.4 MFLOP per frame for the loudness STFT, 0.5 for the mel one).  Each of the three ends has a ragged twin for
// a padded batch of unequal utterances (per-item sample / frame counts): every item gets what its own B = 1 call gets.
#include <hip/hip_runtime.h>

#include "common.h"
#include "serenade_hip.h"

namespace {

// out[b][i] = x[b][reflect(i - pad)] for i < n + 2 pad, 0 up to ld (numpy.pad mode="reflect": no edge repeat)
__global__ __launch_bounds__(256) void pad_signal_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                        const int n, const int pad, const int ld, const int zero) {
  const int b = blockIdx.y;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ld; i += gridDim.x * 256) {
    float v = 0.f;
    if (i < n + 2 * pad) {
      int j = i - pad;
      const bool outside = j < 0 || j >= n;
      if (j < 0) j = -j;
      if (j >= n) j = 2 * (n - 1) - j;
      j = min(max(j, 0), n - 1);
      v = (zero && outside) ? 0.f : x[(int64_t)b * n + j];
    }
    out[(int64_t)b * ld + i] = v;
  }
}

// log_b(a), b = e | 2 | 10 (log_mode 0 | 2 | 10), for finite a > 0, to about an ulp of the result at any magnitude.
// logf / log2f / log10f take the hardware log2 of a itself, which errs by an ulp of ITS result: at the floor
// a = eps = 1e-10 that is an ulp of 33, and ln(eps) came out two float32 spacings off (3.2e-6; the float64 reference
// rounds to the spacing between).  So the exponent is split off first: a = m 2^e with m in [sqrt(1/2), sqrt(2)),
// log2 m is at most 0.5 in magnitude, and e log_b(2) is added from a constant in two parts whose high part has 12 bits
// (e hi is exact) with one rounding.
__device__ __forceinline__ float log_base(const float a, const int log_mode) {
  int e;
  float m = frexpf(a, &e);  // m in [0.5, 1)
  if (m < 0.70710678f) {
    m *= 2.f;
    --e;
  }
  const float l2 = log2f(m), ef = (float)e;
  if (log_mode == 2) return ef + l2;
  const float hi = log_mode == 10 ? 0.301025390625f : 0.693145751953125f;  // log_b(2) = hi + lo
  const float lo = log_mode == 10 ? 4.60503898e-06f : 1.42860682e-06f;
  return fmaf(ef, hi, fmaf(ef, lo, l2 * (hi + lo)));
}

// one frame by one workgroup of 128: |X| of the nb bins into LDS (mag), then mel bin m = threadIdx (mel_t is
// (nb, n_mels): lanes read consecutive addresses), o[m] = log(max(eps, dot)).  The arithmetic of logmel_kernel and
// logmel_ragged_kernel, stated once.
__device__ __forceinline__ void logmel_row(const float* __restrict__ row, const float* __restrict__ mel_t,
                                           float* __restrict__ o, float* mag, const int nb, const int n_mels,
                                           const float eps, const int log_mode) {
  for (int f = threadIdx.x; f < nb; f += 128) {
    const float re = row[f], im = row[nb + f];
    mag[f] = sqrtf(re * re + im * im);
  }
  __syncthreads();
  for (int m = threadIdx.x; m < n_mels; m += 128) {
    float a = 0.f;
    for (int f = 0; f < nb; ++f) a = fmaf(mag[f], mel_t[f * n_mels + m], a);
    a = fmaxf(a, eps);
    o[m] = log_base(a, log_mode);
  }
}

// one workgroup per frame
__global__ __launch_bounds__(128) void logmel_kernel(const float* __restrict__ spec, const float* __restrict__ mel_t,
                                                     float* __restrict__ out, const int nb, const int ld,
                                                     const int n_mels, const float eps, const int log_mode) {
  extern __shared__ float mag[];
  const int64_t fr = blockIdx.x;
  logmel_row(spec + fr * ld, mel_t, out + fr * n_mels, mag, nb, n_mels, eps, log_mode);
}

// one workgroup per (frame, item): logmel_row on the frames t < frames[b]; a frame at or past it is written as 0 and
// its workgroup leaves before it loads anything of spec
__global__ __launch_bounds__(128) void logmel_ragged_kernel(const float* __restrict__ spec,
                                                            const float* __restrict__ mel_t,
                                                            const int32_t* __restrict__ frames,
                                                            float* __restrict__ out, const int T, const int nb,
                                                            const int ld, const int n_mels, const float eps,
                                                            const int log_mode) {
  extern __shared__ float mag[];
  const int t = blockIdx.x, b = blockIdx.y;
  const int64_t fr = (int64_t)b * T + t;
  float* o = out + fr * n_mels;
  if (t >= min(frames[b], T)) {  // the same in every lane: the whole workgroup leaves
    for (int m = threadIdx.x; m < n_mels; m += 128) o[m] = 0.f;
    return;
  }
  logmel_row(spec + fr * ld, mel_t, o, mag, nb, n_mels, eps, log_mode);
}

// out[b][pad + j] = x[b][j] for j < L = min(lens[b], n), 0 everywhere else up to ld (numpy.pad mode="constant" of the
// item on its own); x[b][j] is not read for j >= L
__global__ __launch_bounds__(256) void pad_ragged_zero_kernel(const float* __restrict__ x, const int64_t x_bs,
                                                              const int32_t* __restrict__ lens,
                                                              float* __restrict__ out, const int n, const int pad,
                                                              const int ld) {
  const int b = blockIdx.y;
  const int L = min(lens[b], n);
  const float* xb = x + (int64_t)b * x_bs;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ld; i += gridDim.x * 256) {
    const int j = i - pad;
    out[(int64_t)b * ld + i] = (j >= 0 && j < L) ? xb[j] : 0.f;
  }
}

// the library's one zero-fill (common.h: srn_zero_u32 says why it is a kernel)
__global__ void zero_u32_kernel(unsigned* __restrict__ p, const int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// the running maximum of one frame's bin powers, a workgroup of 256 striding over the bins
__device__ __forceinline__ float power_row_max(const float* __restrict__ row, const int nb, float m) {
  for (int f = threadIdx.x; f < nb; f += 256) {
    const float re = row[f], im = row[nb + f];
    m = fmaxf(m, re * re + im * im);
  }
  return m;
}

// per-utterance maximum of the power spectrogram (non-negative floats order like their bit patterns, so an integer
// atomicMax gives a bit-reproducible result); gmax must be zeroed by the caller
__global__ __launch_bounds__(256) void power_max_kernel(const float* __restrict__ spec, unsigned* __restrict__ gmax,
                                                        const int frames, const int nb, const int ld) {
  const int b = blockIdx.y;
  float m = 0.f;
  for (int fr = blockIdx.x; fr < frames; fr += gridDim.x)
    m = power_row_max(spec + ((int64_t)b * frames + fr) * ld, nb, m);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) atomicMax(gmax + b, __float_as_uint(m));
}

// the same over the item's own frames t < frames[b] of a (B, T) batch: rows at or past it are not read
__global__ __launch_bounds__(256) void power_max_ragged_kernel(const float* __restrict__ spec,
                                                               const int32_t* __restrict__ frames,
                                                               unsigned* __restrict__ gmax, const int T, const int nb,
                                                               const int ld) {
  const int b = blockIdx.y;
  const int len = min(frames[b], T);
  if ((int)blockIdx.x >= len) return;
  float m = 0.f;
  for (int fr = blockIdx.x; fr < len; fr += gridDim.x) m = power_row_max(spec + ((int64_t)b * T + fr) * ld, nb, m);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) atomicMax(gmax + b, __float_as_uint(m));
}

// one frame by one workgroup of 256: mean over bins of 10^((max(10 log10(max(amin, p)), top) + A[f]) / 20), then
// log(. + add_eps); `top` from the utterance's maximum power gmax_b.  The arithmetic of loudness_kernel and
// loudness_ragged_kernel, stated once; red: 4 floats of LDS.
__device__ __forceinline__ float loudness_row(const float* __restrict__ row, const float* __restrict__ aw,
                                              const unsigned gmax_b, float* red, const int nb, const float amin,
                                              const float top_db, const float add_eps) {
  const float floor_db = 10.f * log10f(fmaxf(amin, __uint_as_float(gmax_b))) - top_db;
  float s = 0.f;
  for (int f = threadIdx.x; f < nb; f += 256) {
    const float re = row[f], im = row[nb + f];
    const float db = fmaxf(10.f * log10f(fmaxf(amin, re * re + im * im)), floor_db) + aw[f];
    s += exp10f(0.05f * db);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return logf(((red[0] + red[1]) + (red[2] + red[3])) / nb + add_eps);
}

// one workgroup per frame
__global__ __launch_bounds__(256) void loudness_kernel(const float* __restrict__ spec, const float* __restrict__ aw,
                                                       const unsigned* __restrict__ gmax, float* __restrict__ out,
                                                       const int frames, const int nb, const int ld, const float amin,
                                                       const float top_db, const float add_eps) {
  __shared__ float red[4];
  const int b = blockIdx.y, fr = blockIdx.x;
  const float v = loudness_row(spec + ((int64_t)b * frames + fr) * ld, aw, gmax[b], red, nb, amin, top_db, add_eps);
  if (threadIdx.x == 0) out[(int64_t)b * frames + fr] = v;
}

// one workgroup per (frame, item): loudness_row on the frames t < frames[b] with the item's own maximum; a frame at or
// past it is written as 0 and its workgroup leaves before it loads anything of spec, aw or gmax
__global__ __launch_bounds__(256) void loudness_ragged_kernel(const float* __restrict__ spec,
                                                              const float* __restrict__ aw,
                                                              const int32_t* __restrict__ frames,
                                                              const unsigned* __restrict__ gmax,
                                                              float* __restrict__ out, const int T, const int nb,
                                                              const int ld, const float amin, const float top_db,
                                                              const float add_eps) {
  __shared__ float red[4];
  const int b = blockIdx.y, t = blockIdx.x;
  if (t >= min(frames[b], T)) {  // the same in every lane: the whole workgroup leaves
    if (threadIdx.x == 0) out[(int64_t)b * T + t] = 0.f;
    return;
  }
  const float v = loudness_row(spec + ((int64_t)b * T + t) * ld, aw, gmax[b], red, nb, amin, top_db, add_eps);
  if (threadIdx.x == 0) out[(int64_t)b * T + t] = v;
}

}  // namespace

void srn_zero_u32(unsigned* p, const int n, hipStream_t stream) {
  hipLaunchKernelGGL(zero_u32_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, n);
}

extern "C" int srn_pad_signal(const float* x, float* out, int B, int n, int pad, int ld, int mode, void* stream) {
  SRN_CHECK_ARG(x && out && B > 0 && n > 1 && pad >= 0 && ld >= n + 2 * pad && (mode == 0 || mode == 1),
                "pad_signal: bad args");
  SRN_CHECK_ARG(B <= 65535, "pad_signal: B %d is above the limit of 65535", B);
  SRN_CHECK_ARG(mode == 1 || pad < n, "pad_signal: reflect padding of %d needs more than %d samples", pad, n);
  int bx = (ld + 255) / 256;
  bx = bx > 4096 ? 4096 : bx;
  hipLaunchKernelGGL(pad_signal_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream, x, out, n, pad, ld, mode);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_logmel(const float* spec, const float* mel_t, float* out, int64_t frames, int n_bins, int ld,
                          int n_mels, float eps, int log_mode, void* stream) {
  SRN_CHECK_ARG(spec && mel_t && out && frames > 0 && frames < (1ll << 31) && n_bins > 0 && ld >= 2 * n_bins &&
                    n_mels > 0 && (log_mode == 0 || log_mode == 2 || log_mode == 10) && n_bins <= 8192,
                "logmel: bad args");
  hipLaunchKernelGGL(logmel_kernel, dim3((unsigned)frames), dim3(128), (size_t)n_bins * sizeof(float),
                     (hipStream_t)stream, spec, mel_t, out, n_bins, ld, n_mels, eps, log_mode);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_loudness(const float* spec, const float* a_weight_db, unsigned* gmax_ws, float* out, int B,
                            int frames, int n_bins, int ld, float amin, float top_db, float add_eps, void* stream) {
  SRN_CHECK_ARG(spec && a_weight_db && gmax_ws && out && B > 0 && frames > 0 && n_bins > 0 && ld >= 2 * n_bins,
                "loudness: bad args");
  SRN_CHECK_ARG(B <= 65535, "loudness: B %d is above the limit of 65535", B);
  hipStream_t st = (hipStream_t)stream;
  srn_zero_u32(gmax_ws, B, st);
  hipLaunchKernelGGL(power_max_kernel, dim3(frames < 512 ? frames : 512, B), dim3(256), 0, st, spec, gmax_ws, frames,
                     n_bins, ld);
  hipLaunchKernelGGL(loudness_kernel, dim3(frames, B), dim3(256), 0, st, spec, a_weight_db, gmax_ws, out, frames,
                     n_bins, ld, amin, top_db, add_eps);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_pad_ragged_zero(const float* x, int64_t x_bs, const int32_t* lens, float* out, int B, int n, int pad,
                                   int ld, void* stream) {
  SRN_CHECK_ARG(x && lens && out, "pad_ragged_zero: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && n > 0 && pad >= 0 && ld >= n + 2 * pad && x_bs >= n,
                "pad_ragged_zero: bad sizes (B %d, n %d, pad %d, ld %d, x_bs %lld)", B, n, pad, ld, (long long)x_bs);
  int bx = (ld + 255) / 256;
  bx = bx > 4096 ? 4096 : bx;
  hipLaunchKernelGGL(pad_ragged_zero_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, lens, out, n,
                     pad, ld);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_logmel_ragged(const float* spec, const float* mel_t, const int32_t* frames, float* out, int B,
                                 int T, int n_bins, int ld, int n_mels, float eps, int log_mode, void* stream) {
  SRN_CHECK_ARG(spec && mel_t && frames && out, "logmel_ragged: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && n_bins > 0 && n_bins <= 8192 && ld >= 2 * n_bins && n_mels > 0 &&
                    (log_mode == 0 || log_mode == 2 || log_mode == 10),
                "logmel_ragged: bad args (B %d, T %d, n_bins %d, ld %d, n_mels %d, log_mode %d)", B, T, n_bins, ld,
                n_mels, log_mode);
  hipLaunchKernelGGL(logmel_ragged_kernel, dim3(T, B), dim3(128), (size_t)n_bins * sizeof(float), (hipStream_t)stream,
                     spec, mel_t, frames, out, T, n_bins, ld, n_mels, eps, log_mode);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_loudness_ragged(const float* spec, const float* a_weight_db, const int32_t* frames,
                                   unsigned* gmax_ws, float* out, int B, int T, int n_bins, int ld, float amin,
                                   float top_db, float add_eps, void* stream) {
  SRN_CHECK_ARG(spec && a_weight_db && frames && gmax_ws && out, "loudness_ragged: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && n_bins > 0 && ld >= 2 * n_bins,
                "loudness_ragged: bad args (B %d, T %d, n_bins %d, ld %d)", B, T, n_bins, ld);
  hipStream_t st = (hipStream_t)stream;
  srn_zero_u32(gmax_ws, B, st);
  hipLaunchKernelGGL(power_max_ragged_kernel, dim3(T < 512 ? T : 512, B), dim3(256), 0, st, spec, frames, gmax_ws, T,
                     n_bins, ld);
  hipLaunchKernelGGL(loudness_ragged_kernel, dim3(T, B), dim3(256), 0, st, spec, a_weight_db, frames, gmax_ws, out, T,
                     n_bins, ld, amin, top_db, add_eps);
  SRN_CHECK_LAUNCH();
  return 0;
}
