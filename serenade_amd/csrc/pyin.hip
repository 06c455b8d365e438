// pyin.hip -- probabilistic YIN F0 estimation (librosa 0.10 `librosa.pyin`), the f0 contour that the note transcriber's
// FramewiseDecoder turns into note pitches (serenade/modules/phoneme_midi/decoding.py:36-45).  serenade_amd/pitch.py
// drives it; tests/_pyin_ref.py is the float64 restatement it is held to, state for state.
//   srn_pyin_observe   steps 1-5: per (item, frame) the cumulative mean normalised difference, parabolic shifts,
//                      troughs, their threshold-prior probabilities and the voiced observation row
//   srn_pyin_viterbi   steps 6-7: per item the log-domain Viterbi over 2 n_bins states, backtrack, f0 and flags
//
// Numerics: fp64 throughout, contraction off, so that every rounding is the restatement's: the sums it pins as
// sequential (energy, cumulative mean, autocorrelation over j, threshold prior over k, voiced probability over bins)
// run in one lane in the same order.  Every data-independent constant (thresholds, beta and Boltzmann factors, the
// log-transition band, log p_init, the bin frequencies) comes from the host.
#include <hip/hip_runtime.h>

#include "common.h"
#include "serenade_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT_OBS = 256;
constexpr int NT_VIT = 1024;
constexpr double kTiny = 2.2250738585072014e-308;  // np.finfo(np.float64).tiny

__device__ __forceinline__ int popc(unsigned long long m) { return __popcll(m); }

// (value, index) maximum with the first index winning a tie
__device__ __forceinline__ void argmax_merge(double& v, int& i, double v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) argmax_merge(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
}

// One workgroup per (frame t, item b).  LDS (doubles): y[L], c[L] (later the cumulative sum of d), d[max_p + 1],
// x[nf] (cmnd), sh[nf] (shifts), row[n_bins + 1]; then th[nf], pr[nf] (doubles) and ti[nf], tb[nf], nk[K], cp[K]
// (ints), L = W + max_p + 1, nf = max_p - min_p + 1, K = n_thresholds.
__global__ __launch_bounds__(NT_OBS) void pyin_observe_kernel(
    const float* __restrict__ xin, const int64_t x_bs, const int32_t* __restrict__ lens,
    const int32_t* __restrict__ frames, const double* __restrict__ thr, const double* __restrict__ beta,
    const double* __restrict__ bfact, const double* __restrict__ bexp, const double* __restrict__ notrough,
    double* __restrict__ obs, double* __restrict__ vprob, const int T, const int W, const int hop, const int pad,
    const int min_p, const int max_p, const int K, const double sr, const double f_min, const double bins_per_octave,
    const int n_bins) {
  extern __shared__ double sm[];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int L = W + max_p + 1, nf = max_p - min_p + 1;
  double* y = sm;
  double* c = y + L;
  double* d = c + L;
  double* x = d + max_p + 1;
  double* sh = x + nf;
  double* row = sh + nf;
  double* th = row + n_bins + 1;
  double* pr = th + nf;
  int* ti = reinterpret_cast<int*>(pr + nf);
  int* tb = ti + nf;
  int* nk = tb + nf;
  int* cp = nk + K;

  double* orow = obs + ((int64_t)b * T + t) * n_bins;
  if (t >= frames[b]) {
    if (tid == 0) vprob[(int64_t)b * T + t] = 0.0;
    return;
  }
  // step 1: the frame, zero outside [0, len) (centre padding and the item's own end), as float64
  const int len = lens[b];
  const float* xb = xin + (int64_t)b * x_bs;
  const int s0 = t * hop - pad;
  for (int k = tid; k < L; k += NT_OBS) {
    const int s = s0 + k;
    y[k] = (s >= 0 && s < len) ? (double)xb[s] : 0.0;
  }
  for (int k = tid; k <= n_bins; k += NT_OBS) row[k] = 0.0;
  for (int k = tid; k < K; k += NT_OBS) cp[k] = 0;
  __syncthreads();
  // step 2: c = running sum of y^2 (lane 0); acf[tau] = sum_{j=1..W} y[j] y[j + tau] (one lane per tau), into d
  if (tid == 0) {
    double r = 0.0;
    for (int k = 0; k < L; ++k) {
      r = r + y[k] * y[k];
      c[k] = r;
    }
  }
  for (int tau = tid; tau <= max_p; tau += NT_OBS) {
    if (tau == 0) continue;
    double a = 0.0;
    for (int j = 1; j <= W; ++j) a = a + y[j] * y[j + tau];
    d[tau] = fabs(a) < 1e-6 ? 0.0 : a;
  }
  __syncthreads();
  {
    double e0 = c[W] - c[0];
    if (fabs(e0) < 1e-6) e0 = 0.0;
    for (int tau = tid + 1; tau <= max_p; tau += NT_OBS) {
      double e = c[W + tau] - c[tau];
      if (fabs(e) < 1e-6) e = 0.0;
      d[tau] = (e0 + e) - 2.0 * d[tau];
    }
  }
  __syncthreads();
  if (tid == 0) {  // cumulative sum of d[1 .. max_p] into c[1 .. max_p] (c is free now)
    double r = 0.0;
    for (int tau = 1; tau <= max_p; ++tau) {
      r = r + d[tau];
      c[tau] = r;
    }
  }
  __syncthreads();
  for (int i = tid; i < nf; i += NT_OBS) {
    const int tau = min_p + i;
    x[i] = d[tau] / (c[tau] / (double)tau + kTiny);
  }
  __syncthreads();
  // step 3: parabolic shifts (0 at both ends)
  for (int i = tid; i < nf; i += NT_OBS) {
    double s = 0.0;
    if (i > 0 && i < nf - 1) {
      const double a = x[i + 1] + x[i - 1] - 2.0 * x[i];
      const double bb = (x[i + 1] - x[i - 1]) / 2.0;
      s = fabs(bb) >= fabs(a) ? 0.0 : -bb / a;
    }
    sh[i] = s;
  }
  __syncthreads();
  // step 4: troughs and their probabilities, in wave 0
  if (tid < 64) {
    const int lane = tid;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int R = 0;
    for (int base = 0; base < nf; base += 64) {
      const int i = base + lane;
      bool f = false;
      if (i < nf) {
        if (i == 0)
          f = x[0] < x[1];
        else if (i == nf - 1)
          f = x[i] < x[i - 1];
        else
          f = x[i] < x[i - 1] && x[i] <= x[i + 1];
      }
      const unsigned long long m = __ballot(f);
      if (f) {
        const int slot = R + popc(m & lt);
        ti[slot] = i;
        th[slot] = x[i];
      }
      R += popc(m);
    }
    wave_sync();
    double vs = 0.0;
    if (R > 0) {
      // troughs below each threshold
      for (int k = lane; k < K; k += 64) {
        int n = 0;
        for (int r = 0; r < R; ++r) n += th[r] < thr[k];
        nk[k] = n;
      }
      wave_sync();
      // prior = boltzmann.pmf(position, lambda, count) = fact[count] exp(-lambda position); the sum over k is
      // sequential per trough; positions come from a ballot over each chunk of 64 troughs plus the earlier chunks
      for (int base = 0; base < R; base += 64) {
        const int r = base + lane;
        const bool live = r < R;
        const double h = live ? th[r] : 0.0;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
          const bool below = live && h < thr[k];
          const unsigned long long m = __ballot(below);
          if (below) acc = acc + (bfact[nk[k]] * bexp[cp[k] + popc(m & lt)]) * beta[k];
          wave_sync();
          if (lane == 0) cp[k] += popc(m);
          wave_sync();
        }
        if (live) pr[r] = acc;
      }
      // the global minimum takes no_trough_prob * sum(beta[:m]) for the m thresholds it is not below
      double mv = INFINITY;
      int mi = 0x7fffffff;
      for (int r = lane; r < R; r += 64) {
        const double v = th[r];
        if (v < mv) {
          mv = v;
          mi = r;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(mv, o, 64);
        const int i2 = __shfl_xor(mi, o, 64);
        if (v2 < mv || (v2 == mv && i2 < mi)) {
          mv = v2;
          mi = i2;
        }
      }
      int nm = 0;
      for (int k = lane; k < K; k += 64) nm += !(mv < thr[k]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) nm += __shfl_xor(nm, o, 64);
      wave_sync();
      if (lane == 0 && mi < R) pr[mi] = pr[mi] + notrough[nm];
      wave_sync();
      // step 5: candidates (probability != 0) -> pitch bins; clip's upper end n_bins is the first unvoiced state
      for (int r = lane; r < R; r += 64) {
        int bin = -1;
        if (pr[r] != 0.0) {
          const int i = ti[r];
          const double period = (double)(min_p + i) + sh[i];
          const double f0 = sr / period;
          const double v = rint(bins_per_octave * log2(f0 / f_min));
          bin = v < 0.0 ? 0 : (v > (double)n_bins ? n_bins : (int)v);
        }
        tb[r] = bin;
      }
      wave_sync();
      // periods rise with r and bins fall: walking r downwards visits bins upwards, and the first visit of a bin is
      // the larger period, which wins it; the voiced sum in bin order is the sequential sum over the dense row
      if (lane == 0) {
        int prev = -1;
        for (int r = R - 1; r >= 0; --r) {
          const int bin = tb[r];
          if (bin < 0 || bin == prev) continue;
          prev = bin;
          row[bin] = pr[r];
          if (bin < n_bins) vs = vs + pr[r];
        }
      }
    }
    if (lane == 0) vprob[(int64_t)b * T + t] = fmin(fmax(vs, 0.0), 1.0);
  }
  __syncthreads();
  for (int k = tid; k < n_bins; k += NT_OBS) orow[k] = row[k];
}

// One workgroup per item.  value[] of the previous frame and of the current one in LDS (2 x S doubles, S = 2 n).
// State j = a n + q (a = 0 voiced, 1 unvoiced); thread q handles the states q and n + q, whose in-band predecessors
// are the bins q + dd (|dd| <= h) of both halves.  log_band (2, width, n): [0][dd + h][q] = log((1 - s) T[q + dd][q] +
// tiny) (same voicing), [1] the same with the switch probability; every other entry of the dense log-transition is
// log(tiny).  The dense argmax is exact from the band alone plus W* = max_i (value[i] + log(tiny)) and its first index
// A0: an in-band entry is never below log(tiny), so an in-band best above W* wins outright, one below W* loses to A0
// (which then cannot be in band), and only an exact tie needs the full first-index scan.
__global__ __launch_bounds__(NT_VIT) void pyin_viterbi_kernel(
    const double* __restrict__ obs, const double* __restrict__ vprob, const int32_t* __restrict__ frames,
    const double* __restrict__ log_band, const double* __restrict__ log_p_init, const double* __restrict__ freqs,
    const double log_tiny, const double fill_na, const int fill_unvoiced, uint16_t* __restrict__ ptr,
    int32_t* __restrict__ states,
    double* __restrict__ f0, uint8_t* __restrict__ flag, const int T, const int n, const int width) {
  extern __shared__ double sm[];
  __shared__ double red_v[NT_VIT / 64];
  __shared__ int red_i[NT_VIT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = 2 * n, h = width / 2;
  const int Tb = min(frames[b], T);
  double* vbuf[2] = {sm, sm + S};
  const double* ob = obs + (int64_t)b * T * n;
  uint16_t* pb = ptr + (int64_t)b * T * S;
  const double* LD = log_band;
  const double* LO = log_band + (int64_t)width * n;

  for (int t = max(Tb, 0) + tid; t < T; t += NT_VIT) {
    states[(int64_t)b * T + t] = -1;
    f0[(int64_t)b * T + t] = fill_na;
    flag[(int64_t)b * T + t] = 0;
  }
  if (Tb <= 0) return;
  {  // frame 0
    const double u = (1.0 - vprob[(int64_t)b * T]) / (double)n;
    const double lu = u == 0.0 ? log_tiny : log(u + kTiny);
    for (int q = tid; q < n; q += NT_VIT) {
      const double o = ob[q];
      vbuf[0][q] = (o == 0.0 ? log_tiny : log(o + kTiny)) + log_p_init[q];
      vbuf[0][n + q] = lu + log_p_init[n + q];
    }
  }
  __syncthreads();
  for (int t = 1; t < Tb; ++t) {
    const double* cur = vbuf[(t - 1) & 1];
    double* nxt = vbuf[t & 1];
    // W*, A0
    double wv = -INFINITY;
    int wi = 0x7fffffff;
    for (int i = tid; i < S; i += NT_VIT) argmax_merge(wv, wi, cur[i] + log_tiny, i);
    wave_argmax(wv, wi);
    if (lane == 0) {
      red_v[wid] = wv;
      red_i[wid] = wi;
    }
    __syncthreads();
    wv = red_v[0];
    wi = red_i[0];
    for (int w = 1; w < NT_VIT / 64; ++w) argmax_merge(wv, wi, red_v[w], red_i[w]);
    const double u = (1.0 - vprob[(int64_t)b * T + t]) / (double)n;
    const double lu = u == 0.0 ? log_tiny : log(u + kTiny);
    const double* obt = ob + (int64_t)t * n;
    uint16_t* pt = pb + (int64_t)t * S;
    for (int q = tid; q < n; q += NT_VIT) {
      // [0]: state q (voiced), [1]: state n + q (unvoiced); per state the best over predecessors in the voiced half
      // (v*) and in the unvoiced half (u*), each the first maximum in ascending index order
      double vv = -INFINITY, uv = -INFINITY, vu = -INFINITY, uu = -INFINITY;
      int ivv = 0, iuv = 0, ivu = 0, iuu = 0;
      const int d0 = max(-h, -q), d1 = min(h, n - 1 - q);
      for (int dd = d0; dd <= d1; ++dd) {
        const int p = q + dd;
        const double a = cur[p], cu = cur[n + p];
        const double ld = LD[(int64_t)(dd + h) * n + q], lo = LO[(int64_t)(dd + h) * n + q];
        const double s_vv = a + ld, s_uv = cu + lo, s_vu = a + lo, s_uu = cu + ld;
        if (s_vv > vv) { vv = s_vv; ivv = p; }
        if (s_uv > uv) { uv = s_uv; iuv = n + p; }
        if (s_vu > vu) { vu = s_vu; ivu = p; }
        if (s_uu > uu) { uu = s_uu; iuu = n + p; }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int j = a * n + q;
        double bv = a ? vu : vv;
        int bi = a ? ivu : ivv;
        const double b1 = a ? uu : uv;
        if (b1 > bv) {
          bv = b1;
          bi = a ? iuu : iuv;
        }
        if (bv < wv) {
          bv = wv;
          bi = wi;
        } else if (bv == wv) {  // exact tie with the out-of-band maximum: the first index over all predecessors
          for (int i = 0; i < S; ++i) {
            const int pa = i >= n, pq = i - pa * n, dd = pq - q;
            double s = cur[i] + log_tiny;
            if (dd >= -h && dd <= h) s = cur[i] + (pa == a ? LD : LO)[(int64_t)(dd + h) * n + q];
            if (s == wv) {
              bi = i;
              break;
            }
          }
        }
        const double lo_ = a ? lu : (obt[q] == 0.0 ? log_tiny : log(obt[q] + kTiny));
        nxt[j] = lo_ + bv;
        pt[j] = (uint16_t)bi;
      }
    }
    __syncthreads();
  }
  // the last state: first argmax; then the backtrack in one lane
  const double* last = vbuf[(Tb - 1) & 1];
  double lv = -INFINITY;
  int li = 0x7fffffff;
  for (int i = tid; i < S; i += NT_VIT) argmax_merge(lv, li, last[i], i);
  wave_argmax(lv, li);
  if (lane == 0) {
    red_v[wid] = lv;
    red_i[wid] = li;
  }
  __syncthreads();
  if (tid == 0) {
    lv = red_v[0];
    li = red_i[0];
    for (int w = 1; w < NT_VIT / 64; ++w) argmax_merge(lv, li, red_v[w], red_i[w]);
    int s = li;
    for (int t = Tb - 1; t >= 0; --t) {
      const int64_t o = (int64_t)b * T + t;
      states[o] = s;
      const bool v = s < n;
      flag[o] = v;
      f0[o] = (v || !fill_unvoiced) ? freqs[s] : fill_na;
      if (t > 0) s = pb[(int64_t)t * S + s];
    }
  }
}

size_t observe_smem(int W, int max_p, int min_p, int K, int n_bins) {
  const size_t L = (size_t)W + max_p + 1, nf = (size_t)max_p - min_p + 1;
  return (2 * L + (max_p + 1) + 4 * nf + n_bins + 1) * sizeof(double) + (2 * nf + 2 * (size_t)K) * sizeof(int);
}

constexpr int kObserveSmemMax = 112 * 1024;
constexpr int kViterbiSmemMax = 2 * SRN_PYIN_MAX_STATES * (int)sizeof(double);

}  // namespace

extern "C" int srn_pyin_observe(const float* x, int64_t x_bs, const int32_t* lens, const int32_t* frames,
                                const double* thresholds, const double* beta_probs, const double* boltz_fact,
                                const double* boltz_exp, const double* no_trough, double* obs, double* voiced_prob,
                                int B, int N, int T, int frame_length, int win_length, int hop_length, int pad,
                                int min_period, int max_period, int n_thresholds, double sr, double fmin,
                                double bins_per_octave, int n_bins, void* stream) {
  SRN_CHECK_ARG(x && lens && frames && thresholds && beta_probs && boltz_fact && boltz_exp && no_trough && obs &&
                    voiced_prob,
                "pyin_observe: null pointer");
  SRN_CHECK_ARG(B > 0 && N > 0 && T > 0 && x_bs >= N && hop_length > 0 && pad >= 0,
                "pyin_observe: bad sizes (B %d, N %d, T %d, x_bs %lld, hop %d, pad %d)", B, N, T, (long long)x_bs,
                hop_length, pad);
  SRN_CHECK_ARG(frame_length > 0 && frame_length <= SRN_PYIN_MAX_FRAME && win_length > 0 &&
                    win_length < frame_length && min_period >= 1 && max_period <= frame_length - win_length - 1 &&
                    max_period - min_period + 1 >= 3 && max_period - min_period + 1 <= SRN_PYIN_MAX_PERIODS,
                "pyin_observe: bad frame (frame %d, win %d, periods %d..%d)", frame_length, win_length, min_period,
                max_period);
  SRN_CHECK_ARG(n_thresholds > 0 && n_thresholds <= SRN_PYIN_MAX_THRESHOLDS && n_bins > 0 &&
                    2 * n_bins <= SRN_PYIN_MAX_STATES && sr > 0.0 && fmin > 0.0 && bins_per_octave > 0.0,
                "pyin_observe: bad parameters (thresholds %d, n_bins %d)", n_thresholds, n_bins);
  const size_t smem = observe_smem(win_length, max_period, min_period, n_thresholds, n_bins);
  SRN_CHECK_ARG(smem <= (size_t)kObserveSmemMax, "pyin_observe: %zu bytes of LDS > %d", smem, kObserveSmemMax);
  static SrnSmemAttr attr;
  if (attr.ensure((const void*)pyin_observe_kernel, kObserveSmemMax)) return -2;
  hipLaunchKernelGGL(pyin_observe_kernel, dim3(T, B), dim3(NT_OBS), smem, (hipStream_t)stream, x, x_bs, lens, frames,
                     thresholds, beta_probs, boltz_fact, boltz_exp, no_trough, obs, voiced_prob, T, win_length,
                     hop_length, pad, min_period, max_period, n_thresholds, sr, fmin, bins_per_octave, n_bins);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_pyin_viterbi(const double* obs, const double* voiced_prob, const int32_t* frames,
                                const double* log_band, const double* log_p_init, const double* freqs,
                                double log_tiny, double fill_na, int fill_unvoiced, uint16_t* ptr_ws,
                                int32_t* states, double* f0, uint8_t* voiced_flag, int B, int T, int n_bins, int width,
                                void* stream) {
  SRN_CHECK_ARG(obs && voiced_prob && frames && log_band && log_p_init && freqs && ptr_ws && states && f0 &&
                    voiced_flag,
                "pyin_viterbi: null pointer");
  SRN_CHECK_ARG(B > 0 && T > 0 && n_bins > 0 && 2 * n_bins <= SRN_PYIN_MAX_STATES && width >= 1 && width % 2 == 1,
                "pyin_viterbi: bad sizes (B %d, T %d, n_bins %d, width %d)", B, T, n_bins, width);
  static SrnSmemAttr attr;
  if (attr.ensure((const void*)pyin_viterbi_kernel, kViterbiSmemMax)) return -2;
  hipLaunchKernelGGL(pyin_viterbi_kernel, dim3(B), dim3(NT_VIT), (size_t)2 * 2 * n_bins * sizeof(double),
                     (hipStream_t)stream, obs, voiced_prob, frames, log_band, log_p_init, freqs, log_tiny, fill_na,
                     fill_unvoiced, ptr_ws, states, f0, voiced_flag, T, n_bins, width);
  SRN_CHECK_LAUNCH();
  return 0;
}
