// harvest.hip -- WORLD Harvest F0 estimation (Morise 2017, harvest.cpp) as pyworld.harvest runs it in preprocessing
// (serenade/bin/preprocess.py:485-493): the f0 track of every dump.  serenade_amd/harvest.py drives it;
// tests/_harvest_ref.py is the float64 restatement it is held to, stage by stage.
//   srn_harvest_decimate    GetWaveformAndSpectrum + decimate: edge extension, zero-phase Chebyshev, pick, mean removal
//   srn_harvest_channels    GetRawF0Candidates: per (item, channel) band-pass, four kinds of events, interp1, average
//   srn_harvest_candidates  DetectOfficialF0Candidates + OverlapF0Candidates
//   srn_harvest_refine      RefineF0Candidates: instantaneous frequency at <= 6 harmonics by a direct DFT
//   srn_harvest_contour     RemoveUnreliableCandidates, FixF0Contour steps 1-4, SmoothF0Contour, the frame-period pick
//
// Numerics: fp64 throughout, contraction off, every expression in the restatement's order of operations.  The only
// sums whose order differs from the restatement's are the band-pass (ascending taps here), the DFT sums of the
// refinement and the signal's mean (lane partials + a shuffle tree here); everything after the refinement is the
// restatement's arithmetic bit for bit.  Every data-independent table comes from the host.
#include <hip/hip_runtime.h>

#include "common.h"
#include "serenade_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr int DEC_TILE = 1024;
constexpr int DEC_NFACT = 9;  // reflected samples of MATLAB-style decimate
constexpr int NT_CH = 256;    // threads = samples per tile of the channel kernel
constexpr int NT = 256;
constexpr int MIN_INTERVALS = 2;  // a kind of event needs more than this many intervals
constexpr int MIN_RUN = 10;
constexpr int OVERLAP = 3;
constexpr int MAX_HARMONICS = 6;
constexpr double SCORE_THRESHOLD = 2.5;
constexpr double SAFEGUARD = 1e-12;
constexpr double REMOVE_RANGE = 0.05;
constexpr double STEP1_RANGE = 0.1;
constexpr double STEP3_RANGE = 0.18;
constexpr int EXTEND_FRAMES = 100;
constexpr int EXTEND_MISSES = 4;
constexpr double EXTEND_MEAN_RULE = 2200.0;
constexpr int STEP4_GAP = 9;
constexpr int SMOOTH_PAD = SRN_HARVEST_SMOOTH_PAD;
constexpr int EXT_SLACK = EXTEND_FRAMES + 1;  // frames an extension can reach past a section's end

__device__ __forceinline__ int64_t matlab_round(double x) { return x > 0.0 ? (int64_t)(x + 0.5) : (int64_t)(x - 0.5); }

// ------------------------------------------------------------------------------------------------ decimation
// One wave per item.  The recurrence runs in lane 0 over LDS tiles that the whole wave loads and stores.
template <typename T>
__global__ __launch_bounds__(64) void harvest_decimate_kernel(const T* __restrict__ x, const int64_t x_bs,
                                                              const int32_t* __restrict__ lens,
                                                              const double* __restrict__ coef, double* __restrict__ ws,
                                                              const int64_t ws_stride, double* __restrict__ y,
                                                              const int64_t y_bs, const int ratio, const int lag) {
  __shared__ double s_in[DEC_TILE];
  __shared__ double s_out[DEC_TILE];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = lens[b];
  const T* xb = x + (int64_t)b * x_bs;
  double* yb = y + (int64_t)b * y_bs;
  const int ylen = (n + ratio - 1) / ratio;
  if (n <= 0) return;
  if (ratio == 1) {
    for (int i = lane; i < n; i += 64) yb[i] = (double)xb[i];
  } else {
    double* wb = ws + (int64_t)b * ws_stride;
    const int L = n + 2 * lag, M = L + 2 * DEC_NFACT;
    const int nout = (L - 1) / ratio + 1;
    const int nbeg = ratio - ratio * nout + L;          // 1-based, as MATLAB's decimate
    const int first = DEC_NFACT + nbeg - 1 + lag;       // where y[0] sits in the reflected, extended signal
    const double b0 = coef[0], b1 = coef[1], b2 = coef[2], b3 = coef[3], a1 = coef[5], a2 = coef[6], a3 = coef[7];
    auto nx = [&](int q) -> double {  // the signal extended by lag copies of each edge sample
      int s = q - lag;
      s = s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
      return (double)xb[s];
    };
    auto ext = [&](int p) -> double {  // ... and reflected through its ends over DEC_NFACT samples
      const int q = p - DEC_NFACT;
      if (q < 0) return 2 * nx(0) - nx(-q);
      if (q >= L) return 2 * nx(L - 1) - nx(L - 2 - (q - L));
      return nx(q);
    };
    for (int pass = 0; pass < 2; ++pass) {
      double w0 = 0.0, w1 = 0.0, w2 = 0.0;
      for (int t0 = 0; t0 < M; t0 += DEC_TILE) {
        const int cnt = min(DEC_TILE, M - t0);
        for (int k = lane; k < cnt; k += 64) s_in[k] = pass == 0 ? ext(t0 + k) : wb[M - 1 - (t0 + k)];
        wave_sync();
        if (lane == 0) {
#pragma unroll 8
          for (int k = 0; k < cnt; ++k) {
            const double v = s_in[k];
            const double wt = ((v - a1 * w0) - a2 * w1) - a3 * w2;
            s_out[k] = ((b0 * wt + b1 * w0) + b2 * w1) + b3 * w2;
            w2 = w1;
            w1 = w0;
            w0 = wt;
          }
        }
        wave_sync();
        for (int k = lane; k < cnt; k += 64) {
          if (pass == 0) {
            wb[t0 + k] = s_out[k];
          } else {  // step s of the reversed pass is sample M - 1 - s
            const int r = M - 1 - (t0 + k) - first;
            if (r >= 0 && r % ratio == 0 && r / ratio < ylen) yb[r / ratio] = s_out[k];
          }
        }
        wave_sync();
      }
      __threadfence();
      wave_sync();
    }
  }
  __threadfence();
  wave_sync();
  double s = 0.0;
  for (int i = lane; i < ylen; i += 64) s += yb[i];
  const double mean = wave_sum_d(s) / (double)ylen;
  for (int i = lane; i < ylen; i += 64) yb[i] = yb[i] - mean;
}

// ------------------------------------------------------------------------------------------------ raw candidates
// interp1 of one kind of event at time t: points loc(j) = (e[j] + e[j + 1]) / 2 / fs, f(j) = fs / (e[j + 1] - e[j]),
// j < n_int; linear, extrapolating from the first and the last segment (WORLD's histc + interp1)
__device__ __forceinline__ double interp_events(const double* __restrict__ e, const int n_int, const double fs,
                                                const double t) {
  int lo = 0, hi = n_int;  // first j with loc(j) > t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((e[mid] + e[mid + 1]) / 2.0 / fs > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  int k = lo - 1;
  k = k < 0 ? 0 : (k > n_int - 2 ? n_int - 2 : k);
  const double x0 = (e[k] + e[k + 1]) / 2.0 / fs, x1 = (e[k + 1] + e[k + 2]) / 2.0 / fs;
  const double y0 = fs / (e[k + 1] - e[k]), y1 = fs / (e[k + 2] - e[k + 1]);
  const double s = (t - x0) / (x1 - x0);
  return y0 + s * (y1 - y0);
}

// One workgroup per (channel, item).  The signal is walked in tiles of NT_CH samples: band-pass into LDS, the four
// kinds of events found per sample and compacted in order (ballot within a wave, wave counts within the tile, a running
// count across tiles).  A kind has at most len / 2 events (an edge needs two samples): ev_cap >= that.
__global__ __launch_bounds__(NT_CH) void harvest_channels_kernel(
    const double* __restrict__ y, const int64_t y_bs, const int32_t* __restrict__ ylens,
    const int32_t* __restrict__ frames, const double* __restrict__ taps, const int32_t* __restrict__ tap_off,
    const int32_t* __restrict__ half_len, const double* __restrict__ boundary, double* __restrict__ events,
    const int64_t ev_cap, double* __restrict__ raw, const int ch0, const int n_ch, const int F1, const double fs,
    const double f0_floor, const double f0_ceil) {
  __shared__ double s_h[SRN_HARVEST_MAX_TAPS];
  __shared__ double s_y[NT_CH + 2 + SRN_HARVEST_MAX_TAPS];
  __shared__ double s_f[NT_CH + 2];
  __shared__ int s_cnt[4][NT_CH / 64];
  const int ch = ch0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int len = ylens[b], nf = min(frames[b], F1), hl = half_len[ch], nt = 2 * hl + 1;
  const double* yb = y + (int64_t)b * y_bs;
  double* ev = events + ((int64_t)b * gridDim.x + blockIdx.x) * 4 * ev_cap;
  double* out = raw + ((int64_t)b * n_ch + ch) * F1;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int k = tid; k < nt; k += NT_CH) s_h[k] = taps[tap_off[ch] + k];
  int total[4] = {0, 0, 0, 0};
  for (int t0 = 0; t0 < len; t0 += NT_CH) {
    __syncthreads();
    // filtered[i] = sum_t h[t] y[i + 1 + hl - t], zeros outside the signal; s_y[k] = y[t0 + 1 - hl + k]
    for (int k = tid; k < NT_CH + 2 + 2 * hl; k += NT_CH) {
      const int s = t0 + 1 - hl + k;
      s_y[k] = (s >= 0 && s < len) ? yb[s] : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < NT_CH + 2; idx += NT_CH) {
      double acc = 0.0;
      if (t0 + idx < len) {
        const double* yy = s_y + idx + 2 * hl;
        for (int t = 0; t < nt; ++t) acc = acc + s_h[t] * yy[-t];
      }
      s_f[idx] = acc;
    }
    __syncthreads();
    const int i = t0 + tid;
    const double f0 = s_f[tid], f1 = s_f[tid + 1], f2 = s_f[tid + 2];
    const double g0 = -f0, g1 = -f1, g2 = -f2;
    const double d0 = g0 - g1, d1 = g1 - g2;
    const double n0 = -d0, n1 = -d1;
    const bool in1 = i + 1 < len, in2 = i + 2 < len;
    bool hit[4];
    double pos[4];
    hit[0] = in1 && f0 > 0.0 && f1 <= 0.0;
    hit[1] = in1 && g0 > 0.0 && g1 <= 0.0;
    hit[2] = in2 && d0 > 0.0 && d1 <= 0.0;
    hit[3] = in2 && n0 > 0.0 && n1 <= 0.0;
    pos[0] = (double)(i + 1) - f0 / (f1 - f0);
    pos[1] = (double)(i + 1) - g0 / (g1 - g0);
    pos[2] = (double)(i + 1) - d0 / (d1 - d0);
    pos[3] = (double)(i + 1) - n0 / (n1 - n0);
    unsigned long long m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m[k] = __ballot(hit[k]);
      if (lane == 0) s_cnt[k][wid] = __popcll(m[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < NT_CH / 64; ++w) {
        const int c = s_cnt[k][w];
        before += w < wid ? c : 0;
        all += c;
      }
      const int64_t slot = (int64_t)total[k] + before + __popcll(m[k] & lt);
      if (hit[k] && slot < ev_cap) ev[(int64_t)k * ev_cap + slot] = pos[k];
      total[k] += all;
    }
  }
  __threadfence();
  __syncthreads();
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    total[k] = (int)min((int64_t)total[k], ev_cap);
    ok = ok && (total[k] - 1 > MIN_INTERVALS);
  }
  const double upper = boundary[ch] * 1.1, lower = boundary[ch] * 0.9;
  for (int fr = tid; fr < F1; fr += NT_CH) {
    double c = 0.0;
    if (ok && fr < nf) {
      const double t = (double)fr / 1000.0;
      const double v0 = interp_events(ev, total[0] - 1, fs, t);
      const double v1 = interp_events(ev + ev_cap, total[1] - 1, fs, t);
      const double v2 = interp_events(ev + 2 * ev_cap, total[2] - 1, fs, t);
      const double v3 = interp_events(ev + 3 * ev_cap, total[3] - 1, fs, t);
      c = (((v0 + v1) + v2) + v3) / 4.0;
      if (c > upper || c < lower || c > f0_ceil || c < f0_floor) c = 0.0;
      if (!(c == c)) c = 0.0;  // the restatement's comparisons are all false on a NaN too, but a NaN never arises
    }
    out[fr] = c;
  }
}

// ------------------------------------------------------------------------------------------------ official + overlap
__global__ __launch_bounds__(NT) void harvest_official_kernel(const double* __restrict__ raw,
                                                              const int32_t* __restrict__ frames,
                                                              double* __restrict__ official, const int n_ch,
                                                              const int F1, const int n_base) {
  const int fr = blockIdx.x * NT + threadIdx.x, b = blockIdx.y;
  if (fr >= F1) return;
  double* out = official + ((int64_t)b * F1 + fr) * n_base;
  int count = 0;
  if (fr < min(frames[b], F1)) {
    const double* r = raw + (int64_t)b * n_ch * F1 + fr;
    int run = 0;
    double acc = 0.0;
    for (int j = 1; j < n_ch; ++j) {
      const double v = j < n_ch - 1 ? r[(int64_t)j * F1] : 0.0;
      if (v > 0.0) {
        acc = (run > 0 ? acc : 0.0) + v;
        ++run;
      } else {
        if (run >= MIN_RUN && count < n_base) out[count++] = acc / (double)run;
        run = 0;
        acc = 0.0;
      }
    }
  }
  for (int c = count; c < n_base; ++c) out[c] = 0.0;
}

__global__ __launch_bounds__(NT) void harvest_overlap_kernel(const double* __restrict__ official,
                                                             const int32_t* __restrict__ frames,
                                                             double* __restrict__ cand, const int F1,
                                                             const int n_base) {
  const int C = n_base * (2 * OVERLAP + 1);
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int b = blockIdx.y;
  if (g >= (int64_t)F1 * C) return;
  const int fr = (int)(g / C), slot = (int)(g % C), i = slot / n_base, j = slot % n_base;
  const int nf = min(frames[b], F1);
  const int src = i == 0 ? fr : (i <= OVERLAP ? fr - i : fr + (i - OVERLAP));
  double v = 0.0;
  if (fr < nf && src >= 0 && src < nf) v = official[((int64_t)b * F1 + src) * n_base + j];
  cand[(int64_t)b * F1 * C + g] = v;
}

// ------------------------------------------------------------------------------------------------ refinement
// One wave per (item, frame), looping over the frame's candidates (most are zero).  The main window of a candidate is
// staged in LDS; the derivative window and the two windowed signals are formed from it on the fly per harmonic.
__global__ __launch_bounds__(NT) void harvest_refine_kernel(const double* __restrict__ y, const int64_t y_bs,
                                                            const int32_t* __restrict__ ylens,
                                                            const int32_t* __restrict__ frames,
                                                            const double* __restrict__ cand,
                                                            double* __restrict__ refined, double* __restrict__ score,
                                                            const int F1, const int C, const double fs,
                                                            const double f0_floor, const double f0_ceil) {
  __shared__ double s_w[NT / 64][SRN_HARVEST_MAX_WINDOW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fr = blockIdx.x * (NT / 64) + wid, b = blockIdx.y;
  if (fr >= F1) return;
  const int64_t row = ((int64_t)b * F1 + fr) * C;
  const int len = ylens[b];
  const bool live_frame = fr < min(frames[b], F1) && len > 0;
  const double* yb = y + (int64_t)b * y_bs;
  double* mw = s_w[wid];
  const double pos = (double)fr / 1000.0;
  for (int c = 0; c < C; ++c) {
    const double f0 = live_frame ? cand[row + c] : 0.0;
    double r_out = 0.0, s_out = 0.0;
    const int hw = f0 > 0.0 ? (int)(1.5 * fs / f0 + 1.0) : 0;
    const int W = 2 * hw + 1;
    if (f0 > 0.0 && W <= SRN_HARVEST_MAX_WINDOW) {
      const double wlen = (2.0 * hw + 1.0) / fs;
      const int64_t base = matlab_round((pos + (double)(-hw) / fs) * fs + 0.001);
      const int N = 1 << (2 + 31 - __clz(W));
      wave_sync();
      for (int i = lane; i < W; i += 64) {
        const double tmp = ((double)(base + i) - 1.0) / fs - pos;
        mw[i] = 0.42 + 0.5 * cos(2.0 * kPi * tmp / wlen) + 0.08 * cos(4.0 * kPi * tmp / wlen);
      }
      wave_sync();
      const int n_harm = min((int)(fs / 2.0 / f0), MAX_HARMONICS);
      double num = 0.0, den = 0.0, sc = 0.0;
      for (int k = 1; k <= n_harm; ++k) {
        const int bin = (int)matlab_round(f0 * (double)N / fs * (double)k);
        double mc = 0.0, ms = 0.0, dc = 0.0, ds = 0.0;
        for (int i = lane; i < W; i += 64) {
          int64_t si = base + i - 1;
          si = si < 0 ? 0 : (si > len - 1 ? len - 1 : si);
          const double x = yb[si];
          const double dwin = i == 0 ? -mw[1] / 2.0 : (i == W - 1 ? mw[W - 2] / 2.0 : -(mw[i + 1] - mw[i - 1]) / 2.0);
          const double xm = x * mw[i], xd = x * dwin;
          const int ph = (int)(((int64_t)bin * i) % N);
          const double ang = 2.0 * kPi * (double)ph / (double)N;
          const double cs = cos(ang), sn = sin(ang);
          mc = mc + xm * cs;
          ms = ms + xm * sn;
          dc = dc + xd * cs;
          ds = ds + xd * sn;
        }
        const double m_re = wave_sum_d(mc), m_im = -wave_sum_d(ms);
        const double d_re = wave_sum_d(dc), d_im = -wave_sum_d(ds);
        const double numer = m_re * d_im - m_im * d_re;
        const double power = m_re * m_re + m_im * m_im;
        const double inst = power == 0.0 ? 0.0 : (double)bin * fs / (double)N + numer / power * fs / 2.0 / kPi;
        const double amp = sqrt(power);
        num = num + amp * inst;
        den = den + amp * (double)k;
        sc = sc + fabs((inst / (double)k - f0) / f0);
      }
      const double r = num / (den + SAFEGUARD);
      const double s = 1.0 / (sc / (double)n_harm + SAFEGUARD);
      if (!(r < f0_floor || r > f0_ceil || s < SCORE_THRESHOLD) && r == r && s == s) {
        r_out = r;
        s_out = s;
      }
    }
    if (lane == 0) {
      refined[row + c] = r_out;
      score[row + c] = s_out;
    }
  }
}

// ------------------------------------------------------------------------------------------------ contour
// RemoveUnreliableCandidates: one thread per (frame, candidate); neighbours are read from the state before the step
__global__ __launch_bounds__(NT) void harvest_remove_kernel(const double* __restrict__ cand,
                                                            const double* __restrict__ score,
                                                            const int32_t* __restrict__ frames,
                                                            double* __restrict__ cand2, double* __restrict__ score2,
                                                            const int F1, const int C) {
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int b = blockIdx.y;
  if (g >= (int64_t)F1 * C) return;
  const int fr = (int)(g / C);
  const int nf = min(frames[b], F1);
  const int64_t o = (int64_t)b * F1 * C + g;
  double ref = fr < nf ? cand[o] : 0.0, sc = fr < nf ? score[o] : 0.0;
  if (ref != 0.0 && fr >= 1 && fr < nf - 1) {
    const double* nxt = cand + ((int64_t)b * F1 + fr + 1) * C;
    const double* prv = cand + ((int64_t)b * F1 + fr - 1) * C;
    double err = 1.0;
    for (int k = 0; k < C; ++k) {
      const double t1 = fabs(ref - nxt[k]) / ref, t2 = fabs(ref - prv[k]) / ref;
      if (t1 <= err) err = t1;
      if (t2 <= err) err = t2;
    }
    if (!(err <= REMOVE_RANGE)) {
      ref = 0.0;
      sc = 0.0;
    }
  }
  cand2[o] = ref;
  score2[o] = sc;
}

// SelectBestF0 by a whole wave: the candidate nearest to ref within allowed (relative to ref), the last one of equals;
// 0 when there is none.  Every lane returns the same value.
__device__ __forceinline__ double wave_select_best(const double ref, const double* __restrict__ row, const int C,
                                                   const double allowed, const int lane) {
  double best = INFINITY, val = 0.0;
  int bi = -1;
  for (int j = lane; j < C; j += 64) {
    const double c = row[j];
    const double tmp = fabs(ref - c) / ref;
    if (tmp <= allowed && tmp <= best) {
      best = tmp;
      bi = j;
      val = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double b2 = __shfl_xor(best, o, 64), v2 = __shfl_xor(val, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (i2 >= 0 && (bi < 0 || b2 < best || (b2 == best && i2 > bi))) {
      best = b2;
      bi = i2;
      val = v2;
    }
  }
  return bi < 0 ? 0.0 : val;
}

// SearchScore: the best score among the candidates equal to f0
__device__ __forceinline__ double search_score(const double f0, const double* __restrict__ c,
                                               const double* __restrict__ s, const int C) {
  double best = 0.0;
  for (int j = 0; j < C; ++j)
    if (f0 == c[j] && best < s[j]) best = s[j];
  return best;
}

// voiced sections [st, ed] of f (GetBoundaryList: the first and the last frame count as unvoiced when ends_open is 0);
// returns the number found, at most cap are stored and more set *status
__device__ int list_sections(const double* __restrict__ f, const int nf, const bool force_ends, int32_t* st_out,
                             int32_t* ed_out, const int cap, const int min_len, double* zero_short) {
  int n = 0, st = -1;
  for (int i = 0; i <= nf; ++i) {
    bool v = i < nf && f[i] > 0.0;
    if (force_ends && (i == 0 || i == nf - 1)) v = false;
    if (v && st < 0) st = i;
    if (!v && st >= 0) {
      const int ed = i - 1;
      if (ed - st < min_len) {
        if (zero_short)
          for (int j = st; j <= ed; ++j) zero_short[j] = 0.0;
      } else {
        if (n < cap) {
          st_out[n] = st;
          ed_out[n] = ed;
        }
        ++n;
      }
      st = -1;
    }
  }
  return n;
}

__device__ __forceinline__ void df2_2(const double v, const double* cf, double& w0, double& w1, double& out) {
  const double wt = (v - cf[4] * w0) - cf[5] * w1;
  out = (cf[0] * wt + cf[1] * w0) + cf[2] * w1;
  w1 = w0;
  w0 = wt;
}

// One workgroup per item.  fbuf (6, F1): base, step1/2, step3, step4, smoothed, spare.  sec (7, cap) int32: st, ed,
// extended st, extended ed, pool offset, keep, order.  pool: the sections' extended contours, later the smoothing's
// scratch.
__global__ __launch_bounds__(NT) void harvest_contour_kernel(
    const double* __restrict__ cand2, const double* __restrict__ score2, const int32_t* __restrict__ frames,
    const int32_t* __restrict__ out_frames, const double* __restrict__ smooth_coef, double* __restrict__ fbuf,
    double* __restrict__ pool_all, const int64_t pool_stride, int32_t* __restrict__ sec_all, const int cap,
    int32_t* __restrict__ status, double* __restrict__ f0_out, const int64_t out_stride, const int F1, const int C,
    const int F_out, const int vrm, const double frame_period) {
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nf = min(frames[b], F1);
  const double* cd = cand2 + (int64_t)b * F1 * C;
  const double* sd = score2 + (int64_t)b * F1 * C;
  double* base = fbuf + (int64_t)b * 6 * F1;
  double* f2 = base + F1;
  double* f3 = f2 + F1;
  double* f4 = f3 + F1;
  double* sm = f4 + F1;
  double* pool = pool_all + (int64_t)b * pool_stride;
  int32_t* s_st = sec_all + (int64_t)b * 7 * cap;
  int32_t* s_ed = s_st + cap;
  int32_t* s_st2 = s_ed + cap;
  int32_t* s_ed2 = s_st2 + cap;
  int32_t* s_off = s_ed2 + cap;
  int32_t* s_keep = s_off + cap;
  int32_t* s_ord = s_keep + cap;
  double* out = f0_out + (int64_t)b * out_stride;
  if (tid == 0) status[b] = 0;
  if (nf < 1) {
    for (int i = tid; i < F_out; i += NT) out[i] = 0.0;
    return;
  }
  // SearchF0Base: the best-scoring candidate of each frame (the first of equals)
  for (int i = tid; i < nf; i += NT) {
    double best = 0.0, val = 0.0;
    for (int j = 0; j < C; ++j) {
      const double s = sd[(int64_t)i * C + j];
      if (s > best) {
        best = s;
        val = cd[(int64_t)i * C + j];
      }
    }
    base[i] = val;
  }
  __threadfence();
  __syncthreads();
  // FixStep1
  for (int i = tid; i < nf; i += NT) {
    double v = 0.0;
    if (i >= 2 && base[i] != 0.0) {
      const double ref = base[i - 1] * 2 - base[i - 2];
      const double e1 = fabs((base[i] - ref) / ref), e2 = fabs(base[i] - base[i - 1]) / base[i - 1];
      v = (e1 > STEP1_RANGE && e2 > STEP1_RANGE) ? 0.0 : base[i];
    }
    f2[i] = v;
    sm[i] = 0.0;
  }
  __threadfence();
  __syncthreads();
  // FixStep2 + the section list of FixStep3, with the pool offsets of the sections' extended contours
  if (tid == 0) {
    int n = list_sections(f2, nf, true, s_st, s_ed, cap, vrm, f2);
    if (n > cap) {
      status[b] = 1;
      n = cap;
    }
    int64_t off = 0;
    for (int s = 0; s < n; ++s) {
      const int lo = max(0, s_st[s] - EXT_SLACK), hi = min(nf - 1, s_ed[s] + EXT_SLACK);
      if (off + (hi - lo + 1) > pool_stride) {
        status[b] = 1;
        n = s;
        break;
      }
      s_off[s] = (int32_t)off;
      off += hi - lo + 1;
    }
    s_n = n;
  }
  __threadfence();
  __syncthreads();
  const int n_sec = s_n;
  // FixStep3, Extend: one wave per section
  for (int s = wid; s < n_sec; s += NT / 64) {
    const int st = s_st[s], ed = s_ed[s];
    const int lo = max(0, st - EXT_SLACK), hi = min(nf - 1, ed + EXT_SLACK);
    double* ext = pool + s_off[s] - lo;  // ext[p] for lo <= p <= hi
    for (int p = lo + lane; p <= hi; p += 64) ext[p] = (p >= st && p <= ed) ? f2[p] : 0.0;
    wave_sync();
    int ends[2];
    for (int dir = 0; dir < 2; ++dir) {
      const int shift = dir == 0 ? 1 : -1;
      const int origin = dir == 0 ? ed : st;
      const int last = dir == 0 ? min(nf - 2, ed + EXTEND_FRAMES) : max(1, st - EXTEND_FRAMES);
      const int distance = abs(last - origin);
      double tmp_f0 = f2[origin];
      int shifted = origin, count = 0;
      for (int i = 0; i <= distance; ++i) {
        const int p = origin + shift * i + shift;
        if (p < lo || p > hi) break;
        const double v = wave_select_best(tmp_f0, cd + (int64_t)p * C, C, STEP3_RANGE, lane);
        if (lane == 0) ext[p] = v;
        if (v == 0.0) {
          ++count;
        } else {
          tmp_f0 = v;
          count = 0;
          shifted = p;
        }
        if (count == EXTEND_MISSES) break;
      }
      ends[dir] = shifted;
    }
    if (lane == 0) {
      s_ed2[s] = ends[0];
      s_st2[s] = ends[1];
    }
  }
  __threadfence();
  __syncthreads();
  // ExtendSub, MergeF0, FixStep4 and the smoothing's section list: one lane
  if (tid == 0) {
    int kept = 0;
    double mean_f0 = 0.0;  // carried from section to section, as the restatement (and harvest.cpp) has it
    for (int s = 0; s < n_sec; ++s) {
      const int st = s_st2[s], ed = s_ed2[s];
      const double* ext = pool + s_off[s] - max(0, s_st[s] - EXT_SLACK);
      for (int j = st; j < ed; ++j) mean_f0 += ext[j];
      mean_f0 /= (double)(ed - st);
      s_keep[s] = EXTEND_MEAN_RULE / mean_f0 < (double)(ed - st);
      if (s_keep[s]) {  // stable insertion by the extended start
        int k = kept++;
        while (k > 0 && s_st2[s_ord[k - 1]] > st) {
          s_ord[k] = s_ord[k - 1];
          --k;
        }
        s_ord[k] = s;
      }
    }
    if (kept == 0) {
      for (int i = 0; i < nf; ++i) f3[i] = f2[i];
    } else {
      for (int i = 0; i < nf; ++i) f3[i] = 0.0;
      int st1 = 0, ed1 = 0;
      for (int q = 0; q < kept; ++q) {
        const int s = s_ord[q];
        const int lo = max(0, s_st[s] - EXT_SLACK), hi = min(nf - 1, s_ed[s] + EXT_SLACK);
        const double* ext = pool + s_off[s] - lo;
        const int st2 = s_st2[s], ed2 = s_ed2[s];
        if (q == 0) {
          for (int i = lo; i <= hi; ++i) f3[i] = ext[i];
          st1 = st2;
          ed1 = ed2;
        } else if (st2 - ed1 > 0) {
          for (int i = st2; i <= ed2; ++i) f3[i] = ext[i];
          ed1 = ed2;
        } else if (st1 <= st2 && ed1 >= ed2) {
        } else {
          double sc1 = 0.0, sc2 = 0.0;
          for (int i = st2; i <= ed1; ++i) {
            sc1 += search_score(f3[i], cd + (int64_t)i * C, sd + (int64_t)i * C, C);
            sc2 += search_score(ext[i], cd + (int64_t)i * C, sd + (int64_t)i * C, C);
          }
          for (int i = sc1 > sc2 ? ed1 : st2; i <= ed2; ++i) f3[i] = ext[i];
          ed1 = ed2;
        }
      }
    }
    // FixStep4: unvoiced gaps shorter than STEP4_GAP are bridged linearly
    for (int i = 0; i < nf; ++i) f4[i] = f3[i];
    {
      int prev_ed = -1, st = -1;
      for (int i = 0; i <= nf; ++i) {
        const bool v = i < nf && i != 0 && i != nf - 1 && f3[i] > 0.0;
        if (v && st < 0) {
          st = i;
          if (prev_ed >= 0) {
            const int distance = st - prev_ed - 1;
            if (distance < STEP4_GAP) {
              const double tmp0 = f3[prev_ed] + 1, tmp1 = f3[st] - 1;
              const double coef = (tmp1 - tmp0) / (distance + 1.0);
              int count = 1;
              for (int j = prev_ed + 1; j < st; ++j) f4[j] = tmp0 + coef * (double)count++;
            }
          }
        }
        if (!v && st >= 0) {
          prev_ed = i - 1;
          st = -1;
        }
      }
    }
    int n = list_sections(f4, nf, false, s_st, s_ed, cap, 0, nullptr);
    if (n > cap) {
      status[b] = 1;
      n = cap;
    }
    int64_t off = 0;
    for (int s = 0; s < n; ++s) {
      const int64_t need = s_ed[s] - s_st[s] + 1 + 2 * SMOOTH_PAD;
      if (off + need > pool_stride) {
        status[b] = 1;
        n = s;
        break;
      }
      s_off[s] = (int32_t)off;
      off += need;
    }
    s_n = n;
  }
  __threadfence();
  __syncthreads();
  // SmoothF0Contour: one lane per voiced section, forward then backward over the section padded with its edge values
  {
    double cf[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cf[k] = smooth_coef[k];
    for (int s = tid; s < s_n; s += NT) {
      const int st = s_st[s], ed = s_ed[s], n = ed - st + 1, M = n + 2 * SMOOTH_PAD;
      double* tmp = pool + s_off[s];
      const double first = f4[st], lastv = f4[ed];
      double w0 = 0.0, w1 = 0.0, o;
      for (int i = 0; i < M; ++i) {
        const double v = i < SMOOTH_PAD ? first : (i < SMOOTH_PAD + n ? f4[st + i - SMOOTH_PAD] : lastv);
        df2_2(v, cf, w0, w1, o);
        tmp[i] = o;
      }
      w0 = w1 = 0.0;
      for (int i = 0; i < M; ++i) {
        df2_2(tmp[M - 1 - i], cf, w0, w1, o);
        const int p = M - 1 - i - SMOOTH_PAD;  // position in the section
        if (p >= 0 && p < n) sm[st + p] = o;
      }
    }
  }
  __threadfence();
  __syncthreads();
  // the requested frame period: a pick from the 1 ms contour
  const int n_out = min(out_frames[b], F_out);
  for (int i = tid; i < F_out; i += NT) {
    double v = 0.0;
    if (i < n_out) {
      const double t = (double)i * frame_period / 1000.0;
      int64_t p = matlab_round(t * 1000.0);
      p = p < 0 ? 0 : (p > nf - 1 ? nf - 1 : p);
      v = sm[p];
    }
    out[i] = v;
  }
}

}  // namespace

extern "C" int srn_harvest_decimate(const void* x, int x_is_f64, int64_t x_bs, const int32_t* lens, const double* coef,
                                    double* ws, int64_t ws_stride, double* y, int64_t y_bs, int B, int N, int ratio,
                                    int lag, void* stream) {
  SRN_CHECK_ARG(x && lens && coef && y, "harvest_decimate: null pointer");
  SRN_CHECK_ARG(B > 0 && N > 0 && x_bs >= N && ratio >= 1 && ratio <= SRN_HARVEST_MAX_RATIO && y_bs >= (N + ratio - 1) / ratio,
                "harvest_decimate: bad sizes (B %d, N %d, x_bs %lld, ratio %d, y_bs %lld)", B, N, (long long)x_bs,
                ratio, (long long)y_bs);
  SRN_CHECK_ARG(ratio == 1 || (ws && lag >= DEC_NFACT + 1 && lag % ratio == 0 &&
                               ws_stride >= (int64_t)N + 2 * (int64_t)lag + 2 * DEC_NFACT),
                "harvest_decimate: bad workspace (lag %d, ws_stride %lld)", lag, (long long)ws_stride);
  if (x_is_f64)
    hipLaunchKernelGGL(harvest_decimate_kernel<double>, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)x,
                       x_bs, lens, coef, ws, ws_stride, y, y_bs, ratio, lag);
  else
    hipLaunchKernelGGL(harvest_decimate_kernel<float>, dim3(B), dim3(64), 0, (hipStream_t)stream, (const float*)x,
                       x_bs, lens, coef, ws, ws_stride, y, y_bs, ratio, lag);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_harvest_channels(const double* y, int64_t y_bs, const int32_t* ylens, const int32_t* frames,
                                    const double* taps, const int32_t* tap_off, const int32_t* half_len,
                                    const double* boundary, int max_half_len, double* events, int64_t ev_cap,
                                    double* raw, int B, int ch0, int n_launch, int n_ch, int F1, int max_ylen,
                                    double fs, double f0_floor, double f0_ceil, void* stream) {
  SRN_CHECK_ARG(y && ylens && frames && taps && tap_off && half_len && boundary && events && raw,
                "harvest_channels: null pointer");
  SRN_CHECK_ARG(B > 0 && n_ch > 0 && ch0 >= 0 && n_launch > 0 && ch0 + n_launch <= n_ch && F1 > 0 && max_ylen > 0 &&
                    y_bs >= max_ylen,
                "harvest_channels: bad sizes (B %d, channels %d + %d of %d, F1 %d, max_ylen %d)", B, ch0, n_launch,
                n_ch, F1, max_ylen);
  SRN_CHECK_ARG(max_half_len >= 1 && 2 * max_half_len + 1 <= SRN_HARVEST_MAX_TAPS,
                "harvest_channels: %d taps > %d", 2 * max_half_len + 1, SRN_HARVEST_MAX_TAPS);
  SRN_CHECK_ARG(ev_cap >= 1 && ev_cap >= max_ylen / 2, "harvest_channels: ev_cap %lld < max_ylen / 2 = %d",
                (long long)ev_cap, max_ylen / 2);
  SRN_CHECK_ARG(fs > 0.0 && f0_floor > 0.0 && f0_ceil > f0_floor, "harvest_channels: bad parameters");
  hipLaunchKernelGGL(harvest_channels_kernel, dim3(n_launch, B), dim3(NT_CH), 0, (hipStream_t)stream, y, y_bs, ylens,
                     frames, taps, tap_off, half_len, boundary, events, ev_cap, raw, ch0, n_ch, F1, fs, f0_floor,
                     f0_ceil);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_harvest_candidates(const double* raw, const int32_t* frames, double* official, double* cand, int B,
                                      int n_ch, int F1, int n_base, void* stream) {
  SRN_CHECK_ARG(raw && frames && official && cand, "harvest_candidates: null pointer");
  SRN_CHECK_ARG(B > 0 && n_ch >= 3 && F1 > 0 && n_base > 0 && n_base * (2 * OVERLAP + 1) <= SRN_HARVEST_MAX_CAND,
                "harvest_candidates: bad sizes (B %d, n_ch %d, F1 %d, n_base %d)", B, n_ch, F1, n_base);
  hipLaunchKernelGGL(harvest_official_kernel, dim3((F1 + NT - 1) / NT, B), dim3(NT), 0, (hipStream_t)stream, raw,
                     frames, official, n_ch, F1, n_base);
  SRN_CHECK_LAUNCH();
  const int64_t total = (int64_t)F1 * n_base * (2 * OVERLAP + 1);
  hipLaunchKernelGGL(harvest_overlap_kernel, dim3((unsigned)((total + NT - 1) / NT), B), dim3(NT), 0,
                     (hipStream_t)stream, official, frames, cand, F1, n_base);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_harvest_refine(const double* y, int64_t y_bs, const int32_t* ylens, const int32_t* frames,
                                  const double* cand, double* refined, double* score, int B, int F1, int n_cand,
                                  double fs, double f0_floor, double f0_ceil, void* stream) {
  SRN_CHECK_ARG(y && ylens && frames && cand && refined && score, "harvest_refine: null pointer");
  SRN_CHECK_ARG(B > 0 && F1 > 0 && n_cand > 0 && n_cand <= SRN_HARVEST_MAX_CAND && fs > 0.0 && f0_floor > 0.0 &&
                    f0_ceil > f0_floor,
                "harvest_refine: bad sizes (B %d, F1 %d, n_cand %d)", B, F1, n_cand);
  SRN_CHECK_ARG(2 * (int)(1.5 * fs / f0_floor + 1.0) + 1 <= SRN_HARVEST_MAX_WINDOW,
                "harvest_refine: the window of f0_floor %g at %g Hz exceeds %d samples", f0_floor, fs,
                SRN_HARVEST_MAX_WINDOW);
  hipLaunchKernelGGL(harvest_refine_kernel, dim3((F1 + NT / 64 - 1) / (NT / 64), B), dim3(NT), 0, (hipStream_t)stream,
                     y, y_bs, ylens, frames, cand, refined, score, F1, n_cand, fs, f0_floor, f0_ceil);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_harvest_contour(const double* refined, const double* score, const int32_t* frames,
                                   const int32_t* out_frames, const double* smooth_coef, double* cand2, double* score2,
                                   double* fbuf, double* pool, int64_t pool_stride, int32_t* sections, int sec_cap,
                                   int32_t* status, double* f0_out, int64_t out_stride, int B, int F1, int n_cand,
                                   int F_out, int voice_range_minimum, double frame_period, void* stream) {
  SRN_CHECK_ARG(refined && score && frames && out_frames && smooth_coef && cand2 && score2 && fbuf && pool &&
                    sections && status && f0_out,
                "harvest_contour: null pointer");
  SRN_CHECK_ARG(B > 0 && F1 > 0 && n_cand > 0 && n_cand <= SRN_HARVEST_MAX_CAND && F_out > 0 && out_stride >= F_out &&
                    sec_cap > 0 && pool_stride > 0 && pool_stride < ((int64_t)1 << 31) && voice_range_minimum >= 1 &&
                    frame_period > 0.0,
                "harvest_contour: bad sizes (B %d, F1 %d, n_cand %d, F_out %d, sec_cap %d)", B, F1, n_cand, F_out,
                sec_cap);
  const int64_t total = (int64_t)F1 * n_cand;
  hipLaunchKernelGGL(harvest_remove_kernel, dim3((unsigned)((total + NT - 1) / NT), B), dim3(NT), 0,
                     (hipStream_t)stream, refined, score, frames, cand2, score2, F1, n_cand);
  SRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(harvest_contour_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, cand2, score2, frames,
                     out_frames, smooth_coef, fbuf, pool, pool_stride, sections, sec_cap, status, f0_out, out_stride,
                     F1, n_cand, F_out, voice_range_minimum, frame_period);
  SRN_CHECK_LAUNCH();
  return 0;
}
