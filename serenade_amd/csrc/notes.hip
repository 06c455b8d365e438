// notes.hip -- the host loop behind the note transcriber, on the GPU: what FramewiseDecoder.decode(pred, f0=...) does
// per utterance (serenade/modules/phoneme_midi/decoding.py:22-159: sigmoid, _peak_selector, _decode_notes and the
// pitch summary) and what serenade/bin/preprocess.py:237-259, 117-123, 510-528 does with the notes (midi_to_frames,
// _midi_to_hz(log_f0=True), the arithmetic of the est_lf0_score track).  serenade_amd/transcriber.py drives both
// (FramewiseDecoder.decode_batch, estimate_score_batch); tests/_notes_ref.py is the float64 restatement.
//   srn_note_decode   logits + pYIN contour of a ragged batch -> per item a note count, (onset, offset + 1) pairs and
//                     one pitch per note
//   srn_note_frames   notes of a ragged batch -> per item the MIDI number and the log-Hz score of every acoustic frame
//
// Both run ONE workgroup per item and read nothing of another item, so an item inside a batch gets the bits of its
// own B = 1 call; every reduction has an order fixed by the block size.  The data is a few hundred to a few thousand
// frames per item: the design goal is one launch per batch and exact decisions, not bandwidth.  Scratch lives in
// global memory (it stays in the caches); the frames of two notes of an item never overlap, so one scratch row per
// item serves every note.
//
// srn_note_decode, item of n frames (v = an activation curve, thr = its threshold):
//   activations   fp32 sigmoid 1 / (1 + exp(-x)) of the three channels (onset, offset, frame)
//   peaks         per curve, onset and offset alike: a run is a maximal stretch of frames with v > thr; a run still
//                 open at the last frame emits nothing; a closed run emits the FIRST frame attaining the maximum over
//                 {i in run : v[i] > v[0]} and nothing if that set is empty (the reference keeps "index 0" for "no run
//                 open", so frame 0 is never a peak and every peak value exceeds v[0])
//   onsets        the onset peaks in order; for onset k, nxt = the next onset, or n - 1 for the last; the search
//                 range is onset + 2 <= i < nxt
//   candidates    io = the first frame of the range attaining the maximum offset-peak value;
//                 if = the first fall frame of the range attaining the maximum dip confidence, where a fall frame has
//                 frame[i] >= 0.5 > frame[i + 1] and its confidence is max(1 - frame[j]) (fp32) over j = i + 1, ...
//                 while frame[j] < 0.5 and j < nxt; a confidence of 0 (no such j) does not count
//   offset        the later of io and if; nxt - 1 when neither exists; the note (onset, offset + 1) is emitted only
//                 if offset > onset
//   pitch input   the contour rounded to fp32 (the reference's .float()), then 12 (log2 f - log2 440) + 69 in fp64;
//                 the segment is [onset, offset] clipped to the contour's frames, L values of which m are not NaN
//   pitch         mode 0 median: the lower median (sorted[(m - 1) / 2]) of the non-NaN values;
//                 mode 1 weighted_mean: sum w p / sum w over the non-NaN values, w the periodic Hann window of
//                 length L, w[i] = 0.5 - 0.5 cos(2 pi i / L) (1 for L = 1);
//                 mode 2 weighted_median: weights of NaN frames zeroed, weights divided by their sum S, then
//                 numpy.interp(0.5, (C - w / 2) / C_last, sorted values) with C the running sum of the weights in
//                 sorted order (ties in index order): the last j with xp[j] <= 0.5 gives values[j] if it is the last
//                 value or xp[j] == 0.5, else values[j] + (0.5 - xp[j]) (values[j + 1] - values[j]) / (xp[j + 1] - xp[j]);
//                 a NaN result (no value, or S = 0) is 0
//   arithmetic    everything from the contour on is fp64, contraction off
// Thresholds are compared in fp32, as numpy compares a float32 element with a Python float.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"
#include "serenade_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

// the sum of one value per thread, to every thread: a tree of fixed shape in LDS (s holds NT doubles)
__device__ __forceinline__ double block_sum(double v, double* s) {
  const int tid = threadIdx.x;
  __syncthreads();  // s may still be read from the call before
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] = s[tid] + s[tid + o];
    __syncthreads();
  }
  return s[0];
}

// thread tid owns the `per` consecutive entries from tid * per; it brings how many of them it keeps and gets the
// number kept by the threads before it, and the total (s holds NT + 1 ints)
__device__ __forceinline__ int block_offsets(const int mine, int* s, int* total) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < NT; ++i) {
      const int c = s[i];
      s[i] = run;
      run += c;
    }
    s[NT] = run;
  }
  __syncthreads();
  *total = s[NT];
  return s[tid];
}

// order of the sort behind the medians: by value, ties by index
__device__ __forceinline__ bool before(const double a, const int ia, const double b, const int ib) {
  return a < b || (a == b && ia < ib);
}

__global__ __launch_bounds__(NT) void note_decode_kernel(
    const float* __restrict__ logits, const int32_t* __restrict__ frames, const double* __restrict__ f0,
    const int32_t* __restrict__ f0_frames, const int Tmax, const int Fmax, const float on_thr, const float off_thr,
    const int mode, const double log2_a4, float* __restrict__ ws_f, double* __restrict__ ws_d,
    int32_t* __restrict__ ws_i, int32_t* __restrict__ counts, int32_t* __restrict__ intervals,
    double* __restrict__ pitches) {
  __shared__ double s_d[NT];
  __shared__ int s_i[NT + 1];
  __shared__ double s_pick[4];  // weighted median: xp and value of j, then of j + 1
  __shared__ int s_rank;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(frames[b], 0), Tmax);
  const int nf = min(min(max(f0_frames[b], 0), Fmax), n);  // contour frames a segment can reach
  const float* lg = logits + (int64_t)b * Tmax * 3;
  const double* fb = f0 + (int64_t)b * Fmax;
  float* act = ws_f + (int64_t)b * 5 * Tmax;  // [3][Tmax] activations, then [2][Tmax] peak values (0 = no peak)
  float* pk = act + 3 * (int64_t)Tmax;
  double* pv = ws_d + (int64_t)b * 4 * Tmax;  // pitch per contour frame; weight, xp and rank of the note in hand
  double* wv = pv + Tmax;
  double* xv = wv + Tmax;
  double* rv = xv + Tmax;
  int32_t* on_idx = ws_i + (int64_t)b * 2 * Tmax;  // onset frames in order, then the offset found for each (-1: none)
  int32_t* on_off = on_idx + Tmax;
  int32_t* iv = intervals + (int64_t)b * Tmax * 2;
  double* pt = pitches + (int64_t)b * Tmax;

  // ---- activations, pitch per contour frame; every output entry starts as 0
  for (int t = tid; t < Tmax; t += NT) {
    iv[2 * t] = 0;
    iv[2 * t + 1] = 0;
    pt[t] = 0.0;
    if (t < n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) act[c * Tmax + t] = 1.0f / (1.0f + expf(-lg[3 * t + c]));
      pk[t] = 0.0f;
      pk[Tmax + t] = 0.0f;
    }
    if (t < nf) {
      const double f = (double)(float)fb[t];
      pv[t] = 12.0 * (log2(f) - log2_a4) + 69.0;  // NaN stays NaN
    }
  }
  __syncthreads();

  // ---- peaks: the thread of the frame that closes a run walks the run back
  for (int t = tid + 1; t < n; t += NT) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float* v = act + c * Tmax;
      const float thr = c == 0 ? on_thr : off_thr;
      if (v[t] > thr || !(v[t - 1] > thr)) continue;
      const float v0 = v[0];
      int best = -1;
      float top = 0.0f;
      for (int s = t - 1; s >= 0 && v[s] > thr; --s)
        if (v[s] > v0 && (best < 0 || v[s] >= top)) {
          best = s;
          top = v[s];
        }
      if (best >= 0) pk[c * Tmax + best] = top;
    }
  }
  __syncthreads();

  // ---- onsets in order
  const int per = (n + NT - 1) / NT;
  const int t0 = min(tid * per, n), t1 = min(t0 + per, n);
  int mine = 0;
  for (int t = t0; t < t1; ++t) mine += pk[t] > 0.0f;
  int n_on;
  int at = block_offsets(mine, s_i, &n_on);
  for (int t = t0; t < t1; ++t)
    if (pk[t] > 0.0f) on_idx[at++] = t;
  __syncthreads();

  // ---- one thread per onset: the offset of its note
  const float* poff = pk + Tmax;
  const float* fr = act + 2 * Tmax;
  for (int k = tid; k < n_on; k += NT) {
    const int onset = on_idx[k];
    const int nxt = k + 1 < n_on ? on_idx[k + 1] : n - 1;
    int io = -1, ifl = -1;
    float off_conf = 0.0f, fr_conf = 0.0f;
    for (int i = onset + 2; i < nxt; ++i) {
      if (poff[i] > off_conf) {
        off_conf = poff[i];
        io = i;
      }
      if (fr[i] >= 0.5f && fr[i + 1] < 0.5f) {  // i + 1 <= nxt <= n - 1
        float conf = 0.0f;
        for (int j = i + 1; j < nxt && fr[j] < 0.5f; ++j) conf = fmaxf(conf, 1.0f - fr[j]);
        if (conf > fr_conf) {
          fr_conf = conf;
          ifl = i;
        }
      }
    }
    int offset = max(io, ifl);
    if (offset < 0) offset = nxt - 1;
    on_off[k] = offset > onset ? offset : -1;
  }
  __syncthreads();

  // ---- the notes in order
  const int kper = (n_on + NT - 1) / NT;
  const int k0 = min(tid * kper, n_on), k1 = min(k0 + kper, n_on);
  mine = 0;
  for (int k = k0; k < k1; ++k) mine += on_off[k] >= 0;
  int n_notes;
  at = block_offsets(mine, s_i, &n_notes);
  for (int k = k0; k < k1; ++k)
    if (on_off[k] >= 0) {
      iv[2 * at] = on_idx[k];
      iv[2 * at + 1] = on_off[k] + 1;
      ++at;
    }
  if (tid == 0) counts[b] = n_notes;
  __syncthreads();

  // ---- one pitch per note, the whole workgroup on one note at a time
  for (int c = 0; c < n_notes; ++c) {
    const int onset = iv[2 * c];
    const int L = max(min(iv[2 * c + 1], nf) - onset, 0);
    const double* p = pv + onset;
    double* w = wv + onset;
    double sw = 0.0, swp = 0.0, cnt = 0.0;
    for (int e = tid; e < L; e += NT) {
      const double we = L == 1 ? 1.0 : 0.5 - 0.5 * cos(6.283185307179586476925 * (double)e / (double)L);
      const bool ok = p[e] == p[e];
      w[e] = ok ? we : 0.0;
      if (ok) {
        sw = sw + we;
        swp = swp + we * p[e];
        cnt = cnt + 1.0;
      }
    }
    const int m = (int)block_sum(cnt, s_d);
    double result = NAN;
    if (mode == 1) {
      const double S = block_sum(sw, s_d), SP = block_sum(swp, s_d);
      result = SP / S;
    } else if (mode == 0) {
      if (tid == 0) s_pick[0] = NAN;
      __syncthreads();
      for (int e = tid; e < L; e += NT) {
        const double pe = p[e];
        if (pe != pe) continue;
        int rank = 0;
        for (int j = 0; j < L; ++j) rank += before(p[j], j, pe, e);  // NaN is before nothing
        if (rank == (m - 1) / 2) s_pick[0] = pe;
      }
      __syncthreads();
      result = s_pick[0];
    } else {
      const double S = block_sum(sw, s_d);  // also makes w visible
      // xp and rank of every value; the last value, in sorted order, with xp <= 0.5
      int best = -1;
      for (int e = tid; e < L; e += NT) {
        const double pe = p[e];
        if (pe != pe) continue;
        int rank = 0;
        double C = 0.0;
        for (int j = 0; j < L; ++j) {
          const bool first = before(p[j], j, pe, e);
          rank += first;
          if (first) C = C + w[j] / S;
        }
        const double wn = w[e] / S;
        C = C + wn;
        xv[onset + e] = C - 0.5 * wn;
        rv[onset + e] = (double)rank;
      }
      // the weights are normalised before they are summed, so xp is divided by the last running sum, as numpy does
      double tot = 0.0;
      for (int e = tid; e < L; e += NT) tot = tot + w[e] / S;
      const double Cl = block_sum(tot, s_d);
      for (int e = tid; e < L; e += NT) {
        if (p[e] != p[e]) continue;
        xv[onset + e] = xv[onset + e] / Cl;
        if (xv[onset + e] <= 0.5) best = max(best, (int)rv[onset + e]);
      }
      if (tid == 0) {
        s_rank = -1;
        s_pick[0] = s_pick[1] = s_pick[2] = s_pick[3] = NAN;
      }
      __syncthreads();
      if (best >= 0) atomicMax(&s_rank, best);
      __syncthreads();
      const int rj = max(s_rank, 0);  // 0.5 below every xp: numpy's left value, the first
      for (int e = tid; e < L; e += NT) {
        if (p[e] != p[e]) continue;
        const int r = (int)rv[onset + e];
        if (r == rj) {
          s_pick[0] = xv[onset + e];
          s_pick[1] = p[e];
        } else if (r == rj + 1) {
          s_pick[2] = xv[onset + e];
          s_pick[3] = p[e];
        }
      }
      __syncthreads();
      if (m > 0 && Cl == Cl) {
        const double xj = s_pick[0], vj = s_pick[1], xn = s_pick[2], vn = s_pick[3];
        if (s_rank < 0 || rj == m - 1 || xj == 0.5)
          result = vj;
        else
          result = (vn - vj) / (xn - xj) * (0.5 - xj) + vj;
      }
    }
    if (tid == 0) pt[c] = result == result ? result : 0.0;
    __syncthreads();  // s_pick and the scratch rows are reused by the next note
  }
}

__global__ __launch_bounds__(NT) void note_frames_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ intervals, const double* __restrict__ pitches,
    const int cap, const int32_t* __restrict__ n_samples, const double scale, const double shift,
    const double sampling_rate, const int32_t* __restrict__ table, int32_t* __restrict__ ws,
    int32_t* __restrict__ midi, int32_t* __restrict__ lf0, const int Nmax, int32_t* __restrict__ n_frames,
    int32_t* __restrict__ bad) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int count = min(max(counts[b], 0), cap);
  const double nd = ceil(((double)n_samples[b] / sampling_rate) / shift);
  const int n = nd > 0.0 ? (nd < (double)Nmax ? (int)nd : Nmax) : 0;
  const int32_t* iv = intervals + (int64_t)b * cap * 2;
  const double* pt = pitches + (int64_t)b * cap;
  int32_t* note = ws + (int64_t)b * cap * 3;  // start frame, end frame, MIDI number of every note
  int32_t* mo = midi + (int64_t)b * Nmax;
  int32_t* lo = lf0 + (int64_t)b * Nmax;
  if (tid == 0) n_frames[b] = n;
  for (int k = tid; k < count; k += NT) {
    const double r = rint(pt[k]);  // half to even, Python's round
    const bool ok = r >= 0.0 && r <= 127.0 && iv[2 * k] >= 0;
    if (!ok) atomicOr(bad, 1);
    // numpy's two operations, in its order: (frame * scale) / shift
    const double s = floor(((double)iv[2 * k] * scale) / shift);
    const double e = ceil(((double)iv[2 * k + 1] * scale) / shift);
    note[3 * k] = ok ? (int)fmin(fmax(s, 0.0), (double)n) : n;
    note[3 * k + 1] = ok ? (int)fmin(fmax(e, 0.0), (double)n) : n;
    note[3 * k + 2] = ok ? (int)r : 0;
  }
  __syncthreads();
  for (int f = tid; f < Nmax; f += NT) {
    int v = 0;
    if (f < n)
      for (int k = count - 1; k >= 0; --k)  // the last note covering a frame wins
        if (note[3 * k] <= f && f < note[3 * k + 1]) {
          v = note[3 * k + 2];
          break;
        }
    mo[f] = v;
    lo[f] = table[v];
  }
}

}  // namespace

extern "C" int srn_note_decode(const float* logits, const int32_t* frames, const double* f0, const int32_t* f0_frames,
                               int B, int Tmax, int Fmax, float onset_threshold, float offset_threshold, int pitch_sum,
                               double log2_a4, float* ws_f, double* ws_d, int32_t* ws_i, int32_t* counts,
                               int32_t* intervals, double* pitches, void* stream) {
  SRN_CHECK_ARG(logits && frames && f0 && f0_frames && ws_f && ws_d && ws_i && counts && intervals && pitches,
                "note_decode: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && Tmax > 0 && Tmax <= SRN_NOTE_MAX_FRAMES && Fmax > 0,
                "note_decode: bad sizes (B %d, Tmax %d <= %d, Fmax %d)", B, Tmax, SRN_NOTE_MAX_FRAMES, Fmax);
  SRN_CHECK_ARG(pitch_sum >= 0 && pitch_sum <= 2, "note_decode: pitch_sum %d is none of 0, 1, 2", pitch_sum);
  hipLaunchKernelGGL(note_decode_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, logits, frames, f0, f0_frames,
                     Tmax, Fmax, onset_threshold, offset_threshold, pitch_sum, log2_a4, ws_f, ws_d, ws_i, counts,
                     intervals, pitches);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_note_frames(const int32_t* counts, const int32_t* intervals, const double* pitches, int B, int cap,
                               const int32_t* n_samples, double scale, double shift, double sampling_rate,
                               const int32_t* table, int32_t* ws, int32_t* midi, int32_t* lf0, int Nmax,
                               int32_t* n_frames, int32_t* bad, void* stream) {
  SRN_CHECK_ARG(counts && intervals && pitches && n_samples && table && ws && midi && lf0 && n_frames && bad,
                "note_frames: null pointer");
  SRN_CHECK_ARG(B > 0 && B <= 65535 && cap > 0 && Nmax > 0 && scale > 0.0 && shift > 0.0 && sampling_rate > 0.0,
                "note_frames: bad sizes (B %d, cap %d, Nmax %d, scale %g, shift %g, rate %g)", B, cap, Nmax, scale,
                shift, sampling_rate);
  srn_zero_u32((unsigned*)bad, 1, (hipStream_t)stream);
  hipLaunchKernelGGL(note_frames_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, counts, intervals, pitches, cap,
                     n_samples, scale, shift, sampling_rate, table, ws, midi, lf0, Nmax, n_frames, bad);
  SRN_CHECK_LAUNCH();
  return 0;
}
