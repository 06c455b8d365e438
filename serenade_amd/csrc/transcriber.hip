// transcriber.hip -- the phoneme-informed MIDI note transcriber's own kernels (serenade_amd/transcriber.py; the
// `est_lf0_score` track of serenade/bin/preprocess.py:374-383,506-528, TranscriptionModel in
// serenade/modules/phoneme_midi/model.py, phonerec_model.py, subnetworks.py, feature.py).  The STFT, conv layers 1-2
// of every conv stack, the flatten + Linear layers and the LSTM input projections are srn_conv_gemm.  Here:
//   srn_pad_ragged        reflect padding that mirrors at each item's own end (nnAudio center=True on one item)
//   srn_mel_db            power spectrum @ mel matrix -> 10 log10(max(., amin)) -> max(., max_item - top_db), the
//                         maximum taken per item over its own valid frames (AmplitudeToDB of a B = 1 call)
//   srn_trans_conv0       conv-stack layer 0: Conv2d(1 -> C, 3x3, time dilation 1 or 2) + folded BN + ReLU, written
//                         as a channels-last image with one zero border column on each side of the frequency axis
//   srn_trans_pool        MaxPool2d((1, 2)) that re-zeroes the border, or (flatten) writes the (B, T, C * F/2) rows of
//                         the stack's Linear in channel-major order
//   srn_bilstm_recur      the sequential part of a bidirectional nn.LSTM on a precomputed input projection
#include <hip/hip_runtime.h>

#include "common.h"
#include "serenade_hip.h"

namespace {

// out[b][i] = x[b][reflect(i - pad)] with the reflection at L = min(lens[b], n), for i < L + 2 pad; 0 up to ld
__global__ __launch_bounds__(256) void pad_ragged_kernel(const float* __restrict__ x, const int64_t x_bs,
                                                         const int32_t* __restrict__ lens, float* __restrict__ out,
                                                         const int n, const int pad, const int ld) {
  const int b = blockIdx.y;
  const int L = max(min(lens[b], n), 1);
  const float* xb = x + (int64_t)b * x_bs;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ld; i += gridDim.x * 256) {
    float v = 0.f;
    if (i < L + 2 * pad) {
      int j = i - pad;
      if (j < 0) j = -j;
      if (j >= L) j = 2 * (L - 1) - j;
      j = min(max(j, 0), L - 1);
      v = xb[j];
    }
    out[(int64_t)b * ld + i] = v;
  }
}

// float <-> unsigned with the same order (negative values included): an integer atomicMax gives the exact maximum
__device__ __forceinline__ unsigned f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// one workgroup per (frame, item): the power spectrum of the frame into LDS, then mel bin m per thread (mel_t is
// (nb, n_mels): lanes read consecutive addresses); dB of valid frames, 0 on frames at or past lens[b]; the item's
// maximum dB goes to gmax[b] (order-preserving bits)
__global__ __launch_bounds__(256) void mel_db_kernel(const float* __restrict__ spec, const int ld_spec,
                                                     const int nb, const float* __restrict__ mel_t,
                                                     const int32_t* __restrict__ lens, unsigned* __restrict__ gmax,
                                                     float* __restrict__ out, const int ld_out, const int T,
                                                     const int n_mels, const float amin) {
  extern __shared__ float pw[];
  const int t = blockIdx.x, b = blockIdx.y;
  const bool live = t < min(lens[b], T);
  const float* row = spec + ((int64_t)b * T + t) * ld_spec;
  float* o = out + ((int64_t)b * T + t) * ld_out;
  if (!live) {
    for (int m = threadIdx.x; m < n_mels; m += 256) o[m] = 0.f;
    return;
  }
  for (int f = threadIdx.x; f < nb; f += 256) {
    const float re = row[f], im = row[nb + f];
    pw[f] = re * re + im * im;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int m = threadIdx.x; m < n_mels; m += 256) {
    float a = 0.f;
    for (int f = 0; f < nb; ++f) a = fmaf(pw[f], mel_t[f * n_mels + m], a);
    const float db = 10.f * log10f(fmaxf(a, amin));
    o[m] = db;
    mx = fmaxf(mx, db);
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && mx > -INFINITY) atomicMax(gmax + b, f2ord(mx));
}

// x = max(x, max_b - top_db) on the valid frames of item b
__global__ __launch_bounds__(256) void db_clamp_kernel(float* __restrict__ out, const int ld_out,
                                                       const int32_t* __restrict__ lens,
                                                       const unsigned* __restrict__ gmax, const int T,
                                                       const int n_mels, const float top_db) {
  const int b = blockIdx.y;
  const int len = min(lens[b], T);
  const float floor_db = ord2f(gmax[b]) - top_db;
  const int64_t n = (int64_t)len * n_mels;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / n_mels), m = (int)(i - (int64_t)t * n_mels);
    float* p = out + ((int64_t)b * T + t) * ld_out + m;
    *p = fmaxf(*p, floor_db);
  }
}

// out[b][t][f + 1][c] = ReLU(bias[c] + sum_{dt, df} w[c][dt][df] x[b][t + (dt - 1) dil][f + df - 1]) for t < lens[b],
// 0 <= f < F; input taps outside [0, lens[b]) x [0, F) read as zero; border columns and padded frames are 0.
// One thread per output element, channels fastest (the lanes of a wave share their input taps).
__global__ __launch_bounds__(256) void trans_conv0_kernel(const float* __restrict__ x, const int64_t x_bs,
                                                          const int ld_x, const int32_t* __restrict__ lens,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, const int T, const int F,
                                                          const int C, const int dil) {
  const int b = blockIdx.y;
  const int len = min(lens[b], T);
  const int W = F + 2;
  const int64_t n = (int64_t)T * W * C;
  const float* xb = x + (int64_t)b * x_bs;
  float* ob = out + (int64_t)b * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int t = (int)(r / W), fb = (int)(r - (int64_t)t * W);
    float v = 0.f;
    if (t < len && fb >= 1 && fb <= F) {
      const float* wc = w + c * 9;
      float a = bias[c];
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const int tt = t + (dt - 1) * dil;
        if (tt < 0 || tt >= len) continue;
#pragma unroll
        for (int df = 0; df < 3; ++df) {
          const int ff = fb - 2 + df;
          if (ff >= 0 && ff < F) a = fmaf(wc[dt * 3 + df], xb[(int64_t)tt * ld_x + ff], a);
        }
      }
      v = fmaxf(a, 0.f);
    }
    ob[i] = v;
  }
}

// in (B, T, Fin + 2, C) bordered -> Fo = Fin / 2 pooled columns.  flatten == 0: out (B, T, Fo + 2, C) bordered;
// flatten == 1: out (B, T, ld_out), column c Fo + f for c < Cv, zeros in [Cv Fo, ld_out).  Padded frames are 0.
__global__ __launch_bounds__(256) void trans_pool_kernel(const float* __restrict__ in, const int32_t* __restrict__ lens,
                                                         float* __restrict__ out, const int T, const int Fin,
                                                         const int C, const int Cv, const int flatten,
                                                         const int ld_out) {
  const int b = blockIdx.y;
  const int len = min(lens[b], T);
  const int Fo = Fin / 2;
  const int Wi = Fin + 2;
  const int Wr = flatten ? ld_out : (Fo + 2) * C;  // output floats per frame
  const int64_t n = (int64_t)T * Wr;
  const float* ib = in + (int64_t)b * T * Wi * C;
  float* ob = out + (int64_t)b * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / Wr);
    const int e = (int)(i - (int64_t)t * Wr);
    int c, f;  // f: pooled column, -1 if the element is a border / padding column
    if (flatten) {
      c = e / Fo;
      f = c < Cv ? e - c * Fo : -1;
    } else {
      c = e % C;
      f = e / C - 1;
      if (f >= Fo) f = -1;
    }
    float v = 0.f;
    if (t < len && f >= 0) {
      const float* p = ib + ((int64_t)t * Wi + 2 * f + 1) * C + c;
      v = fmaxf(p[0], p[C]);
    }
    ob[i] = v;
  }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Bidirectional LSTM recurrence (nn.LSTM, gate order i, f, g, o, zero initial state) on g = x W_ih^T + b_ih + b_hh
// (B, T, ld_g): columns [0, 4H) forward, [4H, 8H) reverse.  One workgroup per (item, direction) -- blockIdx.x =
// 2 b + dir, so with an even number of XCDs each XCD's L2 holds one direction's W_hh.  The forward direction runs
// t = 0 .. len - 1, the reverse one t = len - 1 .. 0, len = min(lens[b], T); out[b][t][dir H + j] = h_t, rows t >= len
// are 0.  w_t [dir][k][j][gate] = W_hh[dir][gate H + j][k]: thread (slice s, unit j) owns the four gate rows of unit j
// over the k-slice s and reads them as one float4 per k (lanes: consecutive j, consecutive 16 B); the KS slice
// partials meet in LDS, and the slice-0 thread applies the gate math and keeps c_j in a register.  h is double-buffered
// in LDS.  W_hh (4 H^2 floats, 2.4 MB at H = 384) does not fit in LDS: it streams from L2 every step.
__global__ __launch_bounds__(1024) void bilstm_recur_kernel(const float* __restrict__ g, const int64_t g_bs,
                                                            const int ld_g, const int32_t* __restrict__ lens,
                                                            const float* __restrict__ w_t, float* __restrict__ out,
                                                            const int64_t out_bs, const int ld_out, const int T,
                                                            const int H, const int KS) {
  extern __shared__ float sm[];
  float* hbuf = sm;                                     // [2][H]
  float4* part = reinterpret_cast<float4*>(sm + 2 * H);  // [KS][H]   (H % 8 == 0: 16-byte aligned)
  const int dir = blockIdx.x & 1, b = blockIdx.x >> 1;
  const int tid = threadIdx.x;
  const int s = tid / H, j = tid - s * H;
  const bool active = s < KS;
  const int len = min(max(lens[b], 0), T);
  const int kc = (H + KS - 1) / KS;
  const int k0 = min(s * kc, H), k1 = min(k0 + kc, H);
  const float4* W = reinterpret_cast<const float4*>(w_t) + (int64_t)dir * H * H;
  const float* gb = g + (int64_t)b * g_bs + dir * 4 * H;
  float* ob = out + (int64_t)b * out_bs + dir * H;
  for (int i = tid; i < 2 * H; i += blockDim.x) hbuf[i] = 0.f;
  float c = 0.f;
  __syncthreads();
  for (int step = 0; step < len; ++step) {
    const int t = dir ? len - 1 - step : step;
    const float* hc = hbuf + (step & 1) * H;
    float* hn = hbuf + ((step + 1) & 1) * H;
    float xi = 0.f, xf = 0.f, xg = 0.f, xo = 0.f;
    if (s == 0) {
      const float* gr = gb + (int64_t)t * ld_g;
      xi = gr[j];
      xf = gr[H + j];
      xg = gr[2 * H + j];
      xo = gr[3 * H + j];
    }
    if (active) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4* wk = W + (int64_t)k0 * H + j;
#pragma unroll 8
      for (int k = k0; k < k1; ++k) {
        const float4 w = wk[(int64_t)(k - k0) * H];
        const float hv = hc[k];
        a.x = fmaf(w.x, hv, a.x);
        a.y = fmaf(w.y, hv, a.y);
        a.z = fmaf(w.z, hv, a.z);
        a.w = fmaf(w.w, hv, a.w);
      }
      part[s * H + j] = a;
    }
    __syncthreads();
    if (s == 0) {
      float4 acc = part[j];
      for (int q = 1; q < KS; ++q) {
        const float4 p = part[q * H + j];
        acc.x += p.x;
        acc.y += p.y;
        acc.z += p.z;
        acc.w += p.w;
      }
      const float ig = sigmoidf_(xi + acc.x);
      const float fg = sigmoidf_(xf + acc.y);
      const float cg = tanhf(xg + acc.z);
      const float og = sigmoidf_(xo + acc.w);
      c = fmaf(fg, c, ig * cg);
      const float h = og * tanhf(c);
      hn[j] = h;
      ob[(int64_t)t * ld_out + j] = h;
    }
    __syncthreads();
  }
  const int64_t rest = (int64_t)(T - len) * H;
  for (int64_t i = tid; i < rest; i += blockDim.x) {
    const int t = len + (int)(i / H), jj = (int)(i % H);
    ob[(int64_t)t * ld_out + jj] = 0.f;
  }
}

inline int grid_for(int64_t n, int cap) {
  const int64_t blocks = (n + 255) / 256;
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

}  // namespace

extern "C" int srn_pad_ragged(const float* x, int64_t x_bs, const int32_t* lens, float* out, int B, int n, int pad,
                              int ld, void* stream) {
  SRN_CHECK_ARG(x && lens && out, "pad_ragged: null pointer");
  SRN_CHECK_ARG(B > 0 && n > 0 && pad >= 0 && ld >= n + 2 * pad && x_bs >= n,
                "pad_ragged: bad sizes (B %d, n %d, pad %d, ld %d, x_bs %lld)", B, n, pad, ld, (long long)x_bs);
  hipLaunchKernelGGL(pad_ragged_kernel, dim3(grid_for(ld, 4096), B), dim3(256), 0, (hipStream_t)stream, x, x_bs, lens,
                     out, n, pad, ld);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_mel_db(const float* spec, int ld_spec, int n_bins, const float* mel_t, const int32_t* lens,
                          unsigned* gmax_ws, float* out, int ld_out, int B, int T, int n_mels, float amin,
                          float top_db, void* stream) {
  SRN_CHECK_ARG(spec && mel_t && lens && gmax_ws && out, "mel_db: null pointer");
  SRN_CHECK_ARG(B > 0 && T > 0 && n_bins > 0 && n_bins <= 8192 && ld_spec >= 2 * n_bins && n_mels > 0 &&
                    ld_out >= n_mels && amin > 0.f && top_db >= 0.f,
                "mel_db: bad sizes (B %d, T %d, n_bins %d, ld_spec %d, n_mels %d, ld_out %d)", B, T, n_bins, ld_spec,
                n_mels, ld_out);
  hipStream_t st = (hipStream_t)stream;
  srn_zero_u32(gmax_ws, B, st);
  SRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mel_db_kernel, dim3(T, B), dim3(256), (size_t)n_bins * sizeof(float), st, spec, ld_spec, n_bins,
                     mel_t, lens, gmax_ws, out, ld_out, T, n_mels, amin);
  SRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(db_clamp_kernel, dim3(grid_for((int64_t)T * n_mels, 2048), B), dim3(256), 0, st, out, ld_out,
                     lens, gmax_ws, T, n_mels, top_db);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_trans_conv0(const float* x, int64_t x_bs, int ld_x, const int32_t* lens, const float* w,
                               const float* bias, float* out, int B, int T, int F, int C, int dilation, void* stream) {
  SRN_CHECK_ARG(x && lens && w && bias && out, "trans_conv0: null pointer");
  SRN_CHECK_ARG(B > 0 && T > 0 && F > 0 && C > 0 && ld_x >= F && x_bs >= (int64_t)T * ld_x &&
                    (dilation == 1 || dilation == 2),
                "trans_conv0: bad sizes (B %d, T %d, F %d, C %d, ld_x %d, dilation %d)", B, T, F, C, ld_x, dilation);
  hipLaunchKernelGGL(trans_conv0_kernel, dim3(grid_for((int64_t)T * (F + 2) * C, 4096), B), dim3(256), 0,
                     (hipStream_t)stream, x, x_bs, ld_x, lens, w, bias, out, T, F, C, dilation);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_trans_pool(const float* in, const int32_t* lens, float* out, int B, int T, int F_in, int C,
                              int C_valid, int flatten, int ld_out, void* stream) {
  SRN_CHECK_ARG(in && lens && out && in != out, "trans_pool: null pointer, or out aliases in");
  SRN_CHECK_ARG(B > 0 && T > 0 && F_in >= 2 && C > 0 && C_valid > 0 && C_valid <= C && (flatten == 0 || flatten == 1),
                "trans_pool: bad sizes (B %d, T %d, F_in %d, C %d, C_valid %d)", B, T, F_in, C, C_valid);
  SRN_CHECK_ARG(!flatten || ld_out >= C_valid * (F_in / 2), "trans_pool: ld_out %d < %d", ld_out, C_valid * (F_in / 2));
  const int64_t per = flatten ? (int64_t)ld_out : (int64_t)(F_in / 2 + 2) * C;
  hipLaunchKernelGGL(trans_pool_kernel, dim3(grid_for((int64_t)T * per, 4096), B), dim3(256), 0, (hipStream_t)stream,
                     in, lens, out, T, F_in, C, C_valid, flatten, ld_out);
  SRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int srn_bilstm_slices(int H) {
  if (H < 32 || H > 512 || H % 8 != 0) return 0;
  const int ks = 1024 / H;
  return ks > 16 ? 16 : ks;
}

extern "C" int srn_bilstm_recur(const float* g, int64_t g_bs, int ld_g, const int32_t* lens, const float* w_hh_t,
                                float* out, int64_t out_bs, int ld_out, int B, int T, int H, void* stream) {
  SRN_CHECK_ARG(g && lens && w_hh_t && out, "bilstm_recur: null pointer");
  SRN_CHECK_ARG(H >= 32 && H <= 512 && H % 8 == 0, "bilstm_recur: H %d must be a multiple of 8 in [32, 512]", H);
  SRN_CHECK_ARG(B > 0 && T > 0 && ld_g >= 8 * H && g_bs >= (int64_t)T * ld_g && ld_out >= 2 * H &&
                    out_bs >= (int64_t)T * ld_out,
                "bilstm_recur: bad sizes (B %d, T %d, H %d, ld_g %d, g_bs %lld, ld_out %d, out_bs %lld)", B, T, H,
                ld_g, (long long)g_bs, ld_out, (long long)out_bs);
  SRN_CHECK_ARG((reinterpret_cast<uintptr_t>(w_hh_t) & 15) == 0, "bilstm_recur: w_hh_t must be 16-byte aligned");
  const int ks = srn_bilstm_slices(H);
  const int threads = (ks * H + 63) / 64 * 64;
  const size_t smem = (size_t)(2 * H + 4 * ks * H) * sizeof(float);
  hipLaunchKernelGGL(bilstm_recur_kernel, dim3(2 * B), dim3(threads), smem, (hipStream_t)stream, g, g_bs, ld_g, lens,
                     w_hh_t, out, out_bs, ld_out, T, H, ks);
  SRN_CHECK_LAUNCH();
  return 0;
}
