"""pYIN F0 estimation on the GPU: librosa 0.10 `librosa.pyin`, batched and ragged.  The reference runs it on the host
inside FramewiseDecoder.decode (serenade/modules/phoneme_midi/decoding.py:36-45) to give each decoded note its pitch;
transcriber.reference_f0 makes that exact call through here.

    pyin(wave, lengths=None, *, fmin, fmax, sr=22050, frame_length=2048, ...)   librosa's keywords and defaults
        -> (f0 float64, voiced_flag bool, voiced_prob float64, frames int64)

wave is (B, N) or (N,) float32 on the GPU; item b has lengths[b] samples and frames[b] = 1 + lengths[b] // hop frames
(center=True).  Every item gets exactly what its own B = 1 call gets; entries past an item's frames hold fill_na,
False and 0.

Two HIP entry points (serenade_amd/csrc/pyin.hip): srn_pyin_observe (one workgroup per frame: difference function,
cumulative mean normalisation, parabolic shifts, troughs and their threshold-prior probabilities, the voiced
observation row) and srn_pyin_viterbi (one workgroup per item: the log-domain Viterbi over 2 n_bins states and the
backtrack).  Everything data-independent is built here with numpy / scipy and passed as tables, so only data-dependent
arithmetic runs on the GPU.  Plans (tables and buffers) are cached per (device, B, N, lengths, parameters).

Parity: tests/_pyin_ref.py (float64 numpy + scipy restatement of librosa 0.10) is the pin; librosa is not installed
where this project is tested ("parity unpinned", like the log-mel row).
"""
import math

import numpy as np
import scipy.signal
import scipy.stats
import torch

from . import ops
from .plan import dev_f64, dev_i32, item_lengths, lru_get

__all__ = ["pyin", "pyin_geometry", "pyin_frames"]

TINY = np.finfo(np.float64).tiny
MAX_FRAME, MAX_PERIODS, MAX_STATES, MAX_THRESHOLDS = 4096, 1024, 4096, 1024  # SRN_PYIN_MAX_* of serenade_hip.h


def pyin_geometry(*, fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None, resolution=0.1,
                  max_transition_rate=35.92):
    """the derived sizes of one pyin call (librosa 0.10): periods, pitch bins, transition width"""
    if win_length is None:
        win_length = frame_length // 2
    if hop_length is None:
        hop_length = frame_length // 4
    nbps = int(np.ceil(1.0 / resolution))
    return dict(win_length=win_length, hop_length=hop_length, min_period=int(np.floor(sr / fmax)),
                max_period=min(int(np.ceil(sr / fmin)), frame_length - win_length - 1), nbps=nbps,
                n_bins=int(np.floor(12 * nbps * np.log2(fmax / fmin))) + 1,
                width=round(max_transition_rate * 12 * hop_length / sr) * nbps + 1)


def pyin_frames(lengths, frame_length=2048, hop_length=None, center=True):
    """frames of each item: 1 + (n + 2 (frame_length // 2) - frame_length) // hop centred (1 + n // hop for an even
    frame_length), 1 + (n - frame_length) // hop otherwise"""
    hop = frame_length // 4 if hop_length is None else hop_length
    pad = frame_length // 2 if center else 0
    return [1 + (int(n) + 2 * pad - frame_length) // hop for n in lengths]


def _check(sr, fmin, fmax, frame_length, win_length, hop_length, n_thresholds, resolution, center, pad_mode,
           max_transition_rate=35.92):
    """librosa's __check_yin_params and transition_local's width rule, then the limits of the kernels"""
    if fmin is None or fmax is None:
        raise ValueError("pyin: both fmin and fmax must be provided")
    if fmax > sr / 2:
        raise ValueError(f"pyin: fmax={fmax:.3f} cannot exceed the Nyquist frequency {sr / 2}")
    if fmin >= fmax:
        raise ValueError(f"pyin: fmin={fmin:.3f} must be less than fmax={fmax:.3f}")
    if fmin <= 0:
        raise ValueError(f"pyin: fmin={fmin} must be positive")
    if frame_length <= 0 or win_length <= 0:
        raise ValueError(f"pyin: frame_length={frame_length} and win_length={win_length} must be positive")
    if win_length >= frame_length:
        raise ValueError(f"pyin: win_length={win_length} must be less than frame_length={frame_length}")
    if frame_length - win_length - 1 <= sr // fmax:
        raise ValueError(f"pyin: fmax={fmax:.3f} is too small for frame_length={frame_length} and "
                         f"win_length={win_length} (the shortest period does not fit the frame)")
    if hop_length <= 0:
        raise ValueError(f"pyin: hop_length={hop_length} must be positive")
    if n_thresholds < 1 or resolution <= 0:
        raise ValueError(f"pyin: n_thresholds={n_thresholds} and resolution={resolution} must be positive")
    if center and pad_mode != "constant":
        raise ValueError(f"pyin: pad_mode {pad_mode!r} is not supported (librosa 0.10's default 'constant' is)")
    g = pyin_geometry(fmin=fmin, fmax=fmax, sr=sr, frame_length=frame_length, win_length=win_length,
                      hop_length=hop_length, resolution=resolution, max_transition_rate=max_transition_rate)
    if not 1 <= g["width"] <= g["n_bins"]:  # librosa: transition_local's "width must be between 1 and n_states"
        raise ValueError(f"pyin: transition width {g['width']} (max_transition_rate={max_transition_rate} at "
                         f"hop_length={hop_length}) must lie between 1 and the {g['n_bins']} pitch bins")


def transition_local(n_states, width):
    """librosa.sequence.transition_local(n_states, width, window="triangle", wrap=False)"""
    transition = np.zeros((n_states, n_states), dtype=np.float64)
    win = scipy.signal.get_window("triang", width, fftbins=False)
    lpad = (n_states - width) // 2
    for i in range(n_states):
        row = np.roll(np.pad(win, (lpad, n_states - width - lpad)), n_states // 2 + i + 1)
        row[min(n_states, i + width // 2 + 1):] = 0
        row[:max(0, i - width // 2)] = 0
        transition[i] = row
    transition /= transition.sum(axis=1, keepdims=True)
    return transition


def log_band(n_bins, width, switch_prob):
    """(2, width, n_bins) log-transition band of kron(transition_loop(2, 1 - switch), transition_local): [0] keeps the
    voicing, [1] switches it; [k][d + width // 2][q] = log(p T[q + d][q] + tiny), log(tiny) where q + d is no bin"""
    T = transition_local(n_bins, width)
    stay = 1 - switch_prob
    p = (stay, (1.0 - stay) / 1)  # transition_loop(2, stay): the diagonal, then (1 - stay) / (n_states - 1)
    h = width // 2
    out = np.full((2, width, n_bins), np.log(TINY))
    q = np.arange(n_bins)
    for d in range(-h, h + 1):
        ok = (q + d >= 0) & (q + d < n_bins)
        for k in range(2):
            out[k, d + h, ok] = np.log(p[k] * T[q[ok] + d, q[ok]] + TINY)
    return out


def prior_tables(n_thresholds, beta_parameters, boltzmann_parameter, no_trough_prob, n_periods):
    """thresholds, beta_probs, Boltzmann factors fact[count] and exp(-lambda position), no-trough mass per count"""
    thr = np.linspace(0, 1, n_thresholds + 1)
    beta_probs = np.diff(scipy.stats.beta.cdf(thr, beta_parameters[0], beta_parameters[1]))
    lam = boltzmann_parameter
    with np.errstate(divide="ignore", invalid="ignore"):
        fact = (1 - np.exp(-lam)) / (1 - np.exp(-lam * np.arange(n_periods + 1)))  # scipy boltzmann._pmf
    fact[0] = 0.0  # count 0: never read
    bexp = np.exp(-lam * np.arange(n_periods))
    no_trough = np.array([no_trough_prob * np.sum(beta_probs[:m]) for m in range(n_thresholds + 1)])
    return thr[1:], beta_probs, fact, bexp, no_trough


def _require_cuda(wave):
    if not (isinstance(wave, torch.Tensor) and wave.is_cuda and wave.dtype == torch.float32 and wave.ndim in (1, 2)):
        raise RuntimeError("pyin: wave must be a (B, N) or (N,) float32 CUDA (ROCm) tensor; there is no CPU path")


class _PyinPlan:
    """tables, buffers and the prebuilt Viterbi op of one (device, B, N, lengths, parameters) call; only the
    observation kernel reads the caller's wave, so only its op is built per call"""

    def __init__(self, dev, B, N, lengths, key):
        (sr, fmin, fmax, frame_length, win_length, hop_length, n_thresholds, beta_parameters, boltzmann_parameter,
         resolution, max_transition_rate, switch_prob, no_trough_prob, fill_na, center) = key
        g = pyin_geometry(fmin=fmin, fmax=fmax, sr=sr, frame_length=frame_length, win_length=win_length,
                          hop_length=hop_length, resolution=resolution, max_transition_rate=max_transition_rate)
        self.g = g
        n, nf = g["n_bins"], g["max_period"] - g["min_period"] + 1
        if g["min_period"] < 1 or not 3 <= nf <= MAX_PERIODS or frame_length > MAX_FRAME or 2 * n > MAX_STATES \
                or n_thresholds > MAX_THRESHOLDS or g["width"] % 2 != 1:
            raise ValueError(f"pyin: outside the kernels' limits (frame_length {frame_length} <= {MAX_FRAME}, "
                             f"{nf} periods in [3, {MAX_PERIODS}], {2 * n} states <= {MAX_STATES}, "
                             f"n_thresholds {n_thresholds} <= {MAX_THRESHOLDS}, odd transition width {g['width']})")
        self.pad = frame_length // 2 if center else 0
        frames = pyin_frames(lengths, frame_length, g["hop_length"], center)
        if min(frames) < 1:
            raise ValueError(f"pyin: an item is shorter than frame_length={frame_length} (center=False)")
        self.B, self.N, self.T = B, N, max(frames)
        self.frames = torch.tensor(frames, dtype=torch.int64)
        self.sr, self.fmin = float(sr), float(fmin)
        self.frame_length, self.n_thresholds = frame_length, n_thresholds
        f64 = lambda a: dev_f64(a, dev)
        self.d_lens, self.d_frames = dev_i32(lengths, dev), dev_i32(frames, dev)
        thr, beta_probs, fact, bexp, no_trough = prior_tables(n_thresholds, beta_parameters, boltzmann_parameter,
                                                              no_trough_prob, nf)
        self.tabs = [f64(a) for a in (thr, beta_probs, fact, bexp, no_trough)]
        band = log_band(n, g["width"], switch_prob)
        assert (band >= np.log(TINY)).all()  # the exactness argument of the Viterbi kernel's band + maximum shortcut
        p_init = np.zeros(2 * n)
        p_init[n:] = 1 / n
        freqs = fmin * 2 ** (np.arange(n) / (12 * g["nbps"]))
        self.band, self.log_p_init = f64(band), f64(np.log(p_init + TINY))
        self.freqs = f64(np.concatenate([freqs, freqs]))
        self.log_tiny = float(np.log(TINY))
        T = self.T
        self.obs = torch.empty(B, T, n, dtype=torch.float64, device=dev)
        self.vp = torch.empty(B, T, dtype=torch.float64, device=dev)
        self.ptr = torch.empty(B, T, 2 * n, dtype=torch.int16, device=dev)
        self.states = torch.empty(B, T, dtype=torch.int32, device=dev)
        self.f0 = torch.empty(B, T, dtype=torch.float64, device=dev)
        self.flag = torch.empty(B, T, dtype=torch.uint8, device=dev)

        fill = fill_na is not None
        self._viterbi = ops.CallOp("srn_pyin_viterbi", (
            self.obs, self.vp, self.d_frames, self.band, self.log_p_init, self.freqs, self.log_tiny,
            float(fill_na) if fill else 0.0, int(fill), self.ptr, self.states, self.f0, self.flag, B, T, n, g["width"]))

    def observe(self, x, stream):
        g = self.g
        ops.CallOp("srn_pyin_observe", (
            x, x.stride(0), self.d_lens, self.d_frames, *self.tabs, self.obs, self.vp, self.B, self.N, self.T,
            self.frame_length, g["win_length"], g["hop_length"], self.pad, g["min_period"], g["max_period"],
            self.n_thresholds, self.sr, self.fmin, float(12 * g["nbps"]), g["n_bins"]))(stream)

    def viterbi(self, stream):
        self._viterbi(stream)


_PLANS = {}


def _plan(dev, B, N, lengths, key):
    return lru_get(_PLANS, (str(dev), B, N, lengths, key), 8, lambda: _PyinPlan(dev, B, N, lengths, key))


@torch.no_grad()
def pyin(wave, lengths=None, *, fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None,
         n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92,
         switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan, center=True, pad_mode="constant"):
    """librosa.pyin (0.10) of every item of wave (B, N) or (N,) float32 on the GPU, item b over its own lengths[b]
    samples.  Returns (f0, voiced_flag, voiced_prob, frames): (B, T) float64 / bool / float64 on the GPU ((T,) for a
    1-D wave) and frames (B,) int64 on the host; entries past frames[b] hold fill_na, False and 0."""
    if win_length is None:
        win_length = frame_length // 2
    if hop_length is None:
        hop_length = frame_length // 4
    _check(sr, fmin, fmax, frame_length, win_length, hop_length, n_thresholds, resolution, center, pad_mode,
           max_transition_rate)
    _require_cuda(wave)
    one = wave.ndim == 1
    x = wave.reshape(1, -1) if one else wave
    if x.stride(-1) != 1:
        x = x.contiguous()
    B, N = x.shape
    lengths = item_lengths(lengths, B, N, "pyin")
    fill = None if fill_na is None else float(fill_na)
    key = (sr, float(fmin), float(fmax), frame_length, win_length, hop_length, n_thresholds,
           tuple(beta_parameters), boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob,
           "nan" if fill is not None and math.isnan(fill) else fill, bool(center))  # NaN != NaN: keyed by name
    plan = _plan(x.device, B, N, lengths, key)
    plan.observe(x, None)
    plan.viterbi(None)
    f0, flag, vp = plan.f0.clone(), plan.flag.bool(), plan.vp.clone()
    if one:
        return f0[0], flag[0], vp[0], plan.frames.clone()
    return f0, flag, vp, plan.frames.clone()
