"""Waveform preparation on the GPU: what preprocessing does between the file on disk and the feature front-ends
(serenade/bin/preprocess.py:399-432) and the resampling of stage 9 (ssc_postprocessing.py:146), batched and ragged.

    resample(y, orig_sr, target_sr, lengths=None) -> (out, out_lengths)            librosa.resample's names
    trim(y, top_db=60, frame_length=2048, hop_length=512, lengths=None) -> (out, out_lengths, index (B, 2))
    pad_tail(y, pad, lengths=None) -> (out, out_lengths)                            np.pad(y, (0, pad), mode="reflect")
    prepare(audio, fs, config, lengths=None) -> (audio, lengths, audio16k, lengths16k)      preprocess.py:399-432

y is (B, N) or (N,), float32 or float64, a tensor or a numpy array (a host input is uploaded); item b has lengths[b]
samples and nothing past them is read.  The result has y's dtype and lives on the GPU, zero past each item's own
length.  A 1-D y gives what librosa gives: the array alone (with the (2,) index for trim).  Every item of a batch gets
bit for bit what its own B = 1 call gets; the arithmetic is fp64.  There is no CPU path.

Three HIP entry points (serenade_amd/csrc/audio.hip): srn_resample, srn_trim_bounds, srn_wave_window.

The resampler.  librosa's default is soxr_hq, which cannot be restated bit for bit; this one is defined by the
constants below, chosen after soxr-HQ's published targets: pass-band up to PASSBAND of the lower Nyquist, about
ATTENUATION_DB of rejection from that Nyquist on.  With g = gcd(orig, target), L = target / g, M = orig / g,
f_up = orig L, f_nyq = min(orig, target) / 2, f_pass = PASSBAND f_nyq, f_stop = f_nyq:

    beta = 0.1102 (ATTENUATION_DB - 8.7)        dw = 2 pi (f_stop - f_pass) / f_up
    N = ceil((ATTENUATION_DB - 7.95) / (2.285 dw))      half = (N + 1) // 2      fc = (f_pass + f_stop) / (2 f_up)
    h[n] = L 2 fc sinc(2 fc n) I0(beta sqrt(1 - (n / half)^2)) / I0(beta),  n = -half .. half
    y[m] = sum_j x[j] h[m M - j L]  over 0 <= j < len, |m M - j L| <= half, j ascending (zeros beyond both ends)
    n_out = int(ceil(len * (target / orig)))     librosa's float expression; equal rates are a copy

The host builds the taps in float64 and uploads them once per (device, rates).

Limits (ValueError before anything touches the device): integer rates; taps plus polyphase table of at most
MAX_TABLE_BYTES (24000 -> 23999 is refused); at most MAX_SPAN inputs under one tile of TILE outputs (SRN_RESAMPLE_* of
include/serenade_hip.h: downsampling by more than about 18 : 1 is refused); no empty item; pad_tail's pad below every
item's length (numpy's single reflection).

Parity: unpinned.  Neither librosa nor soxr is installed where this project is tested.  Recollection, not verified: the
trim rules (centred zero-padded frames as librosa 0.10's rms, amin, ref=np.max, the frames_to_samples bounds), the
n_out expression and the 0.913 / 120 dB targets; all are named below, once.  Against real soxr output this resampler
agrees as two near-ideal filters agree -- to about the design ripple inside the pass-band -- and not in the transition
band or within one filter length of the ends.  What is pinned: scipy.signal.resample_poly given the same taps, and the
analytic truth of band-limited signals (tests/test_audio_host.py, tests/test_hip_audio.py).
"""
import math

import numpy as np
import torch

from . import ops
from .plan import dev_f64, dev_i32, item_lengths, lru_get

__all__ = ["resample", "trim", "pad_tail", "prepare", "resample_geometry", "resample_taps", "resample_length",
           "trim_frames"]

# ---- the resampler's definition, one place
PASSBAND = 0.913  # of the lower Nyquist                                          recollection of soxr HQ
ATTENUATION_DB = 120.0  # stop-band rejection                                    recollection of soxr HQ
KAISER_BETA = (0.1102, 8.7)  # beta = a (att - b), Kaiser's formula for att > 50 dB
KAISER_ORDER = (7.95, 2.285)  # N = (att - a) / (b dw)
# ---- librosa.effects.trim / amplitude_to_db                                     recollection
TRIM_AMIN = 1e-5
# ---- the kernels' limits (SRN_RESAMPLE_* of serenade_hip.h)
TILE, MAX_SPAN = 256, 8192
MAX_TABLE_BYTES = 64 << 20
TARGET_16K = 16000  # the rate of ContentVec and the transcriber (preprocess.py:428-432)


def _rates(orig_sr, target_sr):
    out = []
    for name, v in (("orig_sr", orig_sr), ("target_sr", target_sr)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != int(v) or v <= 0:
            raise ValueError(f"resample: {name}={v!r} must be a positive integer rate")
        out.append(int(v))
    return out


def resample_geometry(orig_sr, target_sr):
    """(L, M, half) of the filter between two integer rates: up by L, down by M, taps -half .. half at orig_sr L"""
    orig, target = _rates(orig_sr, target_sr)
    g = math.gcd(orig, target)
    L, M = target // g, orig // g
    f_up = orig * L
    f_nyq = min(orig, target) / 2
    f_pass, f_stop = PASSBAND * f_nyq, f_nyq
    dw = 2 * math.pi * (f_stop - f_pass) / f_up
    n = math.ceil((ATTENUATION_DB - KAISER_ORDER[0]) / (KAISER_ORDER[1] * dw))
    return L, M, (n + 1) // 2


def _table_shape(L, half):
    """(K, q_lo) of the polyphase table: output m reads the inputs floor(m M / L) - q_lo + k, k < K"""
    q_lo, q_hi = half // L, (half + L - 1) // L
    return q_lo + q_hi + 1, q_lo


def _check_resample(orig_sr, target_sr):
    orig, target = _rates(orig_sr, target_sr)
    L, M, half = resample_geometry(orig, target)
    K, q_lo = _table_shape(L, half)
    table_bytes = (2 * half + 1 + K * L) * 8  # the taps and their polyphase arrangement, as the host builds them
    if table_bytes > MAX_TABLE_BYTES:
        raise ValueError(f"resample: {orig} -> {target} Hz needs a filter table of {table_bytes} bytes ({2 * half + 1} "
                         f"taps, {L} phases x {K}), above {MAX_TABLE_BYTES}")
    span = -(-(TILE - 1) * M // L) + K
    if span > MAX_SPAN:
        raise ValueError(f"resample: {orig} -> {target} Hz puts {span} inputs under one tile of {TILE} outputs, above "
                         f"{MAX_SPAN}")
    return orig, target, L, M, half, K, q_lo


def resample_taps(orig_sr, target_sr):
    """h[-half .. half] (float64, 2 half + 1 values, gain L) of the filter above"""
    orig, target, L, M, half, _, _ = _check_resample(orig_sr, target_sr)
    f_up = orig * L
    f_nyq = min(orig, target) / 2
    fc = (PASSBAND * f_nyq + f_nyq) / (2 * f_up)
    beta = KAISER_BETA[0] * (ATTENUATION_DB - KAISER_BETA[1])
    n = np.arange(-half, half + 1, dtype=np.float64)
    window = np.i0(beta * np.sqrt(np.maximum(1.0 - (n / half) ** 2, 0.0))) / np.i0(beta)
    return L * 2 * fc * np.sinc(2 * fc * n) * window


def resample_length(n, orig_sr, target_sr):
    """samples librosa.resample returns for n: int(np.ceil(n * (target_sr / orig_sr))), the float expression"""
    return int(np.ceil(n * (float(target_sr) / orig_sr)))


def trim_frames(n, hop_length):
    """frames of librosa's centred rms over n samples"""
    return 1 + n // hop_length


def polyphase_table(orig_sr, target_sr):
    """the taps as srn_resample reads them: (K, L) float64, table[k][p] = h[p - (k - q_lo) L], 0 beyond the filter"""
    L, M, half = resample_geometry(orig_sr, target_sr)
    K, q_lo = _table_shape(L, half)
    h = resample_taps(orig_sr, target_sr)
    arg = np.arange(L)[None, :] - (np.arange(K)[:, None] - q_lo) * L
    inside = np.abs(arg) <= half
    return np.where(inside, h[np.clip(arg + half, 0, 2 * half)], 0.0)


# ---------------------------------------------------------------------------------------------------- input
def _wave_batch(y, lengths, what, check=None):
    """(n,) or (B, n) float32 / float64 waveform(s), tensor or numpy -> ((B, n) contiguous tensor on the GPU, lengths,
    was 1-D).  A host input is uploaded to the current device; check(lengths) may raise before that happens."""
    if not isinstance(y, torch.Tensor):
        y = np.asarray(y)
        if y.dtype not in (np.float32, np.float64):
            raise ValueError(f"{what}: y must be float32 or float64, got {y.dtype}")
        y = torch.from_numpy(np.ascontiguousarray(y))
    a = y.detach()
    if a.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: y must be float32 or float64, got {a.dtype}")
    if a.dim() not in (1, 2) or min(a.shape) < 1:
        raise ValueError(f"{what}: y must be (n,) or (B, n) and not empty, got shape {tuple(a.shape)}")
    one = a.dim() == 1
    a = a.unsqueeze(0) if one else a
    lens = item_lengths(lengths, *a.shape, what)
    if check is not None:
        check(lens)
    if not a.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} needs a CUDA (ROCm) device; there is no CPU fallback")
        a = a.cuda()
    return a.contiguous(), lens, one


def _bs(a):
    """row stride of a contiguous (B, n) batch (the stride of a size-1 axis is arbitrary)"""
    return a.stride(0) if a.shape[0] > 1 else a.shape[1]


class _Window:
    """srn_wave_window over one (device, dtype, starts, counts, pad): the tables of a plan; x and out vary per call"""

    def __init__(self, dev, starts, counts, pad):
        self.B, self.pad, self.width = len(counts), int(pad), max(1, max(counts) + int(pad))
        self.d_starts, self.d_counts = dev_i32(starts, dev), dev_i32(counts, dev)

    def run(self, x, stream=None):
        out = torch.empty(self.B, self.width, dtype=x.dtype, device=x.device)
        ops.CallOp("srn_wave_window", (x, int(x.dtype == torch.float64), _bs(x), self.d_starts, self.d_counts,
                                       self.pad, out, self.width, self.B, self.width))(stream)
        return out


class _ResamplePlan:
    """the uploaded polyphase table of one (device, rates)"""

    def __init__(self, dev, orig, target):
        _, _, self.L, self.M, self.half, self.K, self.q_lo = _check_resample(orig, target)
        self.table = dev_f64(polyphase_table(orig, target), dev)


class _Lengths:
    """int32 device copies of one call shape's per-item counts"""

    def __init__(self, dev, *lists):
        self.d = [dev_i32(v, dev) for v in lists]


_TABLES, _LENGTHS, _WINDOWS, _TRIMS = {}, {}, {}, {}


def _window(dev, starts, counts, pad):
    key = (str(dev), tuple(starts), tuple(counts), int(pad))
    return lru_get(_WINDOWS, key, 16, lambda: _Window(dev, starts, counts, pad))


@torch.no_grad()
def resample(y, orig_sr, target_sr, lengths=None):
    """librosa.resample(y, orig_sr=, target_sr=) of every item of y over its own lengths[b] samples, by the filter of
    the module docstring.  Returns (out (B, max n_out), [n_out]) for a batch, out (n_out,) for a 1-D y."""
    orig, target = _rates(orig_sr, target_sr)
    if orig != target:
        _check_resample(orig, target)
    a, lens, one = _wave_batch(y, lengths, "resample")
    B, N = a.shape
    dev = a.device
    if orig == target:  # a copy of each item's own samples
        out, out_lens = _window(dev, (0,) * B, lens, 0).run(a), list(lens)
    else:
        out_lens = [resample_length(n, orig, target) for n in lens]
        plan = lru_get(_TABLES, (str(dev), orig, target), 8, lambda: _ResamplePlan(dev, orig, target))
        d = lru_get(_LENGTHS, (str(dev), lens, tuple(out_lens)), 16, lambda: _Lengths(dev, lens, out_lens)).d
        out = torch.empty(B, max(out_lens), dtype=a.dtype, device=dev)
        ops.CallOp("srn_resample", (a, int(a.dtype == torch.float64), _bs(a), d[0], d[1], plan.table, out,
                                    out.shape[1], B, N, out.shape[1], plan.L, plan.M, plan.K, plan.q_lo))()
    return out[0] if one else (out, out_lens)


class _TrimPlan:
    def __init__(self, dev, B, lens, hop):
        self.T = max(trim_frames(n, hop) for n in lens)
        self.d_lens = dev_i32(lens, dev)
        self.ms = torch.zeros(B, self.T, dtype=torch.float64, device=dev)
        self.bounds = torch.zeros(B, 2, dtype=torch.int32, device=dev)


def _check_trim(top_db, frame_length, hop_length):
    for name, v in (("frame_length", frame_length), ("hop_length", hop_length)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"trim: {name}={v!r} must be a positive integer")
    if not top_db == top_db or top_db < 0:
        raise ValueError(f"trim: top_db={top_db} must not be negative")


def _trim_index(a, lens, top_db, frame_length, hop_length):
    B = a.shape[0]
    plan = lru_get(_TRIMS, (str(a.device), lens, int(hop_length)), 8,
                   lambda: _TrimPlan(a.device, B, lens, int(hop_length)))
    ops.CallOp("srn_trim_bounds", (a, int(a.dtype == torch.float64), _bs(a), plan.d_lens, plan.ms, plan.bounds,
                                   B, max(lens), plan.T, int(frame_length), int(hop_length),
                                   float(10.0 ** (-float(top_db) / 10.0))))()
    return plan.bounds.cpu().numpy().astype(np.int64)


@torch.no_grad()
def trim_index(y, top_db=60, frame_length=2048, hop_length=512, lengths=None):
    """the index of librosa.effects.trim alone: (B, 2) numpy int64 [start, end) per item, (0, 0) where no frame lies
    above the threshold"""
    _check_trim(top_db, frame_length, hop_length)
    a, lens, _ = _wave_batch(y, lengths, "trim")
    return _trim_index(a, lens, top_db, frame_length, hop_length)


@torch.no_grad()
def trim(y, top_db=60, frame_length=2048, hop_length=512, lengths=None):
    """librosa.effects.trim of every item: (trimmed (B, max n), [n], index (B, 2) numpy) -- (trimmed, index (2,)) for
    a 1-D y, as librosa returns.  An item with nothing above the threshold comes back with length 0, which takes
    top_db <= 0: an item of exact zeros is kept whole, every frame and the reference level sitting at amin^2."""
    _check_trim(top_db, frame_length, hop_length)
    a, lens, one = _wave_batch(y, lengths, "trim")
    index = _trim_index(a, lens, top_db, frame_length, hop_length)
    counts = [int(e - s) for s, e in index]
    out = _window(a.device, [int(s) for s in index[:, 0]], counts, 0).run(a)
    if one:
        return out[0, :counts[0]], index[0]
    return out, counts, index


@torch.no_grad()
def pad_tail(y, pad, lengths=None):
    """np.pad(item, (0, pad), mode="reflect") of every item: (out (B, max n + pad), [n + pad]); out alone for 1-D"""
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 0:
        raise ValueError(f"pad_tail: pad={pad!r} must be a non-negative integer")

    def check(lens):
        if pad >= min(lens):
            raise ValueError(f"pad_tail: pad={pad} must be below every item's length (shortest {min(lens)}): a single "
                             "reflection does not reach further")

    a, lens, one = _wave_batch(y, lengths, "pad_tail", check)
    out = _window(a.device, (0,) * len(lens), lens, int(pad)).run(a)
    return out[0] if one else (out, [n + int(pad) for n in lens])


# ---------------------------------------------------------------------------------------------------- prepare
def _mono(item, what):
    """one utterance (n,) or (n, channels), as soundfile returns it -> (n,) tensor: the mean over channels
    (preprocess.py:399-400)"""
    t = item if isinstance(item, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(item)))
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: audio must be float32 or float64, got {t.dtype}")
    if t.dim() == 2:
        t = t.mean(dim=1) if t.shape[1] > 1 else t[:, 0]
    if t.dim() != 1 or t.shape[0] < 1:
        raise ValueError(f"{what}: an utterance must be (n,) or (n, channels) and not empty, got {tuple(item.shape)}")
    return t


@torch.no_grad()
def prepare(audio, fs, config, lengths=None):
    """preprocess.py:399-432 for a whole batch: mono mean, the |x| <= 1 check, resampling to
    config["sampling_rate"] where an item's fs differs, librosa.effects.trim if config["trim_silence"] (with
    trim_threshold_in_db / trim_frame_size / trim_hop_size), the reflect pad by config["fft_size"], and the 16 kHz
    copy for ContentVec and the transcriber.

    audio: a list of utterances, each (n,) or (n, channels) as soundfile returns them, or a padded batch (B, N) /
    (B, N, channels) with `lengths`.  fs: one rate for all, or one per item.  Returns (audio (B, N') at
    config["sampling_rate"], its lengths, audio16k (B, N16), its lengths): padded batches on the GPU in the input's
    dtype (float64 as soon as one item is), zero past each item's length."""
    what = "prepare"
    if isinstance(audio, (list, tuple)):
        if lengths is not None:
            raise ValueError(f"{what}: lengths go with a padded batch, not with a list of utterances")
        items = [_mono(v, what) for v in audio]
    else:
        t = audio if isinstance(audio, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(audio)))
        if t.dim() not in (2, 3):
            raise ValueError(f"{what}: a padded batch must be (B, N) or (B, N, channels), got {tuple(t.shape)}")
        lens = item_lengths(lengths, t.shape[0], t.shape[1], what)
        items = [_mono(t[b, :n], what) for b, n in enumerate(lens)]
    B = len(items)
    if B < 1:
        raise ValueError(f"{what}: no utterance")
    rates = [fs] * B if isinstance(fs, (int, float, np.integer, np.floating)) else list(fs)
    if len(rates) != B:
        raise ValueError(f"{what}: fs must be one rate or one per item ({B}), got {len(rates)}")
    sr = _rates(config["sampling_rate"], TARGET_16K)[0]
    rates = [_rates(r, sr)[0] for r in rates]
    for r in sorted(set(rates)):
        if r != sr:
            _check_resample(r, sr)
    if sr != TARGET_16K:
        _check_resample(sr, TARGET_16K)
    fft_size = int(config["fft_size"])
    for b, v in enumerate(items):
        peak = float(v.abs().max())
        if not peak <= 1.0:
            raise ValueError(f"{what}: item {b} peaks at {peak}: it seems to be different from 16 bit PCM")
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs a CUDA (ROCm) device; there is no CPU fallback")
    dtype = torch.float64 if any(v.dtype == torch.float64 for v in items) else torch.float32
    dev = next((v.device for v in items if v.is_cuda), torch.device("cuda", torch.cuda.current_device()))

    def batch(waves):
        x = torch.zeros(len(waves), max(len(w) for w in waves), dtype=dtype, device=dev)
        for i, w in enumerate(waves):
            x[i, :len(w)] = w.to(device=dev, dtype=dtype)
        return x

    x, lens = batch(items), [len(v) for v in items]
    if any(r != sr for r in rates):
        done = [None] * B
        for r in sorted(set(rates)):
            idx = [b for b in range(B) if rates[b] == r]
            sub, sub_lens = resample(batch([x[b, :lens[b]] for b in idx]), r, sr, [lens[b] for b in idx])
            for i, b in enumerate(idx):
                done[b] = sub[i, :sub_lens[i]]
        x, lens = batch(done), [len(v) for v in done]
    if config["trim_silence"]:
        x, lens, _ = trim(x, top_db=config["trim_threshold_in_db"], frame_length=config["trim_frame_size"],
                          hop_length=config["trim_hop_size"], lengths=lens)
        if min(lens) < 1:
            raise ValueError(f"{what}: item {lens.index(min(lens))} is silent throughout: nothing is left of it")
    x, lens = pad_tail(x, fft_size, lens)
    x16, lens16 = resample(x, sr, TARGET_16K, lens)
    return x, lens, x16, lens16
