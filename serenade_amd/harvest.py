"""WORLD Harvest F0 estimation on the GPU: `pyworld.harvest`, batched and ragged.  The reference runs it on the host
for every utterance of preprocessing (serenade/bin/preprocess.py:485-493) and writes the result to the dump as `f0`;
that track is the `lf0` of the decode loop and, shifted, the F0 of stage 9's CheapTrick, D4C and SiFiGAN excitation.

    harvest(x, fs, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0, lengths=None) -> (f0, t)     pyworld's names
    extract_f0(audio, sampling_rate, minf0, maxf0, shiftms) -> (f0 (T, 1) float64, vuv (T, 1) float32)

x is (B, N) or (N,), float32 or float64, on the GPU; item b has lengths[b] samples and nothing past them is used.
f0 is (B, F) float64 on the GPU ((F,) for a 1-D x), F = max_b harvest_frame_count(lengths[b], fs, frame_period); entries
past an item's frames and unvoiced frames are 0.  t is the time axis of the longest item (float64 numpy, seconds).
f0_floor / f0_ceil may be per-item sequences: items are grouped by value on the host and the groups run in turn.  Every
item gets exactly what its own B = 1 call gets.  There is no CPU path.

Five HIP entry points (serenade_amd/csrc/harvest.hip), in this order: srn_harvest_decimate (zero-phase Chebyshev
decimation to about 8 kHz, mean removal), srn_harvest_channels (one workgroup per (item, channel): band-pass, four
kinds of zero-crossing events, the channel's raw candidate at every 1 ms frame), srn_harvest_candidates (runs of >= 10
channels, +-3 frames of overlap), srn_harvest_refine (instantaneous-frequency refinement and score of every candidate)
and srn_harvest_contour (removal of unreliable candidates, FixStep1-4, smoothing, the pick at frame_period).  Everything
data-independent (band-pass taps, decimation and smoothing coefficients) is built here with numpy / scipy.

Limits (checked before anything touches the device; SRN_HARVEST_* of include/serenade_hip.h): the longest band-pass,
2 matlab_round(2 actual_fs / (0.9 f0_floor 2^(1/40))) + 1 taps, at most MAX_TAPS = 1024 (f0_floor >= about 35 Hz at
8 kHz); the refinement window 2 int(1.5 actual_fs / f0_floor + 1) + 1 at most MAX_WINDOW = 1536 samples; at most
MAX_CAND = 256 candidates per frame.  Workspace: every buffer is allocated by the plan, WORKSPACE_BUDGET bytes at the
most per launch sequence; a batch that needs more runs in chunks of items, and the event scratch of the channel kernel
(sized by the provable bound of len / 2 events per kind) is bounded by EVENT_BUDGET by launching ranges of channels.

Parity: tests/_harvest_ref.py (a float64 numpy + scipy restatement written from recollection of harvest.cpp) is the pin;
pyworld is not installed where this project is tested ("parity unpinned", like pitch.py).  All constants below are
recollection except the two filters, which were checked against scipy.
"""
import math

import numpy as np
import scipy.signal
import torch

from . import ops
from .plan import dev_f64, dev_i32, item_lengths, lru_get

__all__ = ["harvest", "extract_f0", "harvest_geometry", "harvest_frames", "harvest_pick", "decimation_table",
           "smoothing_table", "channel_taps"]

# ---- WORLD's constants (harvest.cpp), one place.  Verified against scipy: the two filters.  The rest: recollection.
CHANNELS_IN_OCTAVE = 40.0
FLOOR_FACTOR, CEIL_FACTOR = 0.9, 1.1
TARGET_FS = 8000.0
DECIMATE_LAG_SAMPLES = 140.0
DECIMATE_FILTER = (3, 0.05, 0.8)  # cheby1(order, ripple dB, cutoff / ratio)      verified
SMOOTH_FILTER = (2, 0.06)  # butter(order, cutoff)                                verified
NUTTALL = (0.355768, 0.487396, 0.144232, 0.012604)
FILTER_PERIODS = 2.0
OVERLAP_FRAMES = 3
REFINE_WINDOW_PERIODS = 1.5
# ---- the kernels' limits (SRN_HARVEST_* of serenade_hip.h)
MAX_TAPS, MAX_WINDOW, MAX_CAND, MAX_RATIO, SMOOTH_PAD = 1024, 1536, 256, 12, 300
WORKSPACE_BUDGET = 1 << 30  # bytes of plan buffers per launch sequence; larger batches run in chunks of items
EVENT_BUDGET = 1 << 28  # bytes of event scratch per srn_harvest_channels launch; more channels take more launches


def matlab_round(x):
    return int(x + 0.5) if x > 0 else int(x - 0.5)


def harvest_geometry(fs, f0_floor=71.0, f0_ceil=800.0):
    """the derived sizes of one harvest call: decimation ratio, analysis rate, channels, candidates per frame"""
    ratio = max(min(matlab_round(fs / TARGET_FS), MAX_RATIO), 1)
    actual_fs = fs / ratio
    lo, hi = f0_floor * FLOOR_FACTOR, f0_ceil * CEIL_FACTOR
    n_ch = 1 + int(math.log2(hi / lo) * CHANNELS_IN_OCTAVE)
    boundary = np.array([lo * 2.0 ** ((i + 1) / CHANNELS_IN_OCTAVE) for i in range(n_ch)])
    n_base = matlab_round(n_ch / 10.0)
    return dict(ratio=ratio, actual_fs=actual_fs, n_ch=n_ch, boundary=boundary, n_base=n_base,
                n_cand=n_base * (2 * OVERLAP_FRAMES + 1),
                half_len=[matlab_round(actual_fs / b * FILTER_PERIODS) for b in boundary],
                lag=int(math.ceil(DECIMATE_LAG_SAMPLES / ratio) * ratio),
                voice_range_minimum=int(0.5 + 1000.0 / f0_floor) * 2 + 1,
                max_window=2 * int(REFINE_WINDOW_PERIODS * actual_fs / f0_floor + 1.0) + 1)


def harvest_frames(x_length, fs, frame_period=5.0):
    """frames pyworld.harvest returns (WORLD GetSamplesForHarvest); the body itself always runs at frame_period 1.
    Stage 9 (world.py, as `harvest_frame_count`) keeps nothing else of Harvest."""
    return int(1000.0 * x_length / fs / frame_period) + 1


def harvest_pick(n_out, n_internal, frame_period):
    """the 1 ms frame each requested frame is taken from: min(F1 - 1, matlab_round(1000 t_i))"""
    t = np.arange(n_out) * frame_period / 1000.0
    return np.array([min(n_internal - 1, matlab_round(v * 1000.0)) for v in t], dtype=np.int64)


def decimation_table(ratio):
    """(b, a) of the decimation low-pass: order-3 Chebyshev I, 0.05 dB, 0.8 / ratio"""
    order, ripple, cutoff = DECIMATE_FILTER
    return scipy.signal.cheby1(order, ripple, cutoff / ratio)


def smoothing_table():
    """(b, a) of SmoothF0Contour: order-2 Butterworth at 0.06"""
    return scipy.signal.butter(*SMOOTH_FILTER)


def nuttall_window(n):
    """WORLD's NuttallWindow of n samples (float64): the band-passes here, D4C's band window in world.py"""
    t = np.arange(n) / (n - 1.0)
    a = NUTTALL
    return a[0] - a[1] * np.cos(2.0 * np.pi * t) + a[2] * np.cos(4.0 * np.pi * t) - a[3] * np.cos(6.0 * np.pi * t)


def channel_taps(boundary_f0, actual_fs):
    """a channel's band-pass: Nuttall window of 2 hl + 1 samples x cosine at boundary_f0, hl = round(2 fs / f0)"""
    hl = matlab_round(actual_fs / boundary_f0 * FILTER_PERIODS)
    return nuttall_window(2 * hl + 1) * np.cos(2.0 * np.pi * boundary_f0 * np.arange(-hl, hl + 1) / actual_fs)


def _check(fs, f0_floor, f0_ceil, frame_period):
    """pyworld's argument rules, then the limits of the kernels; raises ValueError before anything touches the device"""
    if not fs > 0:
        raise ValueError(f"harvest: fs={fs} must be positive")
    if not 0 < f0_floor < f0_ceil:
        raise ValueError(f"harvest: need 0 < f0_floor={f0_floor} < f0_ceil={f0_ceil}")
    if not frame_period > 0:
        raise ValueError(f"harvest: frame_period={frame_period} must be positive")
    g = harvest_geometry(fs, f0_floor, f0_ceil)
    if not f0_ceil * CEIL_FACTOR < fs / (2 * g["ratio"]):
        raise ValueError(f"harvest: f0_ceil={f0_ceil} x {CEIL_FACTOR} must lie below the analysis Nyquist "
                         f"{fs / (2 * g['ratio'])} Hz (fs {fs} decimated by {g['ratio']})")
    taps = 2 * max(g["half_len"]) + 1
    if taps > MAX_TAPS or g["max_window"] > MAX_WINDOW or g["n_cand"] > MAX_CAND or g["n_ch"] < 3:
        raise ValueError(f"harvest: outside the kernels' limits (longest band-pass {taps} <= {MAX_TAPS} taps, "
                         f"refinement window {g['max_window']} <= {MAX_WINDOW} samples, {g['n_cand']} <= {MAX_CAND} "
                         f"candidates per frame, {g['n_ch']} >= 3 channels): raise f0_floor or narrow the range")
    return g


def _sizes(g, lengths, fs):
    """section capacity, pool stride, and the plan's bytes per item (buffers are sized by the longest of the items)"""
    N = max(lengths)
    F1 = max(harvest_frames(n, fs, 1.0) for n in lengths)
    ylen = -(-max(lengths) // g["ratio"])
    sec_cap = F1 // min(g["voice_range_minimum"] + 2, 10) + 4
    pool = F1 + 2 * SMOOTH_PAD * sec_cap
    per_item = 8 * ((N + 2 * g["lag"] + 18) + ylen + g["n_ch"] * F1 + g["n_base"] * F1 + 5 * g["n_cand"] * F1 + 7 * F1
                    + pool) + 4 * 7 * sec_cap
    return F1, ylen, sec_cap, pool, per_item


def _require_cuda(x):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
        raise RuntimeError("harvest: x must be a float32 or float64 CUDA (ROCm) tensor; there is no CPU path")


class _HarvestPlan:
    """tables, buffers and prebuilt ops of one (device, B, N, lengths, parameters) call; the five steps are methods so
    that the tests and tools/harvestbench.py can run and time them one by one (each reads the buffers the previous one
    wrote).  Only the decimation reads the caller's x, so only its op is built per call."""

    def __init__(self, dev, B, N, lengths, key):
        fs, f0_floor, f0_ceil, frame_period, is_f64 = key
        N = max(lengths)  # every buffer is sized by the longest of the plan's own items, not by the padded width of x
        g = self.g = harvest_geometry(fs, f0_floor, f0_ceil)
        self.B, self.N, self.fs, self.f0_floor, self.f0_ceil = B, N, float(fs), float(f0_floor), float(f0_ceil)
        self.frame_period, self.is_f64 = float(frame_period), int(is_f64)
        self.frames = [harvest_frames(n, fs, 1.0) for n in lengths]
        self.out_frames = [harvest_frames(n, fs, frame_period) for n in lengths]
        self.ylens = [-(-n // g["ratio"]) for n in lengths]
        self.F1, self.ylen, self.sec_cap, self.pool_stride, _ = _sizes(g, lengths, fs)
        self.F = max(self.out_frames)
        i32, f64 = (lambda a: dev_i32(a, dev)), (lambda a: dev_f64(a, dev))
        z64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        self.d_lens, self.d_ylens = i32(lengths), i32(self.ylens)
        self.d_frames, self.d_out_frames = i32(self.frames), i32(self.out_frames)
        taps = [channel_taps(b, g["actual_fs"]) for b in g["boundary"]]
        self.taps = f64(np.concatenate(taps))
        self.tap_off = i32(np.concatenate([[0], np.cumsum([len(t) for t in taps])[:-1]]))
        self.half_len, self.boundary = i32(g["half_len"]), f64(g["boundary"])
        self.dec_coef = f64(np.concatenate(decimation_table(g["ratio"])))
        self.smooth_coef = f64(np.concatenate(smoothing_table()))
        F1, C = self.F1, g["n_cand"]
        self.ws_stride = N + 2 * g["lag"] + 18
        self.ws = z64(B, self.ws_stride) if g["ratio"] > 1 else None
        self.y = z64(B, self.ylen)
        self.ev_cap = max(1, self.ylen // 2)
        self.ch_chunk = max(1, min(g["n_ch"], EVENT_BUDGET // (B * 4 * self.ev_cap * 8)))
        self.events = z64(B * self.ch_chunk * 4 * self.ev_cap)
        self.raw = z64(B, g["n_ch"], F1)
        self.official = z64(B, F1, g["n_base"])
        self.cand, self.refined, self.score = z64(B, F1, C), z64(B, F1, C), z64(B, F1, C)
        self.cand2, self.score2 = z64(B, F1, C), z64(B, F1, C)
        self.fbuf = z64(B, 6, F1)
        self.pool = z64(B, self.pool_stride)
        self.sections = torch.zeros(B, 7, self.sec_cap, dtype=torch.int32, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.f0 = z64(B, self.F)

        n_ch, fs_a, call = g["n_ch"], g["actual_fs"], ops.CallOp
        self._channels = [call("srn_harvest_channels", (
            self.y, self.y.stride(0), self.d_ylens, self.d_frames, self.taps, self.tap_off, self.half_len,
            self.boundary, max(g["half_len"]), self.events, self.ev_cap, self.raw, B, ch0,
            min(self.ch_chunk, n_ch - ch0), n_ch, F1, self.ylen, fs_a, self.f0_floor, self.f0_ceil))
            for ch0 in range(0, n_ch, self.ch_chunk)]
        self._candidates = call("srn_harvest_candidates", (
            self.raw, self.d_frames, self.official, self.cand, B, n_ch, F1, g["n_base"]))
        self._refine = call("srn_harvest_refine", (
            self.y, self.y.stride(0), self.d_ylens, self.d_frames, self.cand, self.refined, self.score, B, F1, C, fs_a,
            self.f0_floor, self.f0_ceil))
        self._contour = call("srn_harvest_contour", (
            self.refined, self.score, self.d_frames, self.d_out_frames, self.smooth_coef, self.cand2, self.score2,
            self.fbuf, self.pool, self.pool_stride, self.sections, self.sec_cap, self.status, self.f0,
            self.f0.stride(0), B, F1, C, self.F, g["voice_range_minimum"], self.frame_period))

    def decimate(self, x, stream):
        g = self.g
        ops.CallOp("srn_harvest_decimate", (
            x, self.is_f64, x.stride(0), self.d_lens, self.dec_coef, self.ws, self.ws_stride, self.y, self.y.stride(0),
            self.B, self.N, g["ratio"], g["lag"]))(stream)

    def channels(self, stream):
        for op in self._channels:
            op(stream)

    def candidates(self, stream):
        self._candidates(stream)

    def refine(self, stream):
        self._refine(stream)

    def contour(self, stream):
        self._contour(stream)

    def run(self, x, stream=None):
        self.decimate(x, stream)
        self.channels(stream)
        self.candidates(stream)
        self.refine(stream)
        self.contour(stream)
        if int(self.status.max().item()) != 0:  # cannot happen within the stated capacities; never silently wrong
            raise RuntimeError("harvest: an item has more voiced sections than the contour workspace holds")
        return self.f0

    # the 1 ms contours of the last contour() call, for tests: before and after smoothing
    @property
    def unsmoothed(self):
        return self.fbuf[:, 3]

    @property
    def smoothed(self):
        return self.fbuf[:, 4]


_PLANS = {}


def _plan(dev, B, N, lengths, key):
    return lru_get(_PLANS, (str(dev), B, N, lengths, key), 8, lambda: _HarvestPlan(dev, B, N, lengths, key))


def _per_item(v, B, name):
    if isinstance(v, (int, float)):
        return [float(v)] * B
    v = [float(a) for a in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != B:
        raise ValueError(f"harvest: {name} must be a scalar or give one value per item ({B}), got {len(v)}")
    return v


@torch.no_grad()
def harvest(x, fs, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0, lengths=None):
    """pyworld.harvest of every item of x (B, N) or (N,) float32 / float64 on the GPU, item b over its own lengths[b]
    samples.  Returns (f0, t): f0 (B, F) float64 on the GPU ((F,) for a 1-D x), 0 on unvoiced frames and past an item's
    frames; t the time axis of the longest item (numpy float64, seconds)."""
    shape = tuple(getattr(x, "shape", ()))
    if len(shape) not in (1, 2) or min(shape, default=0) < 1:
        raise ValueError(f"harvest: x must be (B, N) or (N,) and not empty, got shape {shape}")
    B, N = (1, shape[0]) if len(shape) == 1 else shape
    floors, ceils = _per_item(f0_floor, B, "f0_floor"), _per_item(f0_ceil, B, "f0_ceil")
    for pair in sorted(set(zip(floors, ceils))):
        _check(fs, pair[0], pair[1], frame_period)
    lengths = item_lengths(lengths, B, N, "harvest")
    _require_cuda(x)
    one = x.ndim == 1
    xb = x.reshape(1, -1) if one else x
    if xb.stride(-1) != 1:
        xb = xb.contiguous()
    F = max(harvest_frames(n, fs, frame_period) for n in lengths)
    out = torch.zeros(B, F, dtype=torch.float64, device=x.device)
    groups = {}
    for b in range(B):
        groups.setdefault((floors[b], ceils[b]), []).append(b)
    for (lo, hi), items in groups.items():
        g = harvest_geometry(fs, lo, hi)
        per_item = _sizes(g, [lengths[b] for b in items], fs)[4]
        step = max(1, WORKSPACE_BUDGET // per_item)
        for i0 in range(0, len(items), step):
            idx = items[i0:i0 + step]
            xs = xb[idx[0]:idx[-1] + 1] if idx == list(range(idx[0], idx[-1] + 1)) else xb[idx]
            lens = tuple(lengths[b] for b in idx)
            key = (float(fs), lo, hi, float(frame_period), x.dtype == torch.float64)
            f0 = _plan(x.device, len(idx), N, lens, key).run(xs)
            out[idx, :f0.shape[1]] = f0
    t = np.arange(F) * frame_period / 1000.0
    return (out[0] if one else out), t


@torch.no_grad()
def extract_f0(audio, sampling_rate, minf0, maxf0, shiftms, lengths=None):
    """what preprocess.py:485-493 writes to the dump: (f0[:, None] float64 (T, 1), vuv = (f0 != 0) float32 (T, 1)),
    T = int(1000 n / sampling_rate / shiftms) + 1; a list of such pairs, each cut to its own T, for a (B, N) batch"""
    f0, _ = harvest(audio, sampling_rate, f0_floor=minf0, f0_ceil=maxf0, frame_period=shiftms, lengths=lengths)
    if f0.ndim == 1:
        f0 = f0[:, None].clone()
        return f0, (f0 != 0).to(torch.float32)
    out = []
    for b, n in enumerate(item_lengths(lengths, *audio.shape, "harvest")):
        v = f0[b, :harvest_frames(n, sampling_rate, shiftms), None].clone()
        out.append((v, (v != 0).to(torch.float32)))
    return out
