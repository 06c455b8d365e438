"""Float64 numpy restatement of the three kernels of serenade_amd/csrc/audio.hip, written from the specification in
DESIGN.md 7e (not from the kernels): every sum a plain dot product.  Shared by tests/test_audio_host.py (CPU) and
tests/test_hip_audio.py (GPU); the signals both files use are built here, once."""
import functools
import math

import numpy as np

# ---- the resampler's definition, stated again on purpose
PASSBAND, ATT = 0.913, 120.0
AMIN = 1e-5
NEAR_TIE = 1e-9


def geometry(orig, target):
    g = math.gcd(orig, target)
    L, M = target // g, orig // g
    f_up = orig * L
    f_nyq = min(orig, target) / 2
    f_pass, f_stop = PASSBAND * f_nyq, f_nyq
    dw = 2 * np.pi * (f_stop - f_pass) / f_up
    N = int(np.ceil((ATT - 7.95) / (2.285 * dw)))
    half = (N + 1) // 2
    return L, M, half, (f_pass + f_stop) / (2 * f_up)


@functools.lru_cache(maxsize=None)
def taps(orig, target):
    L, M, half, fc = geometry(orig, target)
    beta = 0.1102 * (ATT - 8.7)
    n = np.arange(-half, half + 1)
    h = L * 2 * fc * np.sinc(2 * fc * n) * np.i0(beta * np.sqrt(1 - (n / half) ** 2)) / np.i0(beta)
    h.setflags(write=False)
    return h


def out_length(n, orig, target):
    return int(np.ceil(n * (target / orig)))


def resample(x, orig, target):
    """y[m] = sum_j x[j] h[m M - j L] over 0 <= j < len, |m M - j L| <= half"""
    x = np.asarray(x, dtype=np.float64)
    if orig == target:
        return x.copy()
    L, M, half, _ = geometry(orig, target)
    h = taps(orig, target)
    y = np.zeros(out_length(len(x), orig, target))
    for m in range(len(y)):
        lo = max(0, -((half - m * M) // L))  # ceil((m M - half) / L)
        hi = min(len(x) - 1, (m * M + half) // L)
        if hi >= lo:
            j = np.arange(lo, hi + 1)
            y[m] = np.dot(x[j], h[m * M - j * L + half])
    return y


def trim(x, top_db=60, frame_length=2048, hop=512):
    """((start, end), near-tie frames): the decisions of librosa.effects.trim in the power domain"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    padded = np.concatenate([np.zeros(frame_length // 2), x, np.zeros(frame_length // 2)])
    frames = 1 + n // hop
    ms = np.zeros(frames)
    for t in range(frames):
        f = padded[t * hop:t * hop + frame_length]
        ms[t] = np.dot(f, f) / frame_length
    level = np.maximum(AMIN ** 2, ms)
    threshold = 10.0 ** (-top_db / 10.0) * max(AMIN ** 2, ms.max())
    near = np.flatnonzero(np.abs(level / threshold - 1.0) <= NEAR_TIE)
    loud = np.flatnonzero(level > threshold)
    if len(loud) == 0:
        return (0, 0), near
    return (int(loud[0]) * hop, min(n, (int(loud[-1]) + 1) * hop)), near


def window(x, start, n, pad, width=None):
    """out[i] = x[start + i] (i < n), x[start + n - 2 - (i - n)] for the next pad samples, then zeros"""
    x = np.asarray(x)
    width = n + pad if width is None else width
    out = np.zeros(width, dtype=x.dtype)
    for i in range(min(width, n + pad)):
        out[i] = x[start + i] if i < n else x[start + n - 2 - (i - n)]
    return out


# ---------------------------------------------------------------------------------------------------- signals
def sines(sr, orig, target, seconds=0.25):
    """the band-limited test signal at rate sr: 110 Hz and 0.31 / 0.62 / 0.90 of the lower Nyquist of the pair, amplitudes
    1, 1/2, 1/3, 1/4, phases 0.3 k; `seconds` of the ORIGINAL grid, evaluated on the grid of rate sr"""
    nyq = min(orig, target) / 2
    n = int(round(seconds * orig)) if sr == orig else out_length(int(round(seconds * orig)), orig, target)
    t = np.arange(n) / sr
    return sum(np.sin(2 * np.pi * f * t + 0.3 * k) / (k + 1)
               for k, f in enumerate((110.0, 0.31 * nyq, 0.62 * nyq, 0.90 * nyq)))


def edge(orig, target):
    """output samples at each end that the zero extension reaches"""
    L, M, half, _ = geometry(orig, target)
    return int(np.ceil(half * target / (orig * L))) + 2


def truth_error(y, orig, target):
    e = edge(orig, target)
    return float(np.abs(np.asarray(y, np.float64) - sines(target, orig, target))[e:-e].max())


def stopband_tone(orig, target, seconds=0.25):
    return np.sin(2 * np.pi * 1.05 * (target / 2) * np.arange(int(round(seconds * orig))) / orig)


def stopband_level(y, orig, target):
    e = edge(orig, target)
    return float(np.abs(np.asarray(y, np.float64))[e:-e].max())


@functools.lru_cache(maxsize=None)
def trim_signals(sr=24000):
    """name -> (signal float64, by-hand (start, end) at frame_length 2048 / hop 512 or None)"""
    rng = np.random.default_rng(5)
    tone = 0.5 * np.sin(2 * np.pi * 220.0 * np.arange(5000) / sr)
    lead, tail = 3333, 4100  # not on hop multiples
    out = {
        "zeros_tone_zeros": np.concatenate([np.zeros(lead), tone, np.zeros(tail)]),
        "floor_tone_floor": np.concatenate([1e-5 * rng.standard_normal(lead), tone, 1e-5 * rng.standard_normal(tail)]),
        "silent": np.zeros(6000),
        "loud": 0.5 * np.sin(2 * np.pi * 220.0 * np.arange(7001) / sr),
        "short": 0.3 * np.sin(2 * np.pi * 220.0 * np.arange(300) / sr + 1.0),
    }
    for v in out.values():
        v.setflags(write=False)
    return out
