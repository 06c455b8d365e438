"""Inputs shared by the note decoder's tests (tests/test_notes_host.py on the CPU, tests/test_hip_notes.py on the GPU):
random logits on the grid k / 16 with |x| <= 8 -- distinct grid values differ by at least 2e-5 after the sigmoid, far
above an fp32 ulp, and equal values tie on every implementation -- thresholds at least 1e-4 from every sigmoid value of
that grid, and contours whose float64 pitch keeps 1e-3 away from every half-integer."""
import numpy as np

GRID = np.arange(-128, 129) / 16.0
SIGMOID = 1.0 / (1.0 + np.exp(-GRID))  # float64: the guard band below is 1e-4 against an fp32 error of 6e-8
THRESHOLDS = (0.5 + 2e-3, 0.3, 0.725)  # 0.5 itself is sigmoid(0): the decoder's own default lies ON the grid
MODES = ("median", "weighted_mean", "weighted_median")


def guard_banded(threshold):
    return float(np.abs(SIGMOID - threshold).min()) >= 1e-4


def curves(n, seed, smooth=6, ties=True):
    """(n, 3) float32 logits on the grid: smoothed noise, so that runs, peaks and dips of realistic lengths appear;
    coarse steps (ties=True) make equal neighbours common"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n + smooth, 3))
    k = np.ones(smooth) / np.sqrt(smooth)
    y = np.stack([np.convolve(x[:, c], k, mode="valid")[:n] for c in range(3)], axis=1) * 3.0
    step = 8 if ties else 1  # multiples of 1 / 2 or of 1 / 16
    return (np.clip(np.round(y * 16 / step) * step, -128, 128) / 16.0).astype(np.float32)


def contour(n, seed, nan_rate=0.25):
    """(n,) float64 Hz with NaN stretches; every value is fp32-representable and its pitch is 1e-3 clear of k + 0.5"""
    rng = np.random.default_rng(seed)
    midi = 48 + 24 * rng.random(n)
    frac = midi - np.floor(midi)
    midi = np.where(np.abs(frac - 0.5) < 0.01, midi + 0.02, midi)
    f = (440.0 * 2.0 ** ((midi - 69) / 12)).astype(np.float32).astype(np.float64)
    gaps = np.convolve(rng.random(n + 4), np.ones(5) / 5, mode="valid")[:n] < nan_rate * 1.6
    return np.where(gaps, np.nan, f)


def clear_of_half(pitches, band=1e-3):
    p = np.asarray(pitches, dtype=np.float64)
    p = p[p != 0]
    return bool((np.abs(p - np.floor(p) - 0.5) >= band).all())
