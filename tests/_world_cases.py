"""TEST-ONLY: the edge cases of the WORLD analysis kernels (csrc/world.hip: CheapTrick, D4C, the sp2mc projection, the
feature packer, the PCM16 widening, the two F0-contour kernels, the SiFiGAN excitation), shared by the CPU test that
proves the cases fit to be judged (tests/test_world_cases_host.py) and the run on the GPU
(tests/test_hip_world_sweep.py): same signals, same reference, same bounds.

Reference: oracle/world_oracle.py (numpy float64).  Bounds: 1e-6 on the log of the envelope, on the mel-cepstrum and
on the band aperiodicity in dB (the bounds tests/test_world.py holds the same kernels to, and its comment at the
CheapTrick bound says why float64 on both sides does not give 1e-12); everything that is pinned arithmetic (contours,
dilated factors, the packer, the widening, the unvoiced constant) bit for bit.

A bound of 1e-6 on a quantity that differences running sums only judges the kernel if the quantity itself is well
conditioned on the input at hand, and a threshold decision can only be asserted off the threshold.  Both are
CONDITIONS ON THE INPUTS, asserted on the CPU by the host test and never excused:
  * conditioning: the oracle's own output moves by less than MOVE when every sample is multiplied by 1 + 1e-15 randn;
  * Love-Train margin: |share - 0.85| >= MARGIN on every frame whose voiced / unvoiced decision is asserted.
Each reference is computed once per process and never written to.
"""
import functools

import numpy as np
import torch

from oracle import world_oracle as W
from serenade_amd import world
from tests.test_world import _allpole  # the fixed all-pole filter (formants at 700 / 1800 / 3200 Hz of 24 kHz)

FS = 24000
ORDER = 39
UNVOICED = 20 * np.log10(1.0 - 1e-12)
TOL = 1e-6       # log envelope, mel-cepstrum, dB
MOVE = 1e-8      # what the oracle may move under the perturbation, same units
MARGIN = 0.01    # distance of the Love-Train share from its threshold
THRESHOLD = 0.85
SINE_TOL = 2e-7  # the bound of the excitation in tests/test_world.py
HOP = 120


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ signals
@functools.lru_cache(maxsize=None)
def pulses(fs, f0, seconds, noise=1e-3, seed=0):
    """tests/test_world.py's voiced_signal at any (fs, f0): a pulse train through the fixed all-pole filter, normalised,
    plus white noise.  Pulse positions at or past the end (arange's last step can round up to n) are dropped."""
    from scipy.signal import lfilter
    n = int(fs * seconds + 0.5)
    x = np.zeros(n)
    idx = np.arange(0, n, fs / f0).astype(int)
    x[idx[idx < n]] = 1.0
    y = lfilter([1.0], _allpole(), x)
    y /= np.abs(y).max()
    if noise:
        y = y + noise * np.random.default_rng(seed).standard_normal(n)
    return _frozen(y)


@functools.lru_cache(maxsize=None)
def noise(n, seed):
    return _frozen(0.3 * np.random.default_rng(seed).standard_normal(n))


@functools.lru_cache(maxsize=None)
def silence(n):
    return _frozen(np.zeros(n))


def perturbed(x, seed=99):
    """the input of the conditioning check: every sample moved by about one part in 1e15"""
    return x * (1.0 + 1e-15 * np.random.default_rng(seed).standard_normal(len(x)))


def ct_floor(fs, fft_size):
    return 3.0 * fs / (fft_size - 3.0)  # GetF0FloorForCheapTrick


class Case:
    """one analysed signal: x (float64, read-only), its frame times t and the F0 contour handed to the analysis"""

    def __init__(self, name, fs, make, contour, fft_size=None, kind=None):
        self.name, self.fs, self._make, self._contour, self.fft_size, self.kind = name, fs, make, contour, fft_size, kind

    @property
    def x(self):
        return self._make()

    @property
    def t(self):
        return W.harvest_time_axis(len(self.x), self.fs)

    @property
    def f0(self):
        n = len(self.t)
        c = np.atleast_1d(np.asarray(self._contour, dtype=np.float64))
        return np.resize(c, n)  # a constant, or a pattern repeated frame by frame

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------ A. CheapTrick
def _ct_cases():
    out = []
    floor = ct_floor(FS, 1024)
    for label, v in (("zero", 0.0), ("floor", floor), ("floor_next", float(np.nextafter(floor, np.inf))),
                     ("largest_window", 70.6), ("100", 100.0), ("1000", 1000.0), ("5999", 5999.0)):
        src = v if v > 0 else 200.0  # the pulse train follows the contour where there is one
        out.append(Case(f"ct-24k-{label}", FS, functools.partial(pulses, FS, src, 0.4), v))
    # neighbouring workgroups on different branches: default F0, the largest window, a window of 13 samples
    out.append(Case("ct-24k-alternating", FS, functools.partial(pulses, FS, 200.0, 0.4), (0.0, 70.6, 5999.0)))
    for fft_size, values in ((512, (141.0, 141.5)), (2048, (35.0, 35.3))):  # either side of the floor of that size
        for v in values:
            out.append(Case(f"ct-24k-fft{fft_size}-{v}", FS, functools.partial(pulses, FS, v, 0.4), v, fft_size))
    for v in (100.0, 400.0):
        out.append(Case(f"ct-16k-{v:g}", 16000, functools.partial(pulses, 16000, v, 0.4), v))
    # shorter than one window: 1 frame up to 119 samples, 2 from 120 on; every tap of a frame is an edge repeat
    for L in (1, 2, 60, 119, 120, 121):
        for v in (0.0, 71.0, 5999.0):
            out.append(Case(f"ct-short-{L}-{v:g}", FS, functools.partial(noise, L, 100 + L), v))
    return out


CT_CASES = _ct_cases()


def _cheaptrick(case, x):
    return W.cheaptrick(x, case.f0, case.t, case.fs, fft_size=case.fft_size)


@functools.lru_cache(maxsize=None)
def _ct_ref(i):
    case = CT_CASES[i]
    sp = _cheaptrick(case, case.x)
    return _frozen(sp), _frozen(W.sp2mc(sp, ORDER, world.ALPHA[case.fs]))


def ct_ref(case):
    """(envelope, mel-cepstrum of it) of the oracle"""
    return _ct_ref(CT_CASES.index(case))


@functools.lru_cache(maxsize=None)
def _ct_moved(i):
    case = CT_CASES[i]
    return float(np.abs(np.log(_cheaptrick(case, perturbed(case.x)) / _ct_ref(i)[0])).max())


def ct_moved(case):
    """how far the oracle's log envelope moves under the perturbation"""
    return _ct_moved(CT_CASES.index(case))


# ------------------------------------------------------------------------------------------------ B. D4C
# kind "pulses": every frame's decision is asserted, none may be left out; "unvoiced": every band is the unvoiced
# constant (noise: rejected by the Love Train; silence: its exit for an all-zero frame); "short": mostly edge repeats,
# the share is arbitrary, so properties everywhere and the oracle only on the frames off the threshold.
def _d4c_cases():
    out = []
    for v in (35.0, 40.0, 42.0, 47.0, 47.5, 71.0, 100.0, 400.0, 1000.0):  # the 40 / 47 Hz floors, the offset at 100 Hz
        out.append(Case(f"d4c-24k-{v:g}", FS, functools.partial(pulses, FS, v, 0.4), v, kind="pulses"))
    for fs, values in ((16000, (60.0, 400.0)), (12000, (60.0, 200.0))):  # one band; 12 kHz: the 1024-point kernel
        for v in values:
            out.append(Case(f"d4c-{fs // 1000}k-{v:g}", fs, functools.partial(pulses, fs, v, 0.4), v, kind="pulses"))
    out.append(Case("d4c-noise", FS, functools.partial(noise, 9600, 7), 200.0, kind="unvoiced"))
    out.append(Case("d4c-silence", FS, functools.partial(silence, 2400), 150.0, kind="unvoiced"))
    for L in (1, 2, 60, 121):
        out.append(Case(f"d4c-short-{L}", FS, functools.partial(noise, L, 200 + L), 200.0, kind="short"))
    return out


D4C_CASES = _d4c_cases()


def _d4c(case, x):
    f0, t = case.f0, case.t
    bap = W.d4c_band_aperiodicity(x, f0, t, case.fs)
    share = np.array([W.d4c_love_train(x, case.fs, float(f0[i]), t[i]) for i in range(len(t))])
    return _frozen(bap), _frozen(share)


@functools.lru_cache(maxsize=None)
def _d4c_ref(i):
    return _d4c(D4C_CASES[i], D4C_CASES[i].x)


@functools.lru_cache(maxsize=None)
def _d4c_moved(i):
    return _d4c(D4C_CASES[i], perturbed(D4C_CASES[i].x))


def d4c_ref(case):
    """(band aperiodicity in dB, Love-Train share per frame) of the oracle"""
    return _d4c_ref(D4C_CASES.index(case))


def d4c_moved(case):
    """the same on the perturbed input"""
    return _d4c_moved(D4C_CASES.index(case))


def off_threshold(share):
    return np.abs(share - THRESHOLD) >= MARGIN


def d4c_decided(case):
    """frames whose decision the oracle can speak for: off the threshold, on the input and on the perturbed input"""
    return off_threshold(d4c_ref(case)[1]) & off_threshold(d4c_moved(case)[1])


def d4c_frame_moves(case):
    """per frame, how far the oracle's voiced bands move under the perturbation (0 where either run is unvoiced)"""
    a, b = d4c_ref(case)[0], d4c_moved(case)[0]
    both = voiced_rows(a) & voiced_rows(b)
    return np.where(both, np.abs(a - b).max(axis=1), 0.0)


def d4c_compared(case):
    """frames whose voiced values are held to TOL: decided and well conditioned.  The host test lets no frame of a
    "pulses" case fall out; of a short signal some do -- two samples are a step, whose aperiodicity is a ratio of
    rounding residues that the oracle itself moves by 1e-7 dB, whatever the seed."""
    return d4c_decided(case) & (d4c_frame_moves(case) < MOVE)


def voiced_rows(bap):
    return ~(bap == UNVOICED).all(axis=1)


# ------------------------------------------------------------------------------------------------ C. ragged batch
class Scaler:
    def __init__(self, mean, scale):
        self.mean_, self.scale_ = mean, scale


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """lengths 9650 / 121 / 60 -> 81 / 2 / 1 frames; decode-CLI contours of 41 / 3 / 1 values; a scaler and a noise
    draw.  dict(waves [float32], lengths, lf0, mean, scale, noise (3, 1, 81 hop) float32, frames)"""
    rng = np.random.default_rng(17)
    lengths = [9650, 121, 60]
    waves = [pulses(FS, 200.0, 9650 / FS, 1e-3, 5), noise(121, 321), noise(60, 360)]
    waves = [_frozen(w.astype(np.float32)) for w in waves]
    assert [len(w) for w in waves] == lengths
    first = np.full(41, 200.0)
    first[15:20] = 0.0  # an unvoiced stretch
    lf0 = [_frozen(first), _frozen(np.array([180.0, 0.0, 210.0])), _frozen(np.array([150.0]))]
    frames = [W.harvest_frame_count(n, FS) for n in lengths]
    return dict(waves=waves, lengths=lengths, lf0=lf0, mean=_frozen(rng.standard_normal(43)),
                scale=_frozen(rng.uniform(0.5, 2.0, 43)), frames=frames,
                noise=_frozen(rng.standard_normal((3, 1, max(frames) * HOP)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def ragged_ref(i):
    """W.analyze of item i as the stage sees it (through the PCM_16 file), plus its Love-Train shares"""
    b = ragged_batch()
    x = W.pcm16_roundtrip(b["waves"][i])
    ref = W.analyze(x, b["lf0"][i], FS, mean=b["mean"], scale=b["scale"])
    ref["share"] = np.array([W.d4c_love_train(x, FS, float(f), t) if f > 0 else 0.0 for f, t in zip(ref["f0"], ref["t"])])
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------ D. contours
MATCH_PAIRS = ((1, 1), (1, 5), (5, 1), (2, 600), (600, 2), (300, 300), (257, 513), (513, 257), (1000, 999))


@functools.lru_cache(maxsize=None)
def match_inputs():
    """one contour per (n_in, n_out) pair, in [-50, 800]: the clamp at 0 bites, the equal-length item keeps its
    negatives"""
    rng = np.random.default_rng(41)
    out = []
    for n_in, _ in MATCH_PAIRS:
        f = rng.uniform(-50.0, 800.0, n_in)
        f[-1] = -40.0  # every item ends below 0, the short ones too
        out.append(_frozen(f))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def match_refs():
    return tuple(_frozen(np.atleast_1d(W.match_length(f, n_out))) for f, (_, n_out) in zip(match_inputs(), MATCH_PAIRS))


CONT_LENGTHS = (1, 2, 255, 256, 257, 600)  # NT_F0 = 256: below, at and past one chunk, and past two


@functools.lru_cache(maxsize=None)
def cont_items():
    """(label, contour) for every length and voicing pattern"""
    rng = np.random.default_rng(43)
    out = []
    for n in CONT_LENGTHS:
        v = rng.uniform(60.0, 700.0, n)
        only = lambda i: np.where(np.arange(n) == i, v, 0.0)
        pats = [("voiced", v.copy()), ("zero", np.zeros(n)), ("first", only(0)), ("last", only(n - 1)),
                ("middle", only(n // 2)), ("alternating", np.where(np.arange(n) % 2 == 0, v, 0.0)),
                ("random", np.where(rng.random(n) < 0.2, 0.0, v))]
        if n == 600:
            gap = v.copy()
            gap[200:401] = 0.0  # spans the chunk boundary at 256
            pats.append(("gap", gap))
        out += [(f"{label}-{n}", _frozen(p)) for label, p in pats]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cont_refs():
    """(uv, cf0, ok) of the reference's function per item"""
    return tuple(W.convert_continuos_f0(f) for _, f in cont_items())


# ------------------------------------------------------------------------------------------------ E. excitation
EXC_FRAMES = (600, 257, 256, 255, 1)


@functools.lru_cache(maxsize=None)
def excitation_batch():
    """hand-made contours past one chunk of sine_phase_kernel: dict(f0, cf0 (B, 600) float64 zero-padded, noise)"""
    rng = np.random.default_rng(47)
    F = max(EXC_FRAMES)
    f0, cf0 = np.zeros((len(EXC_FRAMES), F)), np.zeros((len(EXC_FRAMES), F))
    for b, n in enumerate(EXC_FRAMES):
        v = rng.uniform(50.0, 1100.0, n)
        if n > 1:
            v[40:70] = 0.0
            v[n - 20:n - 5] = 0.0
            v[250:min(262, n)] = 0.0  # an unvoiced stretch over the chunk boundary
            cf0[b, :n] = W.convert_continuos_f0(v)[1]
        else:
            cf0[b, :n] = v
        f0[b, :n] = v
    noise_draw = rng.standard_normal((len(EXC_FRAMES), 1, F * HOP)).astype(np.float32)
    return dict(f0=_frozen(f0), cf0=_frozen(cf0), noise=_frozen(noise_draw))


def excitation_ref(contour, noise_draw, sine_amp=0.1, noise_amp=0.003):
    """SignalGenerator on one item's contour (n,) with its share of the draw (1, 1, n hop) -> (n hop,) float32"""
    c32 = torch.tensor(np.asarray(contour), dtype=torch.float32).view(1, 1, -1)
    return W.signal_generator_sine(c32, FS, HOP, sine_amp, noise_amp, noise=torch.from_numpy(np.array(noise_draw)))[0, 0].numpy()
