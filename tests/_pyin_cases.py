"""TEST-ONLY: the edge cases of the pYIN kernels (csrc/pyin.hip: srn_pyin_observe, srn_pyin_viterbi), shared by the
CPU test that proves the cases fit to be judged (tests/test_pyin_cases_host.py) and the run on the GPU
(tests/test_zzzz_hip_pyin_sweep.py): same signals, same reference, same bounds.  Nothing here launches anything.

Reference: tests/_pyin_ref.py (float64 numpy + scipy).  Bounds, none of them new: states, f0 and flags identical on
the frames the restatement does not flag as near-ties (tests/test_hip_pyin.py's _compare), voiced_prob and every entry
of the voiced observation matrix within 1e-12 absolute.

A case is only fit to judge the kernel if the restatement decides it: at most NEAR_CAP of its frames may be flagged
near, it must have the voiced / unvoiced frames its signal promises, and it must reach the branch it is named for.
These are CONDITIONS ON THE INPUTS, asserted by the host test and never excused.  Silence and the one-sample item are
the exception to the near flag, not to the check: every difference of theirs is zero, so the restatement flags every
frame, and what they must give is known absolutely (no trough, voiced_prob 0, an all-zero observation row, every frame
unvoiced); both tests assert exactly that.  The one sample is 0.25: its square is a power of two, so the running sums
of the difference function are exact and the normalised difference is exactly 1 at every period (no trough) whatever
the order of summation.

Each reference is computed once per process and never written to.
"""
import functools

import numpy as np

from . import _pyin_ref as R

TOL = 1e-12       # voiced_prob and observation entries, absolute
NEAR_CAP = 0.05   # share of a case's frames the restatement may flag near
TRANS = dict(fmin=65, fmax=2093, sr=16000, frame_length=1024, hop_length=320)  # the transcriber's settings
NARROW = dict(fmin=2000, fmax=2400, sr=16000, frame_length=256, hop_length=64)
LARGEST = dict(fmin=22, fmax=2000, sr=22050, frame_length=4096)
OBSERVE_LDS_CAP = 112 * 1024  # kObserveSmemMax of pyin.hip


def _frozen(a):
    a.setflags(write=False)
    return a


def harmonics(f, sr, amp=0.3, n_harm=3):
    """n_harm harmonics at amplitude amp / k of the instantaneous frequency f (Hz per sample), float64"""
    ph = 2 * np.pi * np.cumsum(f) / sr
    return sum(amp / k * np.sin(k * ph + 0.3 * k) for k in range(1, n_harm + 1))


@functools.lru_cache(maxsize=None)
def base(n, sr=16000, f=220.0, f_end=None, amp=0.3, noise=1e-3, voiced=0.7, seed=0):
    """the base signal: three harmonics at amp / k (a glide to f_end if given), silent after `voiced` of the item,
    plus white noise over the whole item, as float32"""
    freq = np.full(n, float(f)) if f_end is None else np.linspace(f, f_end, n)
    gate = (np.arange(n) < voiced * n).astype(np.float64)
    y = harmonics(freq, sr, amp) * gate + noise * np.random.default_rng(seed).standard_normal(n)
    return _frozen(y.astype(np.float32))


@functools.lru_cache(maxsize=None)
def white(n, amp=0.1, seed=5):
    return _frozen((amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def noisy_tone(n, sr=22050, f=30.0, amp=0.1, seed=5):
    """the 30 Hz tone under 0.1 x white noise: hundreds of shallow noise troughs per frame and, behind them at the
    tone's period and its harmonics', deep ones whose position among the troughs below a threshold is what counts"""
    y = harmonics(np.full(n, float(f)), sr) + white(n, amp, seed).astype(np.float64)
    return _frozen(y.astype(np.float32))


@functools.lru_cache(maxsize=None)
def leap(n, f1=150.0, f2=300.0, noise=1e-3, sr=16000, seed=2):
    """f1, then f2 from the middle of the item on"""
    f = np.where(np.arange(n) < n // 2, f1, f2)
    y = harmonics(f, sr) + noise * np.random.default_rng(seed).standard_normal(n)
    return _frozen(y.astype(np.float32))


@functools.lru_cache(maxsize=None)
def synthetic_leap(n=1203, width=181, switch_prob=0.01, frames=(14, 9, 1), seed=11):
    """observations handed to the Viterbi alone, at the "fine" geometry (2406 states): sparse random rows, and in item 0
    a run of certain frames (voiced_prob 1: every unvoiced state costs log(tiny)) whose only observation jumps from bin
    100 to bin 700, which no path inside the 90-bin band can follow; a run without any observation in item 1.
    Returns (voiced (B, T, n), voiced_prob (B, T), frames, reference states per item)."""
    rng = np.random.default_rng(seed)
    B, T = len(frames), max(frames)
    voiced = rng.random((B, T, n)) ** 8 * (rng.random((B, T, n)) < 0.02)
    vp = np.clip(voiced.sum(-1), 0, 1)
    vp[0, 3:11] = 1.0
    voiced[0, 3:11] = 0.0
    voiced[0, 3:7, 100] = 1.0
    voiced[0, 7:11, 700] = 1.0
    voiced[1, 4:7] = 0.0
    vp[1, 4:7] = 0.0
    p_init = np.zeros(2 * n)
    p_init[n:] = 1 / n
    trans = R.transition(n, width, switch_prob)
    ref = [_frozen(R.viterbi(R.obs_matrix(voiced[b, :f], vp[b, :f]), trans, p_init)) for b, f in enumerate(frames)]
    return _frozen(voiced), _frozen(vp), frames, ref


@functools.lru_cache(maxsize=None)
def quiet(n, amp, seed=3):
    """a 220 Hz tone so quiet that the energy of a 512-sample window (about 350 amp^2) sits at the 1e-6 below which
    the difference function's terms are zeroed; the noise keeps the zeroed stretches from being exact ties"""
    y = harmonics(np.full(n, 220.0), 16000, amp) + 0.02 * amp * np.random.default_rng(seed).standard_normal(n)
    return _frozen(y.astype(np.float32))


class Case:
    """one item: its signal (float32, read-only), the keywords of its pyin call, and what its frames must show.
    voiced: True (has voiced frames), False (has none), None (not asserted); tail: has unvoiced frames;
    absolute: the known all-unvoiced, all-zero answer is asserted directly (the near flag excuses nothing)"""

    def __init__(self, name, make, kw, voiced=True, tail=True, absolute=False):
        self.name, self._make, self.kw, self.voiced, self.tail, self.absolute = name, make, kw, voiced, tail, absolute

    @property
    def y(self):
        return self._make()

    @property
    def g(self):
        k = {a: v for a, v in self.kw.items() if a in ("fmin", "fmax", "sr", "frame_length", "win_length", "hop_length",
                                                        "resolution", "max_transition_rate")}
        return R.geometry(**k)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = BY_NAME[name]
    f0, flag, vp, near, st = R.pyin(c.y, **c.kw, stages=True)
    for a in (f0, flag, vp, near, st["yin"], st["voiced"], st["states"]):
        _frozen(a)
    return f0, flag, vp, near, st


def ref(case):
    """(f0, flag, voiced_prob, near, stages) of the restatement, computed once"""
    return _ref(case.name)


def observe_lds(case):
    """bytes of LDS srn_pyin_observe asks for (observe_smem of pyin.hip)"""
    g = case.g
    L, nf = g["win_length"] + g["max_period"] + 1, g["max_period"] - g["min_period"] + 1
    return (2 * L + g["max_period"] + 1 + 4 * nf + g["n_bins"] + 1) * 8 + (2 * nf + 2 * case.kw.get("n_thresholds", 100)) * 4


def T(**kw):
    return dict(TRANS, **kw)


# chosen on the CPU from the restatement alone (tests/test_pyin_cases_host.py asserts it): without centring, 105 of the
# 3968 window energies fall below 1e-6 and no frame is flagged near.  Centred, frame 0 always is (its first window is all
# padding and its next ones hold a few quiet samples: zero energies, zero differences), so the quiet case is not centred.
QUIET_AMP = 5.38e-5

_b6 = lambda: base(6000)
CASES = [
    Case("fine", lambda: base(4000), T(resolution=0.05)),
    # a 70 Hz tone under 0.05 noise: several troughs around the period's minimum fall into one half-semitone bin
    Case("coarse", lambda: base(6000, f=70.0, noise=0.05), T(resolution=0.5)),
    # 200 Hz, then 280 Hz: with a band of one bin the decoded path can only follow by leaving the band
    Case("width1", lambda: leap(1200, 200.0, 280.0, 1e-4), T(hop_length=16), tail=False),
    Case("narrow", lambda: base(1500, f=2200.0), NARROW),
    Case("narrow-wide", lambda: base(1500, f=2200.0), dict(NARROW, max_transition_rate=62.0)),
    Case("largest-tone", lambda: base(6000, sr=22050, f=30.0), LARGEST),
    Case("largest-noise", lambda: white(6000), LARGEST, voiced=None, tail=False),
    Case("largest-mixed", lambda: noisy_tone(6000), LARGEST, tail=False),
    Case("switch0", _b6, T(switch_prob=0.0)),
    Case("switch1", _b6, T(switch_prob=1.0), voiced=None, tail=False),
    Case("thresholds-1", _b6, T(n_thresholds=1), voiced=None),
    Case("thresholds-63", _b6, T(n_thresholds=63)),
    Case("thresholds-64", _b6, T(n_thresholds=64)),
    Case("thresholds-65", _b6, T(n_thresholds=65, beta_parameters=(1, 1), boltzmann_parameter=0.5, no_trough_prob=0.0),
         voiced=None),
    Case("thresholds-129", _b6, T(n_thresholds=129)),
    Case("nocenter", lambda: base(3000, voiced=0.45), T(center=False)),
    Case("nocenter-win300", lambda: base(3000, voiced=0.45), T(center=False, win_length=300)),
    Case("fill-none", _b6, T(fill_na=None)),
    Case("fill-zero", _b6, T(fill_na=0.0)),
    Case("loud", lambda: base(6000, amp=1e4, noise=1e-3 * 1e4 / 0.3), TRANS),
    Case("quiet", lambda: quiet(6000, QUIET_AMP), T(center=False), voiced=None, tail=False),
    Case("leap", lambda: leap(6000), TRANS, tail=False),
    # the ragged batch at the transcriber's settings
    Case("one-sample", lambda: _frozen(np.array([0.25], dtype=np.float32)), TRANS, voiced=False, absolute=True),
    Case("silence", lambda: _frozen(np.zeros(2000, dtype=np.float32)), TRANS, voiced=False, absolute=True),
    Case("len319", lambda: base(319, voiced=1.0), TRANS, voiced=None, tail=False),
    Case("len320", lambda: base(320, voiced=1.0), TRANS, voiced=None, tail=False),
    Case("len321", lambda: base(321, voiced=1.0), TRANS, voiced=None, tail=False),
    Case("len4000", lambda: base(4000), TRANS),
]
BY_NAME = {c.name: c for c in CASES}
RAGGED = ["one-sample", "len319", "len320", "len321", "silence", "len4000"]  # one batch, tail filled with 1e4
SINGLE = [c.name for c in CASES if c.name not in RAGGED]
EXACT = ["len4000", "one-sample", "leap", "len321", "loud", "silence"]  # share TRANS: each equals its B = 1 call
