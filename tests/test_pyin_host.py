"""CPU checks of pYIN (serenade_amd/pitch.py): the restatement tests/_pyin_ref.py (librosa 0.10 librosa.pyin) and the
host-built tables the HIP kernels take.  No GPU."""
import itertools

import numpy as np
import pytest
import scipy.stats

from serenade_amd import pitch

from . import _pyin_ref as R

TRANS = dict(fmin=65, fmax=2093, sr=16000, frame_length=1024, hop_length=320)  # decoding.py:36-45 at the transcriber's


def _tone(f, sec, sr, n_harm=4, amp=0.3, seed=0):
    t = np.arange(int(sec * sr)) / sr
    y = sum(amp / k * np.sin(2 * np.pi * f * k * t + k) for k in range(1, n_harm + 1))
    return (y + 1e-4 * np.random.default_rng(seed).standard_normal(len(t))).astype(np.float32)


def test_constants_at_the_transcriber_settings():
    g = pitch.pyin_geometry(fmin=65, fmax=2093, sr=16000, frame_length=1024, hop_length=320)
    assert (g["min_period"], g["max_period"], g["n_bins"], g["width"], g["win_length"]) == (7, 247, 602, 91, 512)
    assert g == R.geometry(**TRANS)
    t = R.transition(602, 91, 0.01)
    np.testing.assert_allclose(t.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    thr, beta_probs = R.prior_tables()
    assert abs(beta_probs.sum() - 1.0) < 1e-12 and len(thr) == 100


def test_log_band_equals_the_dense_log_transition():
    n, w, s = 602, 91, 0.01
    dense = np.log(R.transition(n, w, s) + R.TINY)
    band = pitch.log_band(n, w, s)
    h = w // 2
    L = np.log(R.TINY)
    i, j = np.meshgrid(np.arange(2 * n), np.arange(2 * n), indexing="ij")  # predecessor i, state j
    pi, qj = i % n, j % n
    inband = np.abs(pi - qj) <= h
    kind = (i // n != j // n).astype(int)
    got = np.full((2 * n, 2 * n), L)
    got[inband] = band[kind[inband], (pi - qj + h)[inband], qj[inband]]
    assert np.array_equal(got, dense)
    assert (dense[~inband] == L).all() and (band >= L).all()


def test_prior_tables_match_scipy_boltzmann_bitwise():
    thr, beta_probs, fact, bexp, no_trough = pitch.prior_tables(100, (2, 18), 2, 0.01, 241)
    rthr, rbeta = R.prior_tables()
    assert np.array_equal(thr, rthr) and np.array_equal(beta_probs, rbeta)
    for cnt in (1, 2, 3, 17, 120, 241):
        pos = np.arange(cnt)
        assert np.array_equal(fact[cnt] * bexp[pos], scipy.stats.boltzmann.pmf(pos, 2, cnt))
    for m in (0, 1, 7, 100):
        assert no_trough[m] == 0.01 * np.sum(beta_probs[:m])


def _brute_force(prob, trans, p_init):
    """the best path over all S^T paths (log domain), first in lexicographic order on a tie"""
    lt, lp, l0 = np.log(trans + R.TINY), np.log(prob + R.TINY), np.log(p_init + R.TINY)
    T, S = prob.shape
    best, arg = -np.inf, None
    for path in itertools.product(range(S), repeat=T):
        v = l0[path[0]] + lp[0, path[0]]
        for t in range(1, T):
            v = v + lt[path[t - 1], path[t]] + lp[t, path[t]]
        if v > best:
            best, arg = v, path
    return np.array(arg)


@pytest.mark.parametrize("seed", range(6))
def test_dense_viterbi_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    S, T = 4, 5
    prob = rng.random((T, S)) ** 3
    prob[rng.random((T, S)) < 0.3] = 0.0
    trans = rng.random((S, S))
    trans[rng.random((S, S)) < 0.3] = 0.0
    trans /= trans.sum(axis=1, keepdims=True)
    p_init = rng.random(S)
    p_init /= p_init.sum()
    assert np.array_equal(R.viterbi(prob, trans, p_init), _brute_force(prob, trans, p_init))


def test_dense_viterbi_takes_an_out_of_band_octave_leap():
    n, w = 602, 91
    T = 8
    voiced = np.zeros((T, n))
    voiced[:4, 100] = 1.0
    voiced[4:, 220] = 1.0  # one octave (120 bins) up, far outside the 45-bin band
    vp = np.ones(T)  # unvoiced states cost log(tiny) too
    p_init = np.zeros(2 * n)
    p_init[n:] = 1 / n
    states = R.viterbi(R.obs_matrix(voiced, vp), R.transition(n, w, 0.01), p_init)
    assert list(states) == [100] * 4 + [220] * 4
    # a decoder confined to the band would have to stay within 45 bins of bin 100
    assert abs(int(states[4]) - int(states[3])) > w // 2


def test_restatement_tracks_a_harmonic_tone_and_silence():
    y = _tone(220.0, 1.0, 16000)
    f0, flag, vp, _ = R.pyin(y, **TRANS)
    assert len(f0) == 1 + len(y) // 320
    interior = slice(3, len(f0) - 3)
    assert flag[interior].all()
    bins = 120 * np.log2(f0[interior] / 220.0)
    assert np.abs(bins).max() <= 1.0
    f0, flag, vp, _ = R.pyin(np.zeros(8000, np.float32), **TRANS)
    assert np.isnan(f0).all() and not flag.any() and (vp == 0).all()


@pytest.mark.parametrize("kw", [
    dict(fmin=65, fmax=9000, sr=16000),                       # fmax above Nyquist
    dict(fmin=500, fmax=400, sr=16000),                       # fmin >= fmax
    dict(fmin=65, fmax=2093, sr=16000, win_length=1024),      # win_length >= frame_length
    dict(fmin=65, fmax=200, sr=16000, frame_length=256, win_length=200),  # the period range does not fit
    dict(fmin=65, fmax=2093, sr=16000, pad_mode="reflect"),   # only librosa 0.10's constant padding
    dict(fmin=100, fmax=800, sr=8000, frame_length=512, win_length=300, hop_length=700),  # width 381 over 361 bins
])
def test_pyin_rejects_bad_parameters(kw):
    kw = dict(dict(frame_length=1024), **kw)
    with pytest.raises(ValueError):
        pitch.pyin(None, **kw)


def test_frame_counts():
    assert pitch.pyin_frames([16000, 1, 320, 319, 1023, 160000], 1024, 320) == [51, 1, 2, 1, 4, 501]
    assert pitch.pyin_frames([2048, 22050], 2048) == [1 + 2048 // 512, 1 + 22050 // 512]
    for n in (1, 500, 1024, 4321):
        assert pitch.pyin_frames([n], 1024, 320)[0] == len(R.frames_of(np.zeros(n), 1024, 320))


def test_restatement_matches_librosa_when_installed():
    librosa = pytest.importorskip("librosa")
    rng = np.random.default_rng(3)
    for y in (_tone(220.0, 1.0, 16000).astype(np.float64), 0.1 * rng.standard_normal(16000)):
        f0, flag, vp, near = R.pyin(y, **TRANS)
        lf0, lflag, lvp = librosa.pyin(y, fill_na=np.nan, center=True, **TRANS)
        assert (flag == lflag).mean() > 0.99
        both = flag & lflag
        assert (f0[both] == lf0[both]).mean() > 0.99
        np.testing.assert_allclose(vp, lvp, atol=1e-9)
