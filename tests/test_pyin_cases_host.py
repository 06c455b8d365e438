"""The cases of tests/_pyin_cases.py are fit to be judged: no GPU here, only the float64 restatement against itself.

tests/test_zzzz_hip_pyin_sweep.py holds pyin.hip to tests/_pyin_ref.py state for state off the frames the restatement flags
as near-ties.  That only judges the kernels if (a) few frames are flagged, (b) a case has the voiced and unvoiced frames
its signal promises, and (c) it reaches the branch it is named for.  (c) is shown the hard way: a deliberately wrong
variant of the restatement (the argmax taking the last index, a Viterbi confined to the band, trough positions
restarted at every 64th trough, the smaller period winning a shared bin) must give a different answer on the named
case.  A case that misses a condition is replaced, never excused, and no bound moves.

Measured when the cases were chosen: no frame of any case is flagged near except those of silence and of the one-sample
item (every difference is zero there; their answer is asserted absolutely instead); "largest-noise" has 327 troughs in
one frame, but a lost chunk carry moves none of its observations, so "largest-mixed" (the same noise over a
30 Hz tone, 246 troughs) stands for that variant; the largest geometry asks for 103 640 of the 114 688 bytes of LDS."""
import numpy as np
import pytest

from tests import _pyin_cases as C
from tests import _pyin_ref as R


# ------------------------------------------------------------------------------------------------ wrong variants
def _decode(prob, trans, p_init, last=False, band=None, n=None, probe=False):
    """R.viterbi with, on request, the last index instead of the first at every argmax (last), or predecessors further
    than `band` bins away forbidden (band, n bins per half).  probe=True returns instead the (frame, state) pairs at
    which the dense maximum is attained both by a predecessor inside the band and by one outside it."""
    log_trans = np.log(trans + R.TINY)
    log_prob = np.log(prob + R.TINY)
    T, S = prob.shape
    arg = (lambda m: S - 1 - np.argmax(m[::-1], axis=0)) if last else (lambda m: np.argmax(m, axis=0))
    inside = None
    if band is not None:
        q = np.arange(S) % n
        inside = np.abs(q[:, None] - q[None, :]) <= band
        if not probe:
            log_trans = np.where(inside, log_trans, -np.inf)
    value = log_prob[0] + np.log(p_init + R.TINY)
    ptr = np.zeros((T, S), dtype=np.int64)
    hits = []
    for t in range(1, T):
        m = value[:, None] + log_trans
        ptr[t] = arg(m)
        best = m[ptr[t], np.arange(S)]
        if probe:
            at = m == best[None, :]
            both = (at & inside).any(0) & (at & ~inside).any(0)
            hits += [(t, int(j)) for j in np.nonzero(both)[0]]
        value = log_prob[t] + best
    if probe:
        return hits
    state = np.zeros(T, dtype=np.int64)
    state[-1] = arg(value[:, None])[0]
    for t in range(T - 2, -1, -1):
        state[t] = ptr[t + 1, state[t + 1]]
    return state


def _observe(x, shift, g, sr, fmin, thresholds, beta_probs, boltzmann_parameter, no_trough_prob, restart64=False,
             smaller_wins=False):
    """R.observe_frame's voiced row with, on request, the trough positions counted afresh in every chunk of 64 troughs
    (a lost chunk carry) or the smaller period winning a shared bin"""
    import scipy.stats
    n_bins = g["n_bins"]
    obs = np.zeros(n_bins + 1)
    (ti,) = np.nonzero(R.troughs(x))
    if len(ti):
        h = x[ti]
        below = np.less.outer(h, thresholds)
        pos = np.cumsum(below, axis=0) - 1
        if restart64:
            pos = np.concatenate([np.cumsum(below[i:i + 64], axis=0) - 1 for i in range(0, len(ti), 64)])
        cnt = np.count_nonzero(below, axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            prior = scipy.stats.boltzmann.pmf(pos, boltzmann_parameter, cnt)
        prior[~below] = 0
        probs = np.cumsum(prior * beta_probs, axis=1)[:, -1]
        gm = np.argmin(h)
        probs[gm] += no_trough_prob * np.sum(beta_probs[:np.count_nonzero(~below[gm, :])])
        keep = probs != 0
        i = ti[keep]
        f0 = sr / ((g["min_period"] + i) + shift[i])
        b = np.clip(np.round(12 * g["nbps"] * np.log2(f0 / fmin)), 0, n_bins).astype(int)
        if smaller_wins:
            obs[b[::-1]] = probs[keep][::-1]
        else:
            obs[b] = probs[keep]
    return obs[:n_bins]


def _voiced(case, **wrong):
    kw, st = case.kw, C.ref(case)[4]
    thr, beta = R.prior_tables(kw.get("n_thresholds", 100), kw.get("beta_parameters", (2, 18)))
    return np.stack([_observe(x, R.parabolic_shift(x), st["geometry"], kw["sr"], kw["fmin"], thr, beta,
                              kw.get("boltzmann_parameter", 2), kw.get("no_trough_prob", 0.01), **wrong)
                     for x in st["yin"]])


def _states(case, **wrong):
    f0, flag, vp, near, st = C.ref(case)
    g, n = st["geometry"], st["geometry"]["n_bins"]
    p_init = np.zeros(2 * n)
    p_init[n:] = 1 / n
    trans = R.transition(n, g["width"], case.kw.get("switch_prob", 0.01))
    return _decode(R.obs_matrix(st["voiced"], vp), trans, p_init, n=n, **wrong)


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("case", C.CASES, ids=repr)
def test_cases_are_decided(case):
    f0, flag, vp, near, st = C.ref(case)
    g = st["geometry"]
    troughs = [int(R.troughs(x).sum()) for x in st["yin"]]
    print(f"{case}: {len(f0)} frames, {g['n_bins']} bins, width {g['width']}, "
          f"{g['max_period'] - g['min_period'] + 1} periods, near share {near.mean():.3f}, voiced {int(flag.sum())}, "
          f"most troughs in a frame {max(troughs)}, LDS {C.observe_lds(case)} bytes")
    assert C.observe_lds(case) <= C.OBSERVE_LDS_CAP
    assert st["voiced"].shape == (len(f0), g["n_bins"]) and np.isfinite(st["voiced"]).all()
    if case.absolute:  # every difference is zero: all frames are flagged, and the answer is known without the flag
        assert max(troughs) == 0 and not st["voiced"].any() and not vp.any() and not flag.any()
        return
    assert near.mean() <= C.NEAR_CAP
    assert case.voiced is None or flag.any() == case.voiced
    assert not case.tail or (~flag).any()


def test_the_same_transition_and_the_variants_with_nothing_wrong_are_the_restatement():
    """the variant code with every switch off is the restatement bit for bit, so a difference below is the switch's"""
    for name in ("coarse", "narrow", "width1"):
        c = C.BY_NAME[name]
        assert np.array_equal(_voiced(c), C.ref(c)[4]["voiced"]), name
        assert np.array_equal(_states(c), C.ref(c)[4]["states"]), name


def test_geometries_are_the_ones_the_cases_are_named_for():
    g = {c.name: c.g for c in C.CASES}
    per = lambda k: g[k]["max_period"] - g[k]["min_period"] + 1
    assert (g["fine"]["n_bins"], g["fine"]["width"]) == (1203, 181) and 2 * 1203 > 2048  # second trip of q += 1024
    assert (g["coarse"]["n_bins"], g["coarse"]["width"]) == (121, 19)
    assert g["width1"]["width"] == 1 and len(C.ref(C.BY_NAME["width1"])[0]) == 76
    assert (g["narrow"]["min_period"], g["narrow"]["max_period"], g["narrow"]["n_bins"], g["narrow"]["width"]) == (6, 8, 32, 21)
    assert per("narrow") == 3 and (g["narrow-wide"]["n_bins"], g["narrow-wide"]["width"]) == (32, 31)
    assert per("largest-tone") == 993 and (g["largest-tone"]["n_bins"], g["largest-tone"]["width"]) == (781, 201)
    assert 100 * 1024 < C.observe_lds(C.BY_NAME["largest-tone"]) <= C.OBSERVE_LDS_CAP
    assert g["nocenter-win300"]["win_length"] == 300 and g["nocenter-win300"]["max_period"] == 247
    assert [len(C.BY_NAME[k].y) for k in C.RAGGED] == [1, 319, 320, 321, 2000, 4000]
    assert [len(C.ref(C.BY_NAME[k])[0]) for k in C.RAGGED] == [1, 1, 2, 2, 7, 13]


def test_largest_cases_carry_trough_positions_over_chunks_of_64():
    """white noise alone has the troughs (327 in one frame) but every one of them lies above all the thresholds that
    carry prior mass, so a lost carry changes nothing in it (measured: the variant's observations are identical);
    the same noise over a 30 Hz tone puts deep troughs behind the first 64, and there the carry decides"""
    for name in ("largest-noise", "largest-mixed"):
        c = C.BY_NAME[name]
        most = max(int(R.troughs(x).sum()) for x in C.ref(c)[4]["yin"])
        print(f"{name}: {most} troughs in one frame")
        assert most > 128
    wrong = _voiced(c, restart64=True)
    assert not np.array_equal(wrong, C.ref(c)[4]["voiced"])
    print(f"positions restarted every 64 troughs: observations move by {np.abs(wrong - C.ref(c)[4]['voiced']).max():.2e}")
    assert np.abs(wrong - C.ref(c)[4]["voiced"]).max() > 1e3 * C.TOL


def test_coarse_has_shared_bins_that_the_larger_period_wins():
    c = C.BY_NAME["coarse"]
    wrong = _voiced(c, smaller_wins=True)
    d = np.abs(wrong - C.ref(c)[4]["voiced"])
    print(f"coarse: the smaller period winning a shared bin moves {np.count_nonzero(d)} observations by up to {d.max():.2e}")
    assert d.max() > 1e3 * C.TOL


@pytest.mark.parametrize("name", ["switch0", "switch1"])
def test_switch_cases_tie_with_the_out_of_band_maximum(name):
    c = C.BY_NAME[name]
    f0, flag, vp, near, st = C.ref(c)
    band = c.g["width"] // 2
    hits = _states(c, band=band, probe=True)
    print(f"{name}: the dense maximum is attained in and out of band at {len(hits)} (frame, state) pairs")
    assert hits


def test_switch0_needs_the_first_index():
    c = C.BY_NAME["switch0"]
    assert not np.array_equal(_states(c, last=True), C.ref(c)[4]["states"])


def test_width1_path_leaves_the_band():
    c = C.BY_NAME["width1"]
    states, n = C.ref(c)[4]["states"], c.g["n_bins"]
    bins = sorted(set(int(v) for v in states % n))
    print(f"width1: the decoded path visits bins {bins}")
    assert c.g["width"] // 2 == 0 and len(bins) > 1  # a band of one bin: any change of bin is out of band
    assert not np.array_equal(_states(c, band=0), states)


def test_an_octave_leap_stays_in_band_and_the_synthetic_leap_does_not():
    """Measured when the cases were chosen: the restatement decodes the 150 -> 300 Hz signal as 150 Hz throughout (the
    sub-octave is a trough of the upper tone too, and one out-of-band move costs log(tiny) = -708), and the same holds
    for every natural leap tried at a band wider than one bin (150 -> 220 / 260 / 330 / 400 Hz, 200 -> 280 Hz at
    widths 11, 21 and 91: the path walks through the mixed frames or takes a sub-harmonic).  So no natural signal
    shows a band-confined decoder wrong at these widths; the octave leap stays as a decode case and the leap is made
    in the observations handed to the Viterbi kernel alone."""
    c = C.BY_NAME["leap"]
    states, n, h = C.ref(c)[4]["states"], c.g["n_bins"], c.g["width"] // 2
    print(f"leap: largest move between frames {np.abs(np.diff(states % n)).max()} bins, band half-width {h}")
    voiced, vp, frames, ref = C.synthetic_leap()
    n, h = voiced.shape[2], 90
    assert list(ref[0][3:11]) == [100] * 4 + [700] * 4 and 2 * n > 2048
    p_init = np.zeros(2 * n)
    p_init[n:] = 1 / n
    wrong = _decode(R.obs_matrix(voiced[0, :frames[0]], vp[0, :frames[0]]), R.transition(n, 181, 0.01), p_init, band=h, n=n)
    assert not np.array_equal(wrong, ref[0])


def test_quiet_case_straddles_the_zeroing_threshold():
    """some window energies of one signal fall below the 1e-6 at which the difference function zeroes them and some
    above (the near cap is test_cases_are_decided's)"""
    c = C.BY_NAME["quiet"]
    g, W = c.g, c.g["win_length"]
    below = above = 0
    for f in R.frames_of(c.y, c.kw["frame_length"], g["hop_length"], c.kw["center"]):
        s = np.cumsum(f * f)
        e = s[W:W + g["max_period"] + 1] - s[:g["max_period"] + 1]
        below += int((np.abs(e) < 1e-6).sum())
        above += int((np.abs(e) >= 1e-6).sum())
    print(f"quiet: {below} window energies below 1e-6, {above} at or above")
    assert below > 50 and above > 50
    assert C.ref(c)[1].any()  # and it still decodes voiced frames
