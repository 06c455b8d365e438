"""TEST-ONLY: the edge cases of the Harvest kernels (csrc/harvest.hip: srn_harvest_decimate, srn_harvest_channels,
srn_harvest_candidates, srn_harvest_refine, srn_harvest_contour), shared by the CPU test that proves the cases fit to be
judged (tests/test_harvest_cases_host.py) and the run on the GPU (tests/test_zzzz_hip_harvest_sweep.py): same inputs, same
reference, same bounds.  Nothing here launches anything.

Reference: tests/_harvest_ref.py (float64 numpy + scipy), stage by stage, so every input below is the input of ONE
stage: a signal for the decimator, an analysis signal for the channel kernel, and from there on synthetic tables
written straight into the plan's buffers (raw candidates, candidates, refined candidates and scores), because the
shapes that decide these kernels -- a run of exactly 10 channels, a window clamped at both ends, a voiced section of
exactly voice_range_minimum frames, a gap of exactly STEP4_GAP -- are not what natural tones produce.

Bounds, none of them new (tests/test_hip_harvest.py's): decimation 1e-12 of the input's peak; raw candidates, official
candidates and refined F0 1e-9 relative; score 1e-6 relative; the contour before smoothing bit for bit, smoothed 1e-12
relative; voiced / unvoiced patterns identical off the entries the restatement flags as near-ties.

Each reference is computed once per process and never written to.
"""
import functools

import numpy as np

from . import _harvest_ref as R

DEC_TOL, REL_TOL, SCORE_TOL, SMOOTH_TOL = 1e-12, 1e-9, 1e-6, 1e-12
DEC_TILE, CH_TILE = 1024, 256  # samples per tile of the decimator and of the channel kernel (harvest.hip)
DEC_FS = (16000, 32000, 40000, 44100, 96000)  # ratios 2, 4, 5, 6, 12
FS8 = 8000  # ratio 1: the analysis signal is the signal


def _frozen(a):
    a.setflags(write=False)
    return a


def frames_to_samples(F1, fs=FS8):
    """a length whose item has exactly F1 internal (1 ms) frames"""
    n = max(1, (F1 - 1) * fs // 1000)
    assert R.frame_count(n, fs, 1.0) == F1
    return n


# ------------------------------------------------------------------------------------------------ 1. decimation
def dec_geometry(fs):
    ratio = R.geometry(fs)["ratio"]
    return ratio, int(np.ceil(R.DECIMATE_LAG_SAMPLES / ratio) * ratio)


def dec_lengths(fs):
    """1, 2, ratio - 1, ratio, ratio + 1 samples, and the lengths whose reflected, extended signal (n + 2 lag + 18
    samples, what the decimator walks in tiles of 1024) is one short of a tile, a tile, and one more; at ratio 2 also
    two tiles and one more"""
    ratio, lag = dec_geometry(fs)
    edge = [m - 2 * lag - 18 for m in (DEC_TILE - 1, DEC_TILE, DEC_TILE + 1)]
    if ratio == 2:
        edge += [m - 2 * lag - 18 for m in (2 * DEC_TILE, 2 * DEC_TILE + 1)]
    return sorted(set([1, 2, ratio - 1, ratio, ratio + 1] + edge) - {0})


@functools.lru_cache(maxsize=None)
def dec_items(fs, dtype="float64"):
    """the items of one ragged batch at fs: a 300 Hz harmonic tone on a DC offset plus noise, cut to each length"""
    rng = np.random.default_rng(fs)
    out = []
    for n in dec_lengths(fs):
        f = np.full(n, 300.0)
        x = 0.2 + R._harm(f, fs) + 1e-3 * rng.standard_normal(n)
        out.append(_frozen(x.astype(dtype)))
    return out


@functools.lru_cache(maxsize=None)
def dec_ref(fs, dtype="float64"):
    return [_frozen(R.decimate(x.astype(np.float64), fs)[0]) for x in dec_items(fs, dtype)]


# ------------------------------------------------------------------------------------------------ 2. raw candidates
RAW_RANGE = (196.0, 700.0)
RAW_LENGTHS = (3, 255, 256, 257, 258, 513, 1024)


@functools.lru_cache(maxsize=None)
def raw_items():
    """analysis signals (what the decimator would hand on at ratio 1: zero mean) of a 400 -> 500 Hz glide plus noise"""
    rng = np.random.default_rng(21)
    out = []
    for n in RAW_LENGTHS:
        x = R._harm(np.linspace(400.0, 500.0, n), FS8, n_harm=3) + 1e-3 * rng.standard_normal(n)
        out.append(_frozen(R.decimate(x, FS8)[0]))
    return out


@functools.lru_cache(maxsize=None)
def raw_ref():
    """per item (raw (n_ch, F1), near (n_ch, F1))"""
    return [tuple(_frozen(a) for a in R.raw_candidates(y, float(FS8), *RAW_RANGE, R.frame_count(len(y), FS8, 1.0)))
            for y in raw_items()]


# ------------------------------------------------------------------------------------------------ 4. official + overlap
OFF_BATCHES = ((257, 7), (4, 2), (3, 1))  # frame counts of the items of each B = 2 batch
RUN_LENGTHS = (3, 9, 10, 11, 25)
MINIMAL_RANGE = (400.0, 401.0)  # 12 channels, one base candidate


def _tile_frame(rng, n_ch, boundary):
    """one frame's raw candidates: channels 1 .. n_ch - 2 tiled with runs of RUN_LENGTHS separated by 1-3 zeros"""
    col = np.zeros(n_ch)
    j = 1 + int(rng.integers(0, 3))
    runs = []
    while j < n_ch - 1:
        L = int(rng.choice(RUN_LENGTHS))
        end = min(j + L, n_ch - 1)
        col[j:end] = boundary[j:end] * (1.0 + 0.05 * rng.standard_normal(end - j))
        runs.append(end - j)
        j = end + 1 + int(rng.integers(0, 3))
    return col, runs


@functools.lru_cache(maxsize=None)
def synthetic_raw(F1, seed):
    """(raw (n_ch, F1) at the default geometry, list of the run lengths of each frame).  Frame 0 of every item is
    hand-made when F1 allows, the others are random tilings:
      0: 13 runs of exactly 10 separated by one zero, from channel 1 on (the most runs 150 channels can hold)
      1: a run 1 .. 10 (starts at channel 1) and a run 141 .. 150 (ends at channel 150)
      2: channels 0 .. 9 and 142 .. 151 set: runs that reach 10 only by counting the ignored channels 0 and 151
      3: a run of 25 broken by a negative entry into 12 + 12, and one of 21 broken by a zero into 10 + 10"""
    g = R.geometry(FS8)
    n_ch, bd = g["n_ch"], g["boundary"]
    rng = np.random.default_rng(seed)
    raw, runs = np.zeros((n_ch, F1)), []
    for fr in range(F1):
        raw[:, fr], r = _tile_frame(rng, n_ch, bd)
        runs.append(r)
    hand = np.zeros((n_ch, 4))
    for k in range(13):
        hand[1 + 11 * k:11 + 11 * k, 0] = bd[1 + 11 * k:11 + 11 * k]
    hand[1:11, 1], hand[141:151, 1] = bd[1:11], bd[141:151]
    hand[0:10, 2], hand[142:152, 2] = bd[0:10], bd[142:152]
    hand[20:45, 3], hand[60:81, 3] = bd[20:45], bd[60:81]
    hand[32, 3], hand[70, 3] = -bd[32], 0.0
    hand_runs = [[10] * 13, [10, 10], [9, 9], [12, 12, 10, 10]]
    for k in range(min(4, F1)):
        raw[:, k], runs[k] = hand[:, k], hand_runs[k]
    return _frozen(raw), runs


@functools.lru_cache(maxsize=None)
def minimal_raw():
    """(12, 2) at MINIMAL_RANGE: frame 0 has channels 1 .. 10 set (the one possible run of 10), frame 1 channels 1 .. 9"""
    g = R.geometry(FS8, *MINIMAL_RANGE)
    assert g["n_ch"] == 12 and g["n_base"] == 1
    raw = np.zeros((12, 2))
    raw[1:11, 0] = g["boundary"][1:11]
    raw[1:10, 1] = g["boundary"][1:10]
    return _frozen(raw)


def official_ref(raw):
    return _frozen(R.official_candidates(np.asarray(raw)))


# ------------------------------------------------------------------------------------------------ 5. refinement
REF_N = (8000, 100)  # samples of the two items (1001 and 13 frames)
# [start, end) in samples, Hz, harmonics
REF_TONES = ((0, 2000, 72.0, 6), (2000, 4000, 385.0, 6), (4000, 6000, 665.0, 6), (6000, 8000, 385.0, 1))


@functools.lru_cache(maxsize=None)
def refine_signals():
    """item 0: three stretches of a six-harmonic tone (72, 385, 665 Hz) and one of a pure 385 Hz sine, plus noise;
    item 1: 100 samples of 100 Hz"""
    rng = np.random.default_rng(31)
    x = np.zeros(REF_N[0])
    for a, b, f, h in REF_TONES:
        x[a:b] = R._harm(np.full(b - a, f), FS8, n_harm=h)
    x = x + 1e-3 * rng.standard_normal(len(x))
    s = R._harm(np.full(REF_N[1], 100.0), FS8, n_harm=6) + 1e-3 * rng.standard_normal(REF_N[1])
    return _frozen(R.decimate(x, FS8)[0]), _frozen(R.decimate(s, FS8)[0])


# group name -> (item, frame, candidate Hz); the column is the position in this table modulo the row's free columns
REF_GROUPS = {
    "edges": [(0, 0, 72.0), (0, 1, 72.5), (0, 999, 385.0), (0, 1000, 384.0), (0, 375, 385.0)],
    "floor": [(0, 100, 71.0), (0, 101, 71.2), (0, 120, 71.05)],               # 341-sample window
    "window65": [(0, 300, 376.0), (0, 301, 380.0), (0, 302, 387.0)],          # hw 32: 65 samples, two lane trips
    "window63": [(0, 303, 387.2), (0, 304, 388.0), (0, 305, 395.0)],          # hw 31: 63 samples, one lane trip
    "harmonics": [(0, 600, 660.0), (0, 601, 666.0), (0, 602, 666.7), (0, 603, 670.0)],  # 6, 6, 5, 5 harmonics
    "far": [(0, 875, 122.5)],  # on the pure sine: refined inside the range, score 2.01 < 2.5, so the output is zero
    "clamped": [(1, 6, 100.0), (1, 0, 100.5), (1, 12, 99.5)],                  # 243-sample window in 100 samples
}


@functools.lru_cache(maxsize=None)
def refine_cand():
    """per item the hand-placed candidate table (F1, 105)"""
    C = R.geometry(FS8)["n_cand"]
    out = [np.zeros((R.frame_count(n, FS8, 1.0), C)) for n in REF_N]
    for _, item, fr, f, col in refine_entries():
        out[item][fr, col] = f
    return [_frozen(a) for a in out]


@functools.lru_cache(maxsize=None)
def refine_ref():
    """per item (refined, score, near)"""
    g = R.geometry(FS8)
    return [tuple(_frozen(a) for a in R.refine(y, float(FS8), c, 71.0, 800.0))
            for y, c in zip(refine_signals(), refine_cand())]


def refine_entries():
    """[(group, item, frame, candidate Hz, column)] of the hand-placed candidates, in table order"""
    C, out = R.geometry(FS8)["n_cand"], []
    for name, group in REF_GROUPS.items():
        for item, fr, f in group:
            out.append((name, item, fr, f, (7 * len(out)) % C))
    return out


# ------------------------------------------------------------------------------------------------ 6. contour
CONTOUR_BATCHES = ((1500, 700, 257), (3, 1, 2))  # frame counts of the items of each B = 3 batch
SECTION_LENGTHS = (41, 29, 30, 31, 32, 33, 46, 120, 38)  # candidate frames; step 1 always takes a section's first frame
GAPS = (8, 9, 10, 14, 8, 9, 10, 23)                      # empty frames between two sections
DROPOUTS = (3, 4, 5)  # empty frames from frame 100 of the 120-frame sections: the rest stands only if step 3 bridges them


def _walk(rng, n, f):
    """a smooth random walk of n frames from f: within +-0.4 % per frame"""
    return f * np.cumprod(1.0 + 0.004 * rng.uniform(-1.0, 1.0, n))


def _put_track(rng, cand, score, t0, f, s):
    """the track f with scores s from frame t0 on, in three of the free columns of every frame"""
    C = cand.shape[1]
    for i in range(len(f)):
        free = np.nonzero(cand[t0 + i] == 0.0)[0]
        cols = rng.choice(free, size=3, replace=False)
        cand[t0 + i, cols], score[t0 + i, cols] = f[i], s[i]


@functools.lru_cache(maxsize=None)
def contour_input(F1, seed):
    """(refined (F1, 105), score (F1, 105)) written as the refinement would leave them.  From frame seed % 3 on:
    two crossing blocks (a track A and, 25 % above it, a track B that starts before A ends and outscores it from a
    switch frame on: late in the first block, early in the second, so that the overlap merge goes once each way),
    then sections of SECTION_LENGTHS separated by GAPS, the 120-frame ones with a dropout of DROPOUTS that leaves a tail too short to stand alone;
    the last section runs to the end; every third section has an octave competitor that outscores it on single frames 35 apart; stray candidates at 1 %
    of the frames.  The end is frame F1 - 1 (even seed) or F1 - 2 (odd seed)."""
    rng = np.random.default_rng(1000 + seed)
    C = R.geometry(FS8)["n_cand"]
    cand, score = np.zeros((F1, C)), np.zeros((F1, C))
    last = F1 - 1 - seed % 2
    t = seed % 3
    if F1 <= 3:
        for i in range(t if t < F1 else 0, F1):
            _put_track(rng, cand, score, i, np.array([200.0 + i]), np.array([20.0]))
        return _frozen(cand), _frozen(score)
    for m in (85, 58) if F1 >= 700 else ():
        fa, fb = _walk(rng, 100, rng.uniform(150.0, 250.0)), None
        fb = _walk(rng, 90, 1.25 * fa[50])
        ia, ib = np.arange(100), np.arange(50, 140)
        _put_track(rng, cand, score, t, fa, np.where(ia < m, 30.0, 10.0) + rng.uniform(0, 1, 100))
        _put_track(rng, cand, score, t + 50, fb, np.where(ib < m, 10.0, 30.0) + rng.uniform(0, 1, 90))
        t += 140 + 12
    k = d = 0
    while t <= last:
        n = min(SECTION_LENGTHS[k % len(SECTION_LENGTHS)], last - t + 1)
        if last - (t + n - 1) < GAPS[k % len(GAPS)] + 12:  # no room for another section: this one runs to the end
            n = last - t + 1
        f = _walk(rng, n, rng.uniform(120.0, 400.0))
        s = rng.uniform(10.0, 50.0, n)
        live = np.ones(n, dtype=bool)
        if n == 120:
            drop = DROPOUTS[d % len(DROPOUTS)]
            live[100:100 + drop] = False
            d += 1
        for i0 in np.nonzero(np.diff(np.concatenate([[0], live.astype(int), [0]])) == 1)[0]:
            i1 = i0 + int(np.argmin(np.concatenate([live[i0:], [False]])))
            _put_track(rng, cand, score, t + i0, f[i0:i1], s[i0:i1])
        if k % 3 == 2:
            for i in range(35, n - 1, 35):
                if live[i]:
                    col = int(rng.choice(np.nonzero(cand[t + i] == 0.0)[0]))
                    cand[t + i, col], score[t + i, col] = 2.0 * f[i], 60.0
        t += n + GAPS[k % len(GAPS)]
        k += 1
    for i in np.nonzero(rng.random(F1) < 0.01)[0]:
        col = int(rng.choice(np.nonzero(cand[i] == 0.0)[0]))
        cand[i, col], score[i, col] = rng.uniform(80.0, 700.0), rng.uniform(5.0, 80.0)
    return _frozen(cand), _frozen(score)


@functools.lru_cache(maxsize=None)
def contour_ref(F1, seed):
    c = R.contour(*(np.asarray(a) for a in contour_input(F1, seed)), 71.0, 1.0)
    for v in c.values():
        if isinstance(v, np.ndarray):
            _frozen(v)
    return c


def contour_seed(batch, i):
    """the seed of item i of a batch: start frames 0, 1, 2 and both last frames occur over the items"""
    return ((0, 1, 5), (6, 7, 8))[batch][i]
