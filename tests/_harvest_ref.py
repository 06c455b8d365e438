"""float64 numpy + scipy restatement of WORLD's Harvest F0 estimator (harvest.cpp, Morise 2017) as `pyworld.harvest`
calls it: the contract serenade_amd/harvest.py and serenade_amd/csrc/harvest.hip are tested against.  pyworld is not
installed where this project is tested and WORLD's source is not available, so this file was written from recollection
of harvest.cpp and is the pin ("parity unpinned", like tests/_pyin_ref.py).  Only two constants could be checked:
the smoothing filter is scipy.signal.butter(2, 0.06) and the decimation filter is scipy.signal.cheby1(3, 0.05, 0.8 / r).

Stages (each callable on its own, each fed by the previous one):
    decimate             GetWaveformAndSpectrum + decimate: edge extension, zero-phase Chebyshev, pick, mean removal
    raw_candidates       GetRawF0Candidates: per channel the band-pass, four kinds of events, interp1, the average
    official_candidates  DetectOfficialF0Candidates + OverlapF0Candidates
    refine               RefineF0Candidates (GetRefinedF0: instantaneous frequency at up to 6 harmonics, direct DFT)
    contour              RemoveUnreliableCandidates, FixF0Contour (steps 1-4), SmoothF0Contour, the frame-period pick
    harvest              all of it

Pinned here where WORLD leaves it to a library or where this file departs from it (harvest.hip follows):
  - the band-pass is a direct linear convolution (WORLD: an FFT long enough to rule out wrap-around; the same sum);
  - the spectra of the refinement are a direct DFT of the <= 6 bins that are read, with the phase reduced to
    (bin * n) mod fft_size before the cosine (WORLD: an FFT);
  - the smoothing pads each voiced section with its edge values over 300 frames on both sides (WORLD pads over the
    whole 300-frame-extended contour; the filter's poles have radius 0.875, so 300 frames are a steady state to
    below 1e-17 relative);
  - the candidate table always has matlab_round(n_ch / 10) * 7 columns (WORLD sizes it by the largest number of
    candidates any frame has; the extra columns are zero and no step can select a zero);
  - MergeF0 starts from the section with the earliest start (WORLD: from section 0, which is the same section unless
    a backward extension overtakes an earlier section).

Near-ties: every threshold decision whose two sides are within NEAR (1e-9 relative) of each other is reported; a
rounding difference of the GPU's sums or of its cos may legitimately flip only these.
"""
import numpy as np
import scipy.signal

from oracle.world_oracle import matlab_round

# ---- constants of harvest.cpp, all from recollection except where noted
CHANNELS_IN_OCTAVE = 40.0
FLOOR_FACTOR, CEIL_FACTOR = 0.9, 1.1  # adjusted search range
TARGET_FS = 8000.0  # decimation target
MAX_RATIO = 12
DECIMATE_LAG_SAMPLES = 140.0  # edge extension before decimation
DECIMATE_NFACT = 9  # reflected samples of MATLAB-style decimate
DECIMATE_ORDER, DECIMATE_RIPPLE, DECIMATE_CUTOFF = 3, 0.05, 0.8  # verified: WORLD's table == cheby1(3, 0.05, 0.8 / r)
NUTTALL = (0.355768, 0.487396, 0.144232, 0.012604)
FILTER_PERIODS = 2.0  # half length of a channel's band-pass in periods of its boundary F0
CHANNEL_BAND = (0.9, 1.1)  # a raw candidate must lie this close to its channel
MIN_INTERVALS = 2  # a kind of event needs MORE than this many intervals
MIN_RUN = 10  # channels in a row that make an official candidate
OVERLAP_FRAMES = 3  # neighbours on each side whose candidates a frame takes
REFINE_WINDOW_PERIODS = 1.5
MAX_HARMONICS = 6
SCORE_THRESHOLD = 2.5
SAFEGUARD = 1e-12
REMOVE_RANGE = 0.05
STEP1_RANGE = 0.1
STEP3_RANGE = 0.18
EXTEND_FRAMES, EXTEND_MISSES = 100, 4
EXTEND_MEAN_RULE = 2200.0
STEP4_GAP = 9
SMOOTH_PAD = 300
SMOOTH_ORDER, SMOOTH_CUTOFF = 2, 0.06  # verified: WORLD's table == butter(2, 0.06)
NEAR = 1e-9


# ------------------------------------------------------------------------------------------------ geometry and tables
def geometry(fs, f0_floor=71.0, f0_ceil=800.0):
    ratio = max(min(matlab_round(fs / TARGET_FS), MAX_RATIO), 1)
    actual_fs = fs / ratio
    lo, hi = f0_floor * FLOOR_FACTOR, f0_ceil * CEIL_FACTOR
    n_ch = 1 + int(np.log2(hi / lo) * CHANNELS_IN_OCTAVE)
    boundary = np.array([lo * 2.0 ** ((i + 1) / CHANNELS_IN_OCTAVE) for i in range(n_ch)])
    base = matlab_round(n_ch / 10.0)
    return dict(ratio=ratio, actual_fs=actual_fs, n_ch=n_ch, boundary=boundary, n_base=base,
                n_cand=base * (2 * OVERLAP_FRAMES + 1), voice_range_minimum=int(0.5 + 1000.0 / f0_floor) * 2 + 1,
                half_len=[matlab_round(actual_fs / b * FILTER_PERIODS) for b in boundary])


def frame_count(n, fs, frame_period):
    return int(1000.0 * n / fs / frame_period) + 1


def nuttall(n):
    t = np.arange(n) / (n - 1.0)
    a = NUTTALL
    return a[0] - a[1] * np.cos(2.0 * np.pi * t) + a[2] * np.cos(4.0 * np.pi * t) - a[3] * np.cos(6.0 * np.pi * t)


def channel_taps(boundary_f0, actual_fs):
    """GetFilteredSignal's band-pass: Nuttall window x cosine at the channel's boundary F0"""
    hl = matlab_round(actual_fs / boundary_f0 * FILTER_PERIODS)
    k = np.arange(-hl, hl + 1)
    return nuttall(2 * hl + 1) * np.cos(2.0 * np.pi * boundary_f0 * k / actual_fs)


def _round_arr(x):
    return np.where(x > 0, np.trunc(x + 0.5), np.trunc(x - 0.5)).astype(np.int64)


def _near(a, b):
    """a decision between a and b is a near-tie"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (np.abs(a - b) <= NEAR * np.maximum(np.abs(a), np.abs(b)))


# ------------------------------------------------------------------------------------------------ decimation
def _df2(x, b, a):
    """order-3 direct form II from zero state, in this order of operations"""
    w0 = w1 = w2 = 0.0
    b0, b1, b2, b3 = (float(v) for v in b)
    a1, a2, a3 = float(a[1]), float(a[2]), float(a[3])
    y = np.empty(len(x))
    for i, v in enumerate(x.tolist()):
        wt = ((v - a1 * w0) - a2 * w1) - a3 * w2
        y[i] = ((b0 * wt + b1 * w0) + b2 * w1) + b3 * w2
        w2, w1, w0 = w1, w0, wt
    return y


def matlab_decimate(x, r):
    nf = DECIMATE_NFACT
    b, a = scipy.signal.cheby1(DECIMATE_ORDER, DECIMATE_RIPPLE, DECIMATE_CUTOFF / r)
    n = len(x)
    t = np.concatenate([2 * x[0] - x[nf:0:-1], x, 2 * x[-1] - x[n - 2:n - 2 - nf:-1]])
    t = _df2(t, b, a)[::-1]
    t = _df2(t, b, a)[::-1]
    nout = (n - 1) // r + 1
    nbeg = r - r * nout + n
    return t[nf + nbeg - 1:nf + n:r][:nout]


def decimate(x, fs):
    """(y, actual_fs): the zero-mean analysis signal at fs / ratio"""
    x = np.asarray(x, dtype=np.float64)
    ratio = geometry(fs)["ratio"]
    y_len = -(-len(x) // ratio)
    if ratio == 1:
        y = x.copy()
    else:
        lag = int(np.ceil(DECIMATE_LAG_SAMPLES / ratio) * ratio)
        ext = np.concatenate([np.full(lag, x[0]), x, np.full(lag, x[-1])])
        y = matlab_decimate(ext, ratio)[lag // ratio:lag // ratio + y_len]
    return y - np.mean(y), fs / ratio


# ------------------------------------------------------------------------------------------------ raw candidates
def filtered_signal(y, boundary_f0, actual_fs):
    h = channel_taps(boundary_f0, actual_fs)
    hl = len(h) // 2
    return np.convolve(y, h)[hl + 1:hl + 1 + len(y)] if len(y) > 0 else y


def _events(v):
    """ZeroCrossingEngine: fine positions of the negative-going zero crossings of v"""
    if len(v) < 2:
        return np.zeros(0)
    i = np.nonzero((v[:-1] > 0.0) & (v[1:] <= 0.0))[0]
    return (i + 1) - v[i] / (v[i + 1] - v[i])


def _interp1(x, y, xi):
    """matlabfunctions.cpp interp1 with histc: linear, extrapolating from the first and the last segment"""
    k = np.clip(np.searchsorted(x, xi, side="right") - 1, 0, len(x) - 2)
    s = (xi - x[k]) / (x[k + 1] - x[k])
    return y[k] + s * (y[k + 1] - y[k])


def _sign_ties(v):
    """samples of the edge detector's input v whose sign test is a near-tie: within NEAR of zero relative to v's peak.
    Where v crosses zero there (its neighbours lie clearly on opposite sides), both outcomes of the test put an edge
    at the same place to within the perturbation (the interpolated crossing is continuous in v), so only the samples
    where v touches zero without a clear crossing, or that sit at an end, are reported."""
    if len(v) == 0:
        return np.zeros(0, dtype=np.int64)
    lim = NEAR * np.abs(v).max()
    i = np.nonzero((np.abs(v) > 0) & (np.abs(v) <= lim))[0]
    inner = i[(i > 0) & (i < len(v) - 1)]
    crossing = np.zeros(len(i), dtype=bool)
    a, b = v[inner - 1], v[inner + 1]
    crossing[(i > 0) & (i < len(v) - 1)] = (a * b < 0) & (np.abs(a) > lim) & (np.abs(b) > lim)
    return i[~crossing]


def _tie_frames(ties, events, actual_fs, n_frames):
    """frames whose interpolation a flipped sign test at one of the samples `ties` could reach: an edge that appears
    or vanishes there changes the intervals up to the neighbouring events, and interp1 reads two intervals, so
    everything between the third event before and the third after (to the signal's end where there is none)"""
    flag = np.zeros(n_frames, dtype=bool)
    pos = np.arange(n_frames) / 1000.0 * actual_fs
    for i in ties:
        for e in events:
            if len(e) - 1 <= MIN_INTERVALS + 1:
                return np.ones(n_frames, dtype=bool)  # the flip could also decide whether the channel counts at all
            p = int(np.searchsorted(e, i))
            lo = e[p - 3] if p - 3 >= 0 else -np.inf
            hi = e[p + 2] if p + 2 < len(e) else np.inf
            flag |= (pos >= lo) & (pos <= hi)
    return flag


def raw_candidates_channel(y, actual_fs, boundary_f0, f0_floor, f0_ceil, n_frames):
    """(candidate per 1 ms frame, near-tie flag per frame)"""
    f = filtered_signal(y, boundary_f0, actual_fs)
    g = -f
    d = g[:-1] - g[1:]
    events = [_events(v) for v in (f, g, d, -d)]
    ties = np.concatenate([_sign_ties(f), _sign_ties(d)])
    flag = _tie_frames(ties, events, actual_fs, n_frames) if len(ties) else np.zeros(n_frames, dtype=bool)
    if any(len(e) - 1 <= MIN_INTERVALS for e in events):
        return np.zeros(n_frames), flag
    t = np.arange(n_frames) / 1000.0
    sets = [_interp1((e[:-1] + e[1:]) / 2.0 / actual_fs, actual_fs / (e[1:] - e[:-1]), t) for e in events]
    c = (((sets[0] + sets[1]) + sets[2]) + sets[3]) / 4.0
    lims = (boundary_f0 * CHANNEL_BAND[1], boundary_f0 * CHANNEL_BAND[0], f0_ceil, f0_floor)
    for lim in lims:
        flag = flag | _near(c, lim)
    out = (c > lims[0]) | (c < lims[1]) | (c > lims[2]) | (c < lims[3])
    return np.where(out, 0.0, c), flag


def raw_candidates(y, actual_fs, f0_floor, f0_ceil, n_frames):
    """(raw (n_ch, n_frames), near (n_ch, n_frames))"""
    g = geometry(actual_fs, f0_floor, f0_ceil)  # ratio is not used below
    res = [raw_candidates_channel(y, actual_fs, b, f0_floor, f0_ceil, n_frames) for b in g["boundary"]]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def material(raw, near):
    """(n_ch, n_frames): the near-tie flags of raw candidates that can reach an official candidate.  With every flagged
    entry counted as a possible candidate, an entry in a run of fewer than MIN_RUN channels (first and last channel
    excluded) cannot be part of an official candidate whichever way its decision falls, and the zeros that bound the
    run are not flagged, so no other run changes either."""
    n_ch, F = raw.shape
    p = (raw > 0) | near
    p[0] = p[n_ch - 1] = False
    run = np.zeros((n_ch, F), dtype=np.int64)
    for j in range(1, n_ch):  # run length ending at j, then spread backwards
        run[j] = np.where(p[j], run[j - 1] + 1, 0)
    for j in range(n_ch - 2, -1, -1):
        run[j] = np.where(p[j] & p[j + 1], run[j + 1], run[j])
    return near & (run >= MIN_RUN)


# ------------------------------------------------------------------------------------------------ official + overlap
def official_candidates(raw):
    """(n_frames, n_cand): means over runs of >= MIN_RUN channels (first and last channel ignored), then the
    candidates of the frames +-1 .. +-3"""
    n_ch, F = raw.shape
    base = matlab_round(n_ch / 10.0)
    off = np.zeros((F, base))
    count = np.zeros(F, dtype=np.int64)
    run = np.zeros(F, dtype=np.int64)
    acc = np.zeros(F)
    rows = np.arange(F)
    for j in range(1, n_ch):
        v = (raw[j] > 0) if j < n_ch - 1 else np.zeros(F, dtype=bool)
        end = ~v & (run >= MIN_RUN)
        off[rows[end], count[end]] = acc[end] / run[end]
        count[end] += 1
        acc = np.where(v, np.where(run > 0, acc + raw[j], 0.0 + raw[j]), 0.0)
        run = np.where(v, run + 1, 0)
    n = OVERLAP_FRAMES
    cand = np.zeros((F, base * (2 * n + 1)))
    cand[:, :base] = off
    for i in range(1, n + 1):
        cand[i:, base * i:base * (i + 1)] = off[:F - i] if F > i else 0
        cand[:max(F - i, 0), base * (i + n):base * (i + n + 1)] = off[i:]
    return cand


# ------------------------------------------------------------------------------------------------ refinement
def refine(y, actual_fs, cand, f0_floor, f0_ceil):
    """(refined, score, near), each (n_frames, n_cand): GetRefinedF0 of every candidate at its frame's time"""
    fs = actual_fs
    F, C = cand.shape
    refined, score, near = np.zeros((F, C)), np.zeros((F, C)), np.zeros((F, C), dtype=bool)
    fi, ci = np.nonzero(cand > 0.0)
    if len(fi) == 0 or len(y) == 0:
        return refined, score, near
    f0_all = cand[fi, ci]
    hw_all = (REFINE_WINDOW_PERIODS * fs / f0_all + 1.0).astype(np.int64)
    for hw in np.unique(hw_all):
        sel = hw_all == hw
        f0, pos = f0_all[sel], fi[sel] / 1000.0
        W = 2 * int(hw) + 1
        wlen = (2.0 * hw + 1.0) / fs
        N = 2 ** (2 + int(W).bit_length() - 1)
        idx = _round_arr((pos + (-hw) / fs) * fs + 0.001)[:, None] + np.arange(W)[None, :]
        tmp = (idx - 1.0) / fs - pos[:, None]
        main = 0.42 + 0.5 * np.cos(2.0 * np.pi * tmp / wlen) + 0.08 * np.cos(4.0 * np.pi * tmp / wlen)
        diff = np.empty_like(main)
        diff[:, 0] = -main[:, 1] / 2.0
        diff[:, 1:-1] = -(main[:, 2:] - main[:, :-2]) / 2.0
        diff[:, -1] = main[:, -2] / 2.0
        x = y[np.clip(idx - 1, 0, len(y) - 1)]
        xm, xd = x * main, x * diff
        n_harm = np.minimum((fs / 2.0 / f0).astype(np.int64), MAX_HARMONICS)
        num = np.zeros(len(f0))
        den = np.zeros(len(f0))
        sc = np.zeros(len(f0))
        nr = np.zeros(len(f0), dtype=bool)
        for k in range(1, MAX_HARMONICS + 1):
            live = k <= n_harm
            pos_k = f0 * N / fs * k
            nr |= live & (np.abs(pos_k - np.floor(pos_k) - 0.5) <= NEAR * pos_k)
            b = _round_arr(pos_k)
            ang = 2.0 * np.pi * ((b[:, None] * np.arange(W)[None, :]) % N) / N
            c, s = np.cos(ang), np.sin(ang)
            m_re, m_im = (xm * c).sum(1), -(xm * s).sum(1)
            d_re, d_im = (xd * c).sum(1), -(xd * s).sum(1)
            numer = m_re * d_im - m_im * d_re
            power = m_re * m_re + m_im * m_im
            with np.errstate(divide="ignore", invalid="ignore"):
                inst = np.where(power == 0.0, 0.0, b * fs / N + numer / power * fs / 2.0 / np.pi)
            amp = np.sqrt(power)
            num = np.where(live, num + amp * inst, num)
            den = np.where(live, den + amp * k, den)
            sc = np.where(live, sc + np.abs((inst / k - f0) / f0), sc)
        r = num / (den + SAFEGUARD)
        s = 1.0 / (sc / n_harm + SAFEGUARD)
        nr |= _near(r, f0_floor) | _near(r, f0_ceil) | _near(s, SCORE_THRESHOLD)
        bad = (r < f0_floor) | (r > f0_ceil) | (s < SCORE_THRESHOLD)
        refined[fi[sel], ci[sel]] = np.where(bad, 0.0, r)
        score[fi[sel], ci[sel]] = np.where(bad, 0.0, s)
        near[fi[sel], ci[sel]] = nr
    return refined, score, near


# ------------------------------------------------------------------------------------------------ contour
class _Ties:
    def __init__(self):
        self.n = 0

    def see(self, a, b):
        self.n += int(np.count_nonzero(_near(np.asarray(a, dtype=np.float64), b)))


def _select_best(ref, cands, allowed, ties=None):
    """SelectBestF0: the nearest candidate within allowed (relative to ref), the last one of equals; 0 if none"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tmp = np.abs(ref - cands) / ref
    if ties is not None:
        ties.see(tmp, allowed)
    ok = np.nonzero(tmp <= allowed)[0]
    if len(ok) == 0:
        return 0.0, allowed
    m = tmp[ok].min()
    return float(cands[ok[tmp[ok] == m][-1]]), float(m)


def remove_unreliable(cand, score, ties=None):
    F, C = cand.shape
    out_c, out_s = cand.copy(), score.copy()
    for i0 in range(1, F - 1, 256):
        i1 = min(i0 + 256, F - 1)
        ref = cand[i0:i1, :, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            e1 = np.minimum((np.abs(ref - cand[i0 + 1:i1 + 1, None, :]) / ref).min(2), 1.0)
            e2 = np.minimum((np.abs(ref - cand[i0 - 1:i1 - 1, None, :]) / ref).min(2), 1.0)
        err = np.minimum(e1, e2)
        live = cand[i0:i1] != 0.0
        if ties is not None:
            ties.see(err[live], REMOVE_RANGE)
        drop = live & ~(err <= REMOVE_RANGE)
        out_c[i0:i1][drop] = 0.0
        out_s[i0:i1][drop] = 0.0
    return out_c, out_s


def _boundaries(f0):
    n = len(f0)
    vuv = (f0 > 0).astype(np.int64)
    vuv[0] = vuv[n - 1] = 0
    ch = np.nonzero(np.diff(vuv) != 0)[0] + 1
    return [(int(ch[2 * i]), int(ch[2 * i + 1]) - 1) for i in range(len(ch) // 2)]


def _fix_step1(base, ties):
    F = len(base)
    out = np.zeros(F)
    for i in range(2, F):
        if base[i] == 0.0:
            continue
        ref = base[i - 1] * 2 - base[i - 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            e1 = np.abs((base[i] - ref) / ref)
            e2 = np.abs(base[i] - base[i - 1]) / base[i - 1]
        ties.see([e1, e2], STEP1_RANGE)
        out[i] = 0.0 if (e1 > STEP1_RANGE and e2 > STEP1_RANGE) else base[i]
    return out


def _fix_step2(f0, vrm):
    out = f0.copy()
    for st, ed in _boundaries(f0):
        if ed - st < vrm:
            out[st:ed + 1] = 0.0
    return out


def _extend(ext, F, origin, last, shift, cand, ties):
    tmp_f0 = ext[origin]
    shifted = origin
    count = 0
    for i in range(abs(last - origin) + 1):
        p = origin + shift * i + shift
        ext[p], _ = _select_best(tmp_f0, cand[p], STEP3_RANGE, ties)
        if ext[p] == 0.0:
            count += 1
        else:
            tmp_f0 = ext[p]
            count = 0
            shifted = p
        if count == EXTEND_MISSES:
            break
    return shifted


def _search_score(f0, cands, scores):
    s = scores[cands == f0]
    return float(max(s.max(), 0.0)) if len(s) else 0.0


def _fix_step3(f0, cand, score, ties):
    F = len(f0)
    out = f0.copy()
    secs = []
    for st, ed in _boundaries(f0):
        ext = np.zeros(F)
        ext[st:ed + 1] = f0[st:ed + 1]
        ed2 = _extend(ext, F, ed, min(F - 2, ed + EXTEND_FRAMES), 1, cand, ties)
        st2 = _extend(ext, F, st, max(1, st - EXTEND_FRAMES), -1, cand, ties)
        secs.append((st2, ed2, ext))
    kept = []
    mean_f0 = 0.0  # carried from section to section, as harvest.cpp's ExtendSub does
    for st, ed, ext in secs:
        for j in range(st, ed):
            mean_f0 += ext[j]
        mean_f0 /= ed - st
        if EXTEND_MEAN_RULE / mean_f0 < ed - st:
            kept.append((st, ed, ext))
    if not kept:
        return out
    kept.sort(key=lambda s: s[0])  # stable
    st1, ed1, first = kept[0]
    out = first.copy()
    for st2, ed2, f2 in kept[1:]:
        if st2 - ed1 > 0:
            out[st2:ed2 + 1] = f2[st2:ed2 + 1]
            ed1 = ed2
        elif st1 <= st2 and ed1 >= ed2:
            pass
        else:
            s1 = s2 = 0.0
            for i in range(st2, ed1 + 1):
                s1 += _search_score(out[i], cand[i], score[i])
                s2 += _search_score(f2[i], cand[i], score[i])
            lo = ed1 if s1 > s2 else st2
            out[lo:ed2 + 1] = f2[lo:ed2 + 1]
            ed1 = ed2
    return out


def _fix_step4(f0):
    out = f0.copy()
    b = _boundaries(f0)
    for i in range(len(b) - 1):
        distance = b[i + 1][0] - b[i][1] - 1
        if distance >= STEP4_GAP:
            continue
        tmp0 = f0[b[i][1]] + 1
        tmp1 = f0[b[i + 1][0]] - 1
        coef = (tmp1 - tmp0) / (distance + 1.0)
        count = 1
        for j in range(b[i][1] + 1, b[i + 1][0]):
            out[j] = tmp0 + coef * count
            count += 1
    return out


def _df2_2(x, b, a):
    w0 = w1 = 0.0
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    y = np.empty(len(x))
    for i, v in enumerate(x.tolist()):
        wt = (v - a1 * w0) - a2 * w1
        y[i] = (b0 * wt + b1 * w0) + b2 * w1
        w1, w0 = w0, wt
    return y


def smooth(f0):
    """SmoothF0Contour: every voiced section on its own, padded with its edge values, forward-backward Butterworth"""
    b, a = scipy.signal.butter(SMOOTH_ORDER, SMOOTH_CUTOFF)
    F = len(f0)
    out = np.zeros(F)
    v = np.concatenate([[0], (f0 > 0).astype(np.int64), [0]])
    ch = np.nonzero(np.diff(v) != 0)[0]
    for st, ed in zip(ch[0::2], ch[1::2] - 1):
        x = np.concatenate([np.full(SMOOTH_PAD, f0[st]), f0[st:ed + 1], np.full(SMOOTH_PAD, f0[ed])])
        x = _df2_2(_df2_2(x, b, a)[::-1], b, a)[::-1]
        out[st:ed + 1] = x[SMOOTH_PAD:SMOOTH_PAD + ed - st + 1]
    return out


def contour(cand, score, f0_floor, frame_period=1.0, n_out=None):
    """dict: unsmoothed and smoothed 1 ms contours, the picked f0 at frame_period, and the count of near-ties"""
    ties = _Ties()
    F = cand.shape[0]
    c2, s2 = remove_unreliable(cand, score, ties)
    best = np.argmax(s2, axis=1)  # the first maximum, as SearchF0Base's strict comparison
    base = np.where(s2[np.arange(F), best] > 0.0, c2[np.arange(F), best], 0.0)
    f = _fix_step1(base, ties)
    f = _fix_step2(f, int(0.5 + 1000.0 / f0_floor) * 2 + 1)
    f = _fix_step3(f, c2, s2, ties)
    f = _fix_step4(f)
    sm = smooth(f)
    if n_out is None:
        n_out = int((F - 1) / frame_period) + 1
    t = np.arange(n_out) * frame_period / 1000.0
    pick = np.minimum(F - 1, _round_arr(t * 1000.0))
    return dict(unsmoothed=f, smoothed=sm, f0=sm[pick], ties=ties.n, cand=c2, score=s2)


# ------------------------------------------------------------------------------------------------ the whole
def harvest(x, fs, f0_floor=71.0, f0_ceil=800.0, frame_period=5.0, stages=False):
    """(f0, t, near): pyworld.harvest's f0 and time axis, and whether any decision on the way was a near-tie.
    stages=True returns a dict of every stage's output as well."""
    x = np.asarray(x, dtype=np.float64)
    y, afs = decimate(x, fs)
    F1 = frame_count(len(x), fs, 1.0)
    raw, near_raw = raw_candidates(y, afs, f0_floor, f0_ceil, F1)
    cand = official_candidates(raw)
    refined, score, near_ref = refine(y, afs, cand, f0_floor, f0_ceil)
    n_out = frame_count(len(x), fs, frame_period)
    c = contour(refined, score, f0_floor, frame_period, n_out)
    near = bool(material(raw, near_raw).any() or near_ref.any() or c["ties"] > 0)
    t = np.arange(n_out) * frame_period / 1000.0
    if stages:
        return dict(y=y, actual_fs=afs, raw=raw, near_raw=near_raw, cand=cand, refined=refined, score=score,
                    near_ref=near_ref, contour=c, f0=c["f0"], t=t, near=near)
    return c["f0"], t, near


# ------------------------------------------------------------------------------------------------ test signals
def _harm(f, fs, n_harm=5, amp=0.3):
    """harmonics 1 .. n_harm with 1 / k amplitudes at the instantaneous frequency f (Hz per sample)"""
    ph = 2 * np.pi * np.cumsum(f) / fs
    return sum(amp / k * np.sin(k * ph + 0.3 * k) for k in range(1, n_harm + 1))


def signals(fs=24000, sec=0.5, seed=0, extra=False):
    """name -> (x float64, true f0 per 1 ms frame (0 = unvoiced), frames to check against the truth): the eight
    ground-truth signals; extra=True adds an octave leap, white noise and a 0.02 s item.  Checked frames are voiced
    ones at least 50 ms from any onset, offset or signal edge."""
    rng = np.random.default_rng(seed)
    n = int(sec * fs)
    t = np.arange(n) / fs
    F1 = frame_count(n, fs, 1.0)
    at = np.minimum(np.arange(F1) * fs // 1000, n - 1)  # the sample at each frame's time
    noise = lambda: 1e-3 * rng.standard_normal(n)
    out = {}

    def add(name, f, gate=None, x=None):
        f = np.asarray(f, dtype=np.float64) * np.ones(n)
        g = np.ones(n) if gate is None else gate
        wave = (_harm(np.where(f > 0, f, 100.0), fs) * g if x is None else x)
        truth = (f * g)[at]
        ms = np.arange(F1)
        check = np.zeros(F1, dtype=bool)
        v = np.concatenate([[0], (truth > 0).astype(int), [0]])
        ch = np.nonzero(np.diff(v))[0]
        for st, ed in zip(ch[0::2], ch[1::2]):  # voiced [st, ed) in frames
            check |= (ms >= st + 50) & (ms < ed - 50)
        out[name] = (wave, truth, check)

    for f0 in (110.0, 220.0, 440.0, 740.0):
        add(f"tone{int(f0)}", f0)
        out[f"tone{int(f0)}"] = (out[f"tone{int(f0)}"][0] + noise(),) + out[f"tone{int(f0)}"][1:]
    add("glide", 150.0 + 150.0 * t / sec)
    add("vibrato", 220.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.5 * t)))
    gate = ((t < 0.4 * sec) | (t >= 0.6 * sec)).astype(np.float64)
    add("notes", np.where(t < sec / 2, 220.0, 330.0), gate)
    for k in ("glide", "vibrato", "notes"):
        out[k] = (out[k][0] + noise(),) + out[k][1:]
    add("silence", 0.0, np.zeros(n), x=np.zeros(n))
    if extra:
        add("leap", np.where(t < sec / 2, 150.0, 300.0))
        out["leap"] = (out["leap"][0] + noise(), out["leap"][1], out["leap"][2] & (np.abs(np.arange(F1) - 500 * sec) > 50))
        add("noise", 0.0, np.zeros(n), x=0.1 * rng.standard_normal(n))
        m = int(0.02 * fs)
        out["short"] = (_harm(np.full(m, 180.0), fs), np.full(frame_count(m, fs, 1.0), 180.0),
                        np.zeros(frame_count(m, fs, 1.0), dtype=bool))
    return out



def long_signal(fs=24000, seed=1):
    """6 s: twelve notes of 0.4 s, each followed by 0.1 s of silence; (x, truth per 1 ms frame, frames to check)"""
    rng = np.random.default_rng(seed)
    notes = [220.0, 330.0, 261.6, 392.0, 440.0, 174.6, 293.7, 523.3, 196.0, 349.2, 246.9, 466.2]
    n = int(6.0 * fs)
    t = np.arange(n) / fs
    k = np.minimum((t / 0.5).astype(np.int64), len(notes) - 1)
    gate = ((t - 0.5 * k) < 0.4).astype(np.float64)
    f = np.asarray(notes)[k]
    x = _harm(f, fs) * gate + 1e-3 * rng.standard_normal(n)
    F1 = frame_count(n, fs, 1.0)
    ms = np.arange(F1)
    truth = (f * gate)[np.minimum(ms * fs // 1000, n - 1)]
    check = ((ms % 500) >= 50) & ((ms % 500) < 350) & (ms < 6000)
    return x, truth, check


# largest |f0 - true| / true of this restatement over each signal's checked frames at 24 kHz, (71, 800), 1 ms frames,
# seed 0, as measured; a test's gate is twice this (the margin is for a change of noise seed only)
TRUTH_RECORDED = {"tone110": 1.022e-4, "tone220": 8.988e-5, "tone440": 5.103e-5, "tone740": 4.867e-5,
                  "glide": 2.644e-4, "vibrato": 1.543e-4, "notes": 1.178e-4}
LONG_RECORDED = 1.934e-4  # the same for long_signal()
PARAMETER_SETS = ((71.0, 800.0), (70.0, 1100.0), (196.0, 700.0))
_CACHE = {}


def reference(name, fs=24000, f0_floor=71.0, f0_ceil=800.0):
    """every stage of the restatement on signal `name` of signals(fs, extra=True) at 1 ms frames, computed once"""
    key = (name, fs, f0_floor, f0_ceil)
    if key not in _CACHE:
        if ("signals", fs) not in _CACHE:
            _CACHE[("signals", fs)] = signals(fs, extra=True)
        _CACHE[key] = harvest(_CACHE[("signals", fs)][name][0], fs, f0_floor, f0_ceil, 1.0, stages=True)
    return _CACHE[key]


def truth_error(f0, truth, check):
    """(all checked frames voiced, largest relative error over them)"""
    if not check.any():
        return True, 0.0
    return bool((f0[check] > 0).all()), float((np.abs(f0 - truth) / np.maximum(truth, 1.0))[check].max())
