"""The note decoder and the score tracks on the MI355X (serenade_amd/csrc/notes.hip: srn_note_decode, srn_note_frames;
FramewiseDecoder.decode_batch, estimate_score_batch, extract_features(device_decode=True)) against the host decoder,
the float64 restatement tests/_notes_ref.py and estimate_score.

Decisions (counts, intervals) must equal the host decoder's exactly.  That is a condition on the inputs, asserted for
the inputs used: logits lie on the grid k / 16 with |x| <= 8, where distinct values differ by at least 2e-5 after the
sigmoid and equal values tie on both sides, and every threshold keeps 1e-4 from every sigmoid value of the grid.
Pitches: median mode within 1e-4 semitone of the host decoder (whose fp32 path -- two log2 near 11, a subtraction, a
product near 64, an add -- carries at most about 5e-5); the weighted modes within twice the host decoder's own distance
from the restatement, measured on the test's inputs; every mode within 1e-9 of the restatement.  Every padded batch
is filled past the items with values that would change the result if read."""
import json

import numpy as np
import pytest
import torch

from serenade_amd import preprocess
from serenade_amd.contentvec import ContentVec
from serenade_amd.transcriber import (NOTE_MAX_FRAMES, FramewiseDecoder, TranscriptionModel, estimate_score,
                                      estimate_score_batch, reference_f0_device)

from . import _notes_cases as C
from . import _notes_ref as R
from .test_notes_host import NOTES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = dict(sample_rate=16000, win_length=256, hop_length=64)
THR = C.THRESHOLDS[0]
HI, LO = 2.0, -2.0  # sigmoid 0.88 and 0.12


def _decoder(mode, on_thr=THR, off_thr=THR):
    return FramewiseDecoder(dict(CFG, onset_threshold=on_thr, offset_threshold=off_thr, pitch_sum=mode))


def _on_grid(logits):
    return bool((np.abs(logits) <= 8).all() and (logits * 16 == np.round(logits * 16)).all())


def _device(items, mode, on_thr=THR, off_thr=THR):
    """decode_batch of [(logits (n, 3), f0 (nf,))] as one padded batch -> [(intervals, pitches)] and the raw tensors"""
    B = len(items)
    T, F = max(max(len(l) for l, _ in items), 1), max(max(len(f) for _, f in items), 1)
    logits = torch.full((B, T, 3), 8.0)  # past an item: above every threshold
    f0 = torch.full((B, F), 1e4, dtype=torch.float64)
    for b, (l, f) in enumerate(items):
        logits[b, :len(l)] = torch.from_numpy(np.asarray(l, dtype=np.float32).reshape(-1, 3))
        f0[b, :len(f)] = torch.from_numpy(np.asarray(f, dtype=np.float64))
    raw = _decoder(mode, on_thr, off_thr).decode_batch(logits.to(DEV), [len(l) for l, _ in items], f0.to(DEV),
                                                       [len(f) for _, f in items])
    counts, iv, p = (t.cpu().numpy() for t in raw)
    assert not iv[np.arange(T)[None] >= counts[:, None]].any() and not p[np.arange(T)[None] >= counts[:, None]].any()
    return [(iv[b, :counts[b]].astype(np.int64), p[b, :counts[b]]) for b in range(B)], raw


def _host(logits, f0, mode, on_thr=THR, off_thr=THR):
    p, iv = _decoder(mode, on_thr, off_thr).decode(torch.from_numpy(np.asarray(logits, dtype=np.float32)), f0=f0)
    return np.asarray(iv, dtype=np.int64).reshape(-1, 2), np.asarray([float(v) for v in p], dtype=np.float64)


# ------------------------------------------------------------------------------------------------- random curves
LENGTHS = (2, 3, 63, 64, 65, 255, 256, 257, 400, 523)


@pytest.fixture(scope="module")
def random_items():
    items = [(C.curves(n, seed, ties=seed % 2 == 0), C.contour(n, 50 + seed)) for seed, n in enumerate(LENGTHS)]
    assert all(_on_grid(l) for l, _ in items) and all(C.guard_banded(t) for t in C.THRESHOLDS)
    for _, f in items:  # no frame's float64 pitch within 1e-3 of a half-integer: a median rounds the same everywhere
        assert C.clear_of_half(R.midi_pitch(f[~np.isnan(f)]))
    return items


@pytest.mark.parametrize("mode", C.MODES)
def test_random_curves_against_host_and_restatement(random_items, mode):
    notes = 0
    for thr in C.THRESHOLDS:
        got, _ = _device(random_items, mode, thr, thr)
        host_gap, dev_host, dev_ref = 0.0, 0.0, 0.0
        for (l, f), (iv, p) in zip(random_items, got):
            hiv, hp = _host(l, f, mode, thr, thr)
            riv, rp = R.decode(R.activations(l), f, thr, thr, mode)
            assert iv.tolist() == hiv.tolist() == riv.tolist()
            assert mode != "median" or C.clear_of_half(rp)
            notes += len(iv)
            if len(iv):
                host_gap = max(host_gap, float(np.abs(hp - rp).max()))
                dev_host = max(dev_host, float(np.abs(p - hp).max()))
                dev_ref = max(dev_ref, float(np.abs(p - rp).max()))
        print(f"{mode} thr {thr}: host-restatement {host_gap:.2e}, device-host {dev_host:.2e}, "
              f"device-restatement {dev_ref:.2e}")
        assert dev_ref <= 1e-9
        assert dev_host <= (1e-4 if mode == "median" else 2 * host_gap)
    assert notes > 60


@pytest.mark.parametrize("mode", C.MODES)
def test_the_reference_results(golden, mode):
    d = golden("transcriber_small")
    cfg = json.loads(str(d["config"]))
    assert cfg["onset_threshold"] == cfg["offset_threshold"] == 0.5
    items = [(d[f"ref{i}"].astype(np.float32), d[f"f0_{i}"]) for i in range(2)]
    # the fixture's threshold 0.5 is sigmoid(0): exact here because no logit of the fixture is near 0
    assert min(float(np.abs(l).min()) for l, _ in items) > 1e-3
    got, _ = _device(items, mode, 0.5, 0.5)
    for i, (iv, p) in enumerate(got):
        assert iv.tolist() == d[f"intervals{i}_{mode}"].tolist()
        err = float(np.abs(p - d[f"pitches{i}_{mode}"]).max())
        print(f"item {i} {mode}: {err:.2e} from the fixture")
        if mode == "median":
            assert err <= 1e-4


# ------------------------------------------------------------------------------------------------- edge shapes
def _curve(n, on=(), off=(), fr=None):
    """(n, 3) logits: LO everywhere, the listed (frame, value) pairs set; frames HI unless given"""
    l = np.full((n, 3), LO, dtype=np.float32)
    l[:, 2] = HI if fr is None else fr
    for c, pairs in ((0, on), (1, off)):
        for t, v in pairs:
            l[t, c] = v
    return l


def _edge_items():
    n = 40
    tone = np.full(n, 220.0)
    fr_dip = np.full(n, HI, dtype=np.float32)
    fr_dip[11:13] = [-1.0, -3.0]  # fall at 10, confidence 1 - sigmoid(-3)
    fr_late = np.full(n, HI, dtype=np.float32)
    fr_late[16:18] = LO  # fall at 15
    fr_zero = np.full(n, HI, dtype=np.float32)
    fr_zero[30] = LO  # fall at 29 = nxt - 1: the dip starts at nxt, confidence 0
    long_n = 1200
    nan_seg = tone.copy()
    nan_seg[2:31] = np.nan
    ramp = 200.0 * 2.0 ** (np.arange(long_n) % 37 / 36.0)
    items = {
        "T=1": (_curve(1), tone[:1]),
        "T=2": (_curve(2, on=[(1, HI)]), tone[:2]),
        "T=3": (_curve(3, on=[(1, HI)]), tone[:3]),
        "all below": (_curve(n), tone),
        "open at the end": (_curve(n, on=[(38, HI), (39, HI)]), tone),
        "never exceeds v[0]": (_curve(n, on=[(0, 3.0), (10, HI), (11, 2.5)]), tone),
        "peak at frame 0": (_curve(n, on=[(0, 3.0), (1, HI)]), tone),
        "onset at n-2": (_curve(n, on=[(n - 2, HI)]), tone),
        "onset at n-1": (_curve(n, on=[(n - 1, HI)]), tone),
        "onset+2 >= nxt": (_curve(n, on=[(5, HI), (7, HI)]), tone),
        "io after if": (_curve(n, on=[(2, HI), (30, HI)], off=[(20, HI)], fr=fr_dip), tone),
        "if after io": (_curve(n, on=[(2, HI), (30, HI)], off=[(8, HI)], fr=fr_late), tone),
        "confidence 0": (_curve(n, on=[(2, HI), (30, HI)], fr=fr_zero), tone),
        "tied onsets": (_curve(n, on=[(4, HI), (5, HI), (6, HI), (20, 1.0), (21, HI), (22, HI)]), tone),
        "short contour": (_curve(n, on=[(2, HI), (20, HI)]), tone[:25]),
        "contour ends before the note": (_curve(n, on=[(2, HI), (20, HI)]), tone[:10]),
        "all-NaN segment": (_curve(n, on=[(2, HI), (30, HI)]), nan_seg),
        "segment of 2": (_curve(n, on=[(5, HI), (7, HI)]), 200.0 + np.arange(n)),
        "segment of 64": (_curve(100, on=[(3, HI), (67, HI)]), 200.0 + np.arange(100.0)),
        "segment of 65": (_curve(100, on=[(3, HI), (68, HI)]), 200.0 + np.arange(100.0)),
        "segment over 1024": (_curve(long_n, on=[(3, HI), (1100, HI)]), ramp),
        "no frames": (np.zeros((0, 3), dtype=np.float32), np.zeros(0)),
    }
    return items


@pytest.mark.parametrize("mode", C.MODES)
def test_edge_shapes(mode):
    items = _edge_items()
    assert all(_on_grid(l) for l, _ in items.values()) and C.guard_banded(THR)
    got, raw = _device(list(items.values()), mode)
    want = {"T=1": [], "T=2": [], "T=3": [], "all below": [], "open at the end": [], "never exceeds v[0]": [],
            "peak at frame 0": [], "onset at n-2": [], "onset at n-1": [], "no frames": [],
            "onset+2 >= nxt": [[5, 7], [7, 39]], "io after if": [[2, 21], [30, 39]], "if after io": [[2, 16], [30, 39]],
            "confidence 0": [[2, 30], [30, 39]], "tied onsets": [[4, 21], [21, 39]],
            "segment of 2": [[5, 7], [7, 39]], "segment of 64": [[3, 67], [67, 99]],
            "segment of 65": [[3, 68], [68, 99]], "segment over 1024": [[3, 1100], [1100, 1199]]}
    for (name, (l, f)), (iv, p) in zip(items.items(), got):
        if name in want:
            assert iv.tolist() == want[name], name
        if len(l) == 0:
            continue
        riv, rp = R.decode(R.activations(l), f, THR, THR, mode)
        assert iv.tolist() == riv.tolist(), name
        assert np.abs(p - rp).max(initial=0) <= 1e-9, name
        if mode == "median" or "contour ends" not in name:  # the host's weighted forms cannot take an empty segment
            hiv, hp = _host(l, f, mode)
            assert iv.tolist() == hiv.tolist(), name
            if mode == "median":
                assert np.abs(p - hp).max(initial=0) <= 1e-4, name
    by = dict(zip(items, got))
    assert by["all-NaN segment"][1][0] == 0 and by["contour ends before the note"][1][1] == 0
    assert int(raw[0][list(items).index("no frames")]) == 0


def test_the_length_limit_is_an_error():
    dec = _decoder("median")
    logits = torch.zeros(1, NOTE_MAX_FRAMES + 1, 3, device=DEV)
    f0 = torch.full((1, 8), 220.0, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=str(NOTE_MAX_FRAMES)):
        dec.decode_batch(logits, [NOTE_MAX_FRAMES + 1], f0, [8])
    counts, _, _ = dec.decode_batch(logits[:, :NOTE_MAX_FRAMES], [NOTE_MAX_FRAMES], f0, [8])  # the limit itself runs
    assert int(counts[0]) == 0
    with pytest.raises(ValueError):
        dec.decode_batch(logits[:, :10], [11], f0, [8])


# ------------------------------------------------------------------------------------------------- srn_note_frames
SCORE_CFG = dict(CFG, hop_length=320)  # scale 0.02 against shift 0.01: floor and ceil leave 2k at k = 29 and k = 7


def _frames_device(notes, n_samples, cfg=SCORE_CFG, sr=24000, shiftms=10):
    """estimate_score_batch of [(pitches, intervals)] -> [(midi, lf0)] cut to each item's frames"""
    B, cap = len(notes), max(max(len(p) for p, _ in notes), 1)
    counts = torch.tensor([len(p) for p, _ in notes], dtype=torch.int32)
    iv = torch.full((B, cap, 2), 3, dtype=torch.int32)  # past an item's count: a note that would show
    pt = torch.full((B, cap), 100.0, dtype=torch.float64)
    for b, (p, i) in enumerate(notes):
        if len(p):
            pt[b, :len(p)] = torch.tensor(p, dtype=torch.float64)
            iv[b, :len(p)] = torch.tensor(i, dtype=torch.int32).reshape(-1, 2)
    midi, lf0, frames = estimate_score_batch(counts.to(DEV), iv.to(DEV), pt.to(DEV), n_samples, cfg,
                                             sampling_rate=sr, shiftms=shiftms)
    midi, lf0 = midi.cpu().numpy(), lf0.cpu().numpy()
    for b in range(B):
        assert not midi[b, frames[b]:].any() and not lf0[b, frames[b]:].any()
    return [(midi[b, :frames[b]], lf0[b, :frames[b]]) for b in range(B)]


def test_every_interval_up_to_64_equals_estimate_score():
    pairs = [(a, b) for a in range(64) for b in range(a + 1, 65)]
    n = 24000  # 100 frames: ends beyond frame 50 are clipped, starts beyond it give nothing
    got = _frames_device([([61.5], [[a, b]]) for a, b in pairs], [n] * len(pairs))
    for (a, b), (midi, lf0) in zip(pairs, got):
        m, e = estimate_score([61.5], [[a, b]], n, SCORE_CFG, sampling_rate=24000, shiftms=10)
        assert midi.dtype == m.dtype == np.int32 and np.array_equal(midi, m), (a, b)
        assert np.array_equal(lf0[:, None], e), (a, b)
    by = dict(zip(pairs, got))
    assert np.flatnonzero(by[(29, 30)][0]).tolist() == [57, 58, 59]  # floor(29 * 0.02 / 0.01) = 57, not 58
    assert np.flatnonzero(by[(1, 7)][0])[-1] == 14  # ceil(7 * 0.02 / 0.01) = 15, not 14


def test_score_cases():
    cases = [
        ([60.0, 64.0, 67.0], [[0, 10], [5, 12], [8, 9]], 9600),  # overlapping: the later note wins
        ([60.5, 61.5, 62.5, 0.5], [[0, 2], [2, 4], [4, 6], [6, 8]], 4800),  # half to even: 60, 62, 62, 0
        ([57.0, 69.0], [[0, 3], [3, 6]], 4800),  # 220 and 440 Hz exactly
        ([72.0], [[2, 400]], 2400),  # the end is clipped to n = 10
        ([72.0, 50.0], [[30, 40], [0, 1]], 2400),  # a start at or past n
        ([], [], 2400),  # no note
        ([127.4, 0.0], [[0, 3], [3, 5]], 2399),  # the last MIDI number; n = ceil(9.99..)
    ]
    got = _frames_device([(p, i) for p, i, _ in cases], [n for _, _, n in cases])
    for (p, i, n), (midi, lf0) in zip(cases, got):
        m, e = estimate_score(p, i, n, SCORE_CFG, sampling_rate=24000, shiftms=10) if p else \
            (np.zeros(10, np.int32), np.zeros((10, 1), np.int32))
        rm, rl = R.note_frames(p, i, n, 0.02, 0.01, 24000)
        assert np.array_equal(midi, m) and np.array_equal(lf0[:, None], e), p
        assert np.array_equal(midi, rm) and np.array_equal(lf0, rl), p
    assert got[0][0].tolist() == [60] * 10 + [64] * 6 + [67] * 2 + [64] * 6 + [0] * 16
    assert sorted(set(got[1][0].tolist())) == [0, 60, 62]
    assert sorted(set(got[2][1].tolist())) == [0, 5, 6]
    assert got[3][0].tolist() == [0] * 4 + [72] * 6 and got[4][0].tolist() == [50, 50] + [0] * 8
    for bad in (128.0, 127.5, -0.6):
        with pytest.raises(ValueError, match="0..127"):
            _frames_device([([60.0, bad], [[0, 2], [2, 4]])], [4800])


# ------------------------------------------------------------------------------------------------- raggedness
def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("mode", C.MODES)
def test_a_batch_equals_its_single_calls_bit_for_bit(mode):
    lens = (523, 65, 256, 3, 130)
    items = [(C.curves(n, 7 + n), C.contour(max(n - 5 * (i % 2), 1), n)) for i, n in enumerate(lens)]
    _, (counts, iv, p) = _device(items, mode)
    assert int(counts.sum()) > 10
    dec = _decoder(mode)
    for b, (l, f) in enumerate(items):
        c1, iv1, p1 = dec.decode_batch(torch.from_numpy(l)[None].to(DEV), [len(l)],
                                       torch.from_numpy(f)[None].to(DEV), [len(f)])
        k = int(c1[0])
        assert k == int(counts[b]) and torch.equal(iv1[0, :k], iv[b, :k])
        assert torch.equal(_bits(p1[0, :k]), _bits(p[b, :k]))
    n_samples = [int(n * 64 * 1.5) for n in lens]
    midi, lf0, frames = estimate_score_batch(counts, iv, p, n_samples, CFG, sampling_rate=24000, shiftms=10)
    for b in range(len(lens)):
        m1, l1, f1 = estimate_score_batch(counts[b:b + 1], iv[b:b + 1], p[b:b + 1], n_samples[b:b + 1], CFG,
                                          sampling_rate=24000, shiftms=10)
        assert f1[0] == frames[b] and torch.equal(m1[0, :f1[0]], midi[b, :f1[0]])
        assert torch.equal(l1[0, :f1[0]], lf0[b, :f1[0]])
        k = int(counts[b])
        if k:
            m, e = estimate_score(p[b, :k].tolist(), iv[b, :k].tolist(), n_samples[b], CFG, sampling_rate=24000,
                                  shiftms=10)
            assert np.array_equal(midi[b, :frames[b]].cpu().numpy(), m)
            assert np.array_equal(lf0[b, :frames[b], None].cpu().numpy(), e)


# ------------------------------------------------------------------------------------------------- the dump
def _state(d):
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}


@pytest.fixture(scope="module")
def models(golden):
    dc, dt = golden("contentvec_small"), golden("transcriber_small")
    cv = ContentVec(device=DEV, **json.loads(str(dc["config"]))).load_state_dict(_state(dc))
    midi_config = json.loads(str(dt["config"]))
    return cv, TranscriptionModel(midi_config, device=DEV).load_state_dict(_state(dt)), midi_config


def test_extract_features_on_the_device_equals_the_host_path(models):
    from .test_hip_audio import CONFIG, _songs
    from serenade_amd import audio as A
    cv, tm, midi_config = models
    songs = _songs()
    _, _, x16, lens16 = A.prepare(songs, 24000, CONFIG)
    logits, frames = tm(x16.float(), lengths=lens16)
    act = torch.sigmoid(logits[0, :frames[0], 0]).cpu().numpy()
    # thresholds inside item 0's onset curve, each clear of every activation by 1e-4; the first whose pitches keep
    # 1e-3 from every half-integer is used
    ranked = np.sort(np.unique(act))
    gaps = np.flatnonzero(np.diff(ranked) > 4e-4)
    assert len(gaps)
    order = sorted(gaps, key=lambda g: abs(g - len(ranked) // 2))
    seqs = [NOTES, None]
    done = False
    for g in order[:8]:
        threshold = float((ranked[g] + ranked[g + 1]) / 2)
        mc = dict(midi_config, onset_threshold=threshold)
        host = preprocess.extract_features(songs, 24000, CONFIG, cv, tm, mc, note_seqs=seqs)
        dev = preprocess.extract_features(songs, 24000, CONFIG, cv, tm, mc, note_seqs=seqs, device_decode=True)
        if all(h is None for h in host):
            continue
        counts, iv, p = FramewiseDecoder(mc).decode_batch(logits, frames, *reference_f0_device(x16.float(), lens16, mc))
        if not C.clear_of_half(p.cpu().numpy()):
            continue
        done = True
        assert [h is None for h in host] == [d is None for d in dev]
        for h, d in zip(host, dev):
            if h is None:
                continue
            assert tuple(d) == preprocess.TRACKS
            for k in preprocess.TRACKS:
                assert d[k].dtype == np.float32 and d[k].shape == h[k].shape, k
                assert np.array_equal(d[k], h[k], equal_nan=True), k
        if host[0] is not None:
            T = len(host[0]["midi"])
            want = R.gt_score(NOTES, 0.01)[:T].astype(np.float32)
            assert host[0]["gt_lf0_score"].shape == want.shape and np.array_equal(dev[0]["gt_lf0_score"], want)
        if host[1] is not None:
            assert host[1]["gt_lf0_score"].shape == (len(host[1]["midi"]), 1, 1)
        break
    assert done
    none = preprocess.extract_features(songs, 24000, CONFIG, cv, tm, dict(midi_config, onset_threshold=1.5),
                                       device_decode=True)
    assert none == [None, None]
