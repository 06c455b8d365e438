"""The float64 restatement of the note decoder and of the score tracks (tests/_notes_ref.py) against the host code it
restates (transcriber.FramewiseDecoder, estimate_score) and the reference's recorded results
(tests/golden/transcriber_small.npz); the ground-truth score track against hand-built note lists.  The restatement is
what the GPU entry points are held to (tests/test_hip_notes.py)."""
import json

import numpy as np
import pytest
import torch

from serenade_amd import preprocess
from serenade_amd.transcriber import FramewiseDecoder, estimate_score

from . import _notes_cases as C
from . import _notes_ref as R

CFG = dict(sample_rate=16000, win_length=256, hop_length=64)
# the host decoder follows the reference's float32 from the contour on: two fp32 log2 near 11, a subtraction, a product
# near 64 and an add carry at most about 5e-5 semitone; the weighted forms add the fp32 window, sums and interpolation
MEDIAN_BOUND = 1e-4
WEIGHTED_BOUND = 2e-3


def _host(logits, f0, on_thr, off_thr, mode):
    dec = FramewiseDecoder(dict(CFG, onset_threshold=on_thr, offset_threshold=off_thr, pitch_sum=mode))
    p, iv = dec.decode(torch.from_numpy(logits), f0=f0)
    return np.asarray(iv, dtype=np.int64).reshape(-1, 2), np.asarray([float(v) for v in p], dtype=np.float64)


@pytest.mark.parametrize("mode", C.MODES)
def test_restatement_equals_the_host_decoder_on_random_curves(mode):
    notes, worst = 0, 0.0
    for seed in range(40):
        n = (3, 17, 64, 65, 200, 257, 400, 523)[seed % 8]
        logits, f0 = C.curves(n, seed, ties=seed % 2 == 0), C.contour(n, 100 + seed)
        thr = C.THRESHOLDS[seed % 3]
        iv, p = R.decode(R.activations(logits), f0, thr, thr, mode)
        hiv, hp = _host(logits, f0, thr, thr, mode)
        assert iv.tolist() == hiv.tolist(), seed
        notes += len(iv)
        if len(iv):
            worst = max(worst, float(np.abs(p - hp).max()))
    print(f"{mode}: {notes} notes, host against the restatement {worst:.2e} semitone")
    assert notes > 100
    assert worst <= (MEDIAN_BOUND if mode == "median" else WEIGHTED_BOUND)


def test_ties_are_present_and_break_to_the_first():
    assert R.peaks(np.float32([0.1, 0.9, 0.9, 0.2]), 0.5).tolist() == [1]
    assert R.peaks(np.float32([0.9, 0.9, 0.2, 0.95, 0.2]), 0.5).tolist() == [3]  # frame 0 is never a peak
    assert R.peaks(np.float32([0.7, 0.6, 0.2]), 0.5).tolist() == []  # the run never exceeds v[0]
    assert R.peaks(np.float32([0.1, 0.6, 0.7]), 0.5).tolist() == []  # open at the end
    act = R.activations(C.curves(400, 0, ties=True))
    assert (np.diff(act[:, 0]) == 0).sum() > 20


@pytest.mark.parametrize("mode", C.MODES)
def test_restatement_against_the_reference_results(golden, mode):
    d = golden("transcriber_small")
    cfg = json.loads(str(d["config"]))
    for i in range(2):
        iv, p = R.decode(R.activations(d[f"ref{i}"]), d[f"f0_{i}"], cfg["onset_threshold"], cfg["offset_threshold"], mode)
        assert iv.tolist() == d[f"intervals{i}_{mode}"].tolist()
        err = float(np.abs(p - d[f"pitches{i}_{mode}"]).max())
        print(f"item {i} {mode}: {err:.2e}")
        assert err <= (MEDIAN_BOUND if mode == "median" else WEIGHTED_BOUND)


@pytest.mark.parametrize("case", ["decoded", "halves"])
def test_note_frames_against_the_reference_results(golden, case):
    d = golden("transcriber_small")
    cfg = json.loads(str(d["config"]))
    midi, lf0 = R.note_frames(d[f"score_{case}_pitches"], d[f"score_{case}_intervals"], int(d[f"score_{case}_n24"]),
                              cfg["hop_length"] / cfg["sample_rate"], 10 / 1000.0, 24000)
    assert midi.dtype == np.int32 and np.array_equal(midi, d[f"score_{case}_midi"])
    assert lf0.dtype == np.int32 and np.array_equal(lf0[:, None], d[f"score_{case}_lf0"])


def test_note_frames_equals_estimate_score_where_the_quotient_is_inexact():
    cfg = dict(CFG, sample_rate=16000, hop_length=320)  # scale 0.02 against shift 0.01
    scale, shift = 320 / 16000, 10 / 1000.0
    off_floor = [k for k in range(200) if np.floor((k * scale) / shift) != 2 * k]
    off_ceil = [k for k in range(200) if np.ceil((k * scale) / shift) != 2 * k]
    assert off_floor[0] == 29 and off_ceil[0] == 7
    for a, b in ((7, 29), (29, 30), (1, 7), (3, 64)):
        midi, est = estimate_score([60.5], [[a, b]], 24000, cfg, sampling_rate=24000, shiftms=10)
        m, l = R.note_frames([60.5], [[a, b]], 24000, scale, shift, 24000)
        assert np.array_equal(m, midi) and np.array_equal(l[:, None], est)
    assert np.array_equal(R.log_hz_table()[[0, 57, 69]], [0, 5, 6])  # 220 and 440 Hz exactly: log truncates


NOTES = [{"note": [60, 0, 64], "note_start": [0.0, 0.105, 0.2], "note_end": [0.105, 0.2, 0.299]},
         {"note": [67, 72], "note_start": [0.25, 0.38], "note_end": [0.33, 0.4]}]


def test_ground_truth_score_of_hand_built_notes():
    got = preprocess.ground_truth_score(NOTES, 0.01)
    assert got.shape == (40, 1) and got.dtype == np.float64
    midi = np.zeros(40)
    midi[0:10] = 60   # int(0.105 / 0.01) = 10: the end is truncated
    midi[20:29] = 64  # int(0.299 / 0.01) = 29
    midi[25:33] = 67  # overlaps 64 and, later in the list, wins
    midi[38:40] = 72  # ends at the last frame
    want = np.where(midi > 0, np.log(440.0 * 2.0 ** ((midi - 69.0) / 12.0)), 0.0)
    assert np.array_equal(got[:, 0], want)
    assert not got[10:20].any()  # the rest: 0 stays 0
    assert np.array_equal(got, R.gt_score(NOTES, 0.01))
    assert got[0, 0] != np.floor(got[0, 0])  # nothing is truncated on float frames
