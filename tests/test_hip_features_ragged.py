"""The ragged log-mel / loudness front-end on the MI355X: features.logmelfilterbank / loudness_extract with `lengths=`
(srn_pad_ragged / srn_pad_ragged_zero -> the STFT -> srn_logmel_ragged / srn_loudness_ragged) and
extract_features(ragged=True), at the recipe's geometry (24 kHz, hop 240, mel fft 512 / win 480 / 80 mels / 63-12000 Hz,
loudness n_fft 2048).  The cases, the reference (oracle/features_oracle.py on the unpadded item) and the bound (2e-4)
are tests/_features_ragged_cases.py's, which the CPU suite runs through the C-ABI emulator at the same shapes."""
import ctypes
import json

import numpy as np
import pytest
import torch

from serenade_amd import _lib, features, preprocess
from serenade_amd.contentvec import ContentVec
from serenade_amd.transcriber import TranscriptionModel
from tests import _features_ragged_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def edge_1e4():
    features._PLANS.clear()
    return C.run_edge(DEV, 1e4)


def test_edge_lengths_meet_the_oracle_per_item(edge_1e4):
    C.check_against_oracle(edge_1e4)


def test_nothing_past_an_item_is_read(edge_1e4):
    C.check_fill_independent(edge_1e4, C.run_edge(DEV, float("nan")))


def test_items_do_not_see_each_other():
    C.check_items_do_not_see_each_other(DEV)


def test_all_lengths_full_is_the_dense_call():
    C.check_anchored_to_dense(DEV)


# ------------------------------------------------------------------------------------------------ extract_features
CONFIG = dict(sampling_rate=24000, trim_silence=True, trim_threshold_in_db=60, trim_frame_size=2048,
              trim_hop_size=512, fft_size=2048, hop_size=240, win_length=1200, window="hann", num_mels=80, fmin=80,
              fmax=7600, shiftms=10)  # tests/test_hip_audio.py's


def _state(d):
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}


def _songs():
    t = np.arange(14400) / 24000  # 0.6 s
    tone = sum(np.sin(2 * np.pi * 220 * k * t) / k for k in (1, 2, 3)) * 0.3
    t = np.arange(9600) / 24000  # 0.4 s
    gap = 0.5 * np.sin(2 * np.pi * 262 * t) * ((t < 0.15) | (t > 0.25))
    return [tone, gap]


def test_extract_features_ragged_against_the_grouped_path(golden):
    dc, dt = golden("contentvec_small"), golden("transcriber_small")
    cv = ContentVec(device=DEV, **json.loads(str(dc["config"]))).load_state_dict(_state(dc))
    midi_config = json.loads(str(dt["config"]))
    tm = TranscriptionModel(midi_config, device=DEV).load_state_dict(_state(dt))
    songs = _songs()
    _, _, x16, lens16 = preprocess.A.prepare(songs, 24000, CONFIG)
    logits, frames = tm(x16.float(), lengths=lens16)
    inside = float(torch.sigmoid(logits[0, :frames[0], 0]).cpu().median())  # a threshold under which notes exist
    some = False
    for threshold in (midi_config["onset_threshold"], inside):
        mc = dict(midi_config, onset_threshold=threshold)
        want = preprocess.extract_features(songs, 24000, CONFIG, cv, tm, mc)
        got = preprocess.extract_features(songs, 24000, CONFIG, cv, tm, mc, ragged=True)
        assert len(got) == len(want) == 2
        assert [g is None for g in got] == [w is None for w in want]
        for g, w in zip(got, want):
            if w is None:
                continue
            some = True
            assert tuple(g) == preprocess.TRACKS
            for k in preprocess.TRACKS:
                assert g[k].dtype == np.float32 and g[k].shape == w[k].shape, k
                if k in ("logmel", "loud"):
                    err = float(np.abs(g[k].astype(np.float64) - w[k]).max())
                    print(f"extract_features ragged vs grouped, {k}: max abs diff {err:.3e}")
                    assert err < C.TOL, (k, err)
                else:
                    assert np.array_equal(g[k], w[k], equal_nan=True), k
    assert some


# ------------------------------------------------------------------------------------------------ C ABI
def test_bad_arguments_are_refused_before_any_launch():
    h = _lib.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    zeros = torch.zeros(64, device=DEV)
    ones = torch.ones(2, device=DEV, dtype=torch.int32)
    f, i = ptr(zeros), ptr(ones)
    out = torch.full((64,), 7.0, device=DEV)
    o = ptr(out)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb, ld = 3, 8
    cases = {
        "srn_pad_ragged_zero": [
            (None, 8, i, o, 2, 8, 2, 16, st),           # null x
            (f, 8, None, o, 2, 8, 2, 16, st),           # null lens
            (f, 8, i, o, 2, 8, 2, 11, st),              # ld < n + 2 pad
            (f, 8, i, o, 0, 8, 2, 16, st)],             # B <= 0
        "srn_logmel_ragged": [
            (None, f, i, o, 2, 2, nb, ld, 4, 1e-10, 10, st),   # null spec
            (f, f, None, o, 2, 2, nb, ld, 4, 1e-10, 10, st),   # null frames
            (f, f, i, o, 2, 0, nb, ld, 4, 1e-10, 10, st),      # T <= 0
            (f, f, i, o, 2, 2, nb, 5, 4, 1e-10, 10, st),       # ld < 2 n_bins
            (f, f, i, o, 2, 2, nb, ld, 4, 1e-10, 3, st)],      # log base 3
        "srn_loudness_ragged": [
            (None, f, i, i, o, 2, 2, nb, ld, 1e-10, 80.0, 1e-5, st),   # null spec
            (f, f, i, None, o, 2, 2, nb, ld, 1e-10, 80.0, 1e-5, st),   # null workspace
            (f, f, i, i, o, 2, -1, nb, ld, 1e-10, 80.0, 1e-5, st),     # T <= 0
            (f, f, i, i, o, 2, 2, nb, 5, 1e-10, 80.0, 1e-5, st)],      # ld < 2 n_bins
    }
    for name, calls in cases.items():
        for args in calls:
            assert getattr(h, name)(*args) != 0, (name, args)
            assert name[4:].encode() in h.srn_last_error(), (name, h.srn_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched: the output is untouched
