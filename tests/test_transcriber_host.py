"""CPU checks of the MIDI note transcriber's host side (serenade_amd/transcriber.py): frame counts, the state-dict
mapping against the reference's key set, the BatchNorm fold, the mel matrix, and the host decoder + estimate_score
against the reference's own decoding.py / preprocess.py (tests/golden/transcriber_small.npz)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from serenade_amd import transcriber as tr
from serenade_amd.transcriber import FramewiseDecoder, TranscriptionModel, estimate_score

MODES = ("median", "weighted_mean", "weighted_median")


@pytest.fixture(scope="module")
def fx(golden):
    d = golden("transcriber_small")
    return d, json.loads(str(d["config"]))


def _sd(d):
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}


def test_frame_counts(fx):
    d, cfg = fx
    m = TranscriptionModel(cfg, device="cpu")
    for i in range(2):
        assert m.frames(len(d[f"wave{i}"])) == d[f"ref{i}"].shape[0] == d[f"phon{i}"].shape[0]
    assert TranscriptionModel(device="cpu").frames(160000) == 501


def test_state_dict_keys_match_the_reference(fx):
    d, cfg = fx
    m = TranscriptionModel(cfg, device="cpu")
    sd = _sd(d)
    network = {k for k in sd if "feat_ext." not in k and not k.endswith("num_batches_tracked")}
    assert network == set(m.state_shapes())
    for k, shp in m.state_shapes().items():
        assert tuple(sd[k].shape) == shp, k
    for k in ("pitch_feat_ext.feat.mel_basis", "lang_model.feat_ext.feat.mel_basis"):
        assert k in sd  # ignored as a network key, used as the mel matrix


@pytest.mark.parametrize("drop", ["combined_rnn.rnn.weight_hh_l0_reverse", "lang_conv_stack.cnn.9.running_var"])
def test_missing_key_raises(fx, drop):
    d, cfg = fx
    sd = _sd(d)
    del sd[drop]
    with pytest.raises(KeyError, match="missing"):
        TranscriptionModel(cfg, device="cpu").load_state_dict(sd)


def test_unexpected_key_raises(fx):
    d, cfg = fx
    sd = _sd(d)
    sd["combined_fc.extra"] = torch.zeros(3)
    with pytest.raises(KeyError, match="unexpected"):
        TranscriptionModel(cfg, device="cpu").load_state_dict(sd)


def test_bn_fold_equals_conv_then_batchnorm():
    g = torch.Generator().manual_seed(0)
    w, b = torch.randn(6, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
    gamma, beta = 1 + 0.2 * torch.randn(6, generator=g), 0.1 * torch.randn(6, generator=g)
    mean, var = torch.randn(6, generator=g), 0.5 + torch.rand(6, generator=g)
    x = torch.randn(2, 3, 9, 11, generator=g, dtype=torch.float64)
    ref = F.batch_norm(F.conv2d(x, w, b, padding=1), mean.double(), var.double(), gamma.double(), beta.double(),
                       False, 0.0, 1e-5)
    wf, bf = tr.fold_bn(w, b, gamma, beta, mean, var)
    assert torch.allclose(F.conv2d(x, wf, bf, padding=1), ref, rtol=0, atol=1e-12)


def test_w_hh_layout():
    H = 8
    w = torch.arange(2 * 4 * H * H, dtype=torch.float32).reshape(2, 4 * H, H)
    t = tr.lstm_w_hh_t(w[0], w[1])
    assert t.shape == (2, H, H, 4)
    for d_, k, j, q in ((0, 3, 5, 2), (1, 7, 0, 3), (1, 0, 7, 0)):
        assert t[d_, k, j, q] == w[d_, q * H + j, k]


def test_mel_matrix_against_the_fixture(fx):
    d, cfg = fx
    m = TranscriptionModel(cfg, device="cpu")
    built = m.mel_matrix("pitch")
    assert built.shape == d["mel64"].shape
    assert np.abs(built - d["mel64"]).max() <= 1e-12 * np.abs(d["mel64"]).max()
    sd = _sd(d)  # a checkpoint's mel_basis of the right shape is taken as it is
    assert np.array_equal(m.mel_matrix("lang", sd), sd["lang_model.feat_ext.feat.mel_basis"].double().numpy())


@pytest.mark.parametrize("mode", MODES)
def test_decoder_matches_the_reference(fx, mode):
    d, cfg = fx
    dec = FramewiseDecoder(dict(cfg, pitch_sum=mode))
    for i in range(2):
        p, iv = dec.decode(torch.from_numpy(d[f"ref{i}"].astype(np.float32)), f0=d[f"f0_{i}"])
        assert np.asarray(iv, dtype=np.int64).reshape(-1, 2).tolist() == d[f"intervals{i}_{mode}"].tolist(), (i, mode)
        assert np.array_equal(np.asarray(p, dtype=np.float64), d[f"pitches{i}_{mode}"]), (i, mode)


def test_decoder_needs_f0_or_librosa(fx):
    d, cfg = fx
    dec = FramewiseDecoder(cfg)
    try:
        import librosa  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="librosa"):
            dec.decode(torch.from_numpy(d["ref1"]), audio=d["wave1"])
    with pytest.raises(ValueError):
        dec.decode(torch.from_numpy(d["ref1"]))


@pytest.mark.parametrize("case", ["decoded", "halves"])
def test_estimate_score_matches_the_reference(fx, case):
    d, cfg = fx
    p = list(d[f"score_{case}_pitches"])
    iv = d[f"score_{case}_intervals"].tolist()
    midi, lf0 = estimate_score(p, iv, int(d[f"score_{case}_n24"]), cfg, sampling_rate=24000, shiftms=10)
    ref_midi, ref_lf0 = d[f"score_{case}_midi"], d[f"score_{case}_lf0"]
    assert midi.dtype == ref_midi.dtype == np.int32 and np.array_equal(midi, ref_midi)
    assert lf0.shape == ref_lf0.shape and lf0.dtype == ref_lf0.dtype and np.array_equal(lf0, ref_lf0)
    if case == "halves":
        assert set(midi.tolist()) == {0, 60, 62, 63, 65}  # half to even: 60.5 -> 60, 61.5 -> 62, 62.5 -> 62, 0.5 -> 0
