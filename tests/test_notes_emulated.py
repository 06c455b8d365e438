"""The host side of the GPU note decoding on the CPU: FramewiseDecoder.decode_batch, estimate_score_batch and
extract_features(device_decode=True) through CPU statements of the two entry points (srn_note_decode and
srn_note_frames, stated here with tests/_notes_ref.py; the other ops stay tests/_emulator.py's).  What is checked is
the plumbing -- padding, counts, limits, the crop and the single copy per track -- not the kernels
(tests/test_hip_notes.py)."""
import numpy as np
import pytest
import torch

from serenade_amd import preprocess, transcriber
from serenade_amd.transcriber import NOTE_MAX_FRAMES, FramewiseDecoder, estimate_score, estimate_score_batch
from tests import _emulator as E
from tests import _notes_cases as C
from tests import _notes_ref as R

from .test_notes_host import NOTES

CFG = dict(sample_rate=16000, win_length=256, hop_length=64, onset_threshold=C.THRESHOLDS[0],
           offset_threshold=C.THRESHOLDS[0], pitch_sum="weighted_median")


def emul_notes(name, a):
    if name == "srn_note_decode":
        logits, frames, f0, f0_frames, B, Tmax, Fmax, on, off, mode, _, _, _, _, counts, intervals, pitches = a
        intervals.zero_()
        pitches.zero_()
        for b in range(B):
            n, nf = min(int(frames[b]), Tmax), min(int(f0_frames[b]), Fmax)
            iv, p = R.decode(R.activations(logits[b, :n].numpy()), f0[b, :nf].numpy(), on, off, C.MODES[mode])
            counts[b] = len(iv)
            intervals[b, :len(iv)] = torch.from_numpy(iv).int()
            pitches[b, :len(iv)] = torch.from_numpy(p)
    elif name == "srn_note_frames":
        counts, intervals, pitches, B, cap, ns, scale, shift, sr, table, _, midi, lf0, Nmax, n_frames, bad = a
        assert np.array_equal(table.numpy(), R.log_hz_table())
        midi.zero_()
        lf0.zero_()
        bad.zero_()
        for b in range(B):
            k = int(counts[b])
            p = pitches[b, :k].numpy()
            if ((np.rint(p) < 0) | (np.rint(p) > 127)).any():
                bad[0] = 1
                continue
            m, l = R.note_frames(p, intervals[b, :k].numpy(), int(ns[b]), scale, shift, sr)
            n_frames[b] = len(m)
            midi[b, :len(m)] = torch.from_numpy(m)
            lf0[b, :len(m)] = torch.from_numpy(l)
    else:
        return E.emul_call(name, a)


@pytest.fixture
def emulated(monkeypatch):
    with E.installed():  # restores CallOp.__call__ on exit
        transcriber.ops.CallOp.__call__ = lambda self_, stream=None: emul_notes(self_.name, self_.targs)
        monkeypatch.setattr(transcriber, "_require_cuda", lambda *a: None)
        yield


def _batch(items):
    T, F = max(len(l) for l, _ in items), max(len(f) for _, f in items)
    logits, f0 = torch.full((len(items), T, 3), 8.0), torch.full((len(items), F), 1e4, dtype=torch.float64)
    for b, (l, f) in enumerate(items):
        logits[b, :len(l)], f0[b, :len(f)] = torch.from_numpy(l), torch.from_numpy(f)
    return logits, [len(l) for l, _ in items], f0, [len(f) for _, f in items]


def test_decode_batch_and_score_batch_plumbing(emulated):
    items = [(C.curves(n, n), C.contour(max(n - 3, 1), n + 1)) for n in (257, 3, 130)]
    dec = FramewiseDecoder(CFG)
    counts, iv, p = dec.decode_batch(*_batch(items))
    assert counts.dtype == torch.int32 and iv.shape == (3, 257, 2) and p.shape == (3, 257) and p.dtype == torch.float64
    assert int(counts.sum()) > 5
    n24 = [int(len(l) * 64 * 1.5) for l, _ in items]
    midi, lf0, frames = estimate_score_batch(counts, iv, p, n24, CFG, sampling_rate=24000, shiftms=10)
    for b, (l, f) in enumerate(items):
        hp, hiv = dec.decode(torch.from_numpy(l), f0=f)
        k = int(counts[b])
        assert iv[b, :k].tolist() == hiv and np.abs(p[b, :k].numpy() - np.array(hp)).max(initial=0) < 1e-3
        if k:
            m, e = estimate_score(p[b, :k].tolist(), hiv, n24[b], CFG, sampling_rate=24000, shiftms=10)
            assert frames[b] == len(m) and np.array_equal(midi[b, :frames[b]].numpy(), m)
            assert np.array_equal(lf0[b, :frames[b], None].numpy(), e)
    with pytest.raises(ValueError, match=str(NOTE_MAX_FRAMES)):
        dec.decode_batch(torch.zeros(1, NOTE_MAX_FRAMES + 1, 3), [5], torch.zeros(1, 4, dtype=torch.float64), [4])
    with pytest.raises(ValueError, match="frames"):
        dec.decode_batch(torch.zeros(1, 8, 3), [9], torch.zeros(1, 4, dtype=torch.float64), [4])
    p[0, 0] = 128.0
    with pytest.raises(ValueError, match="0..127"):
        estimate_score_batch(counts, iv, p, n24, CFG, sampling_rate=24000, shiftms=10)


def test_without_the_emulator_a_cpu_tensor_is_an_error():
    with pytest.raises(RuntimeError, match="no CPU path"):
        FramewiseDecoder(CFG).decode_batch(torch.zeros(1, 8, 3), [8], torch.zeros(1, 8, dtype=torch.float64), [8])
    with pytest.raises(RuntimeError, match="no CPU path"):
        estimate_score_batch(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 2, dtype=torch.int32),
                             torch.zeros(1, 1, dtype=torch.float64), [10])


def test_extract_features_device_path_composes_like_the_host_path(emulated, monkeypatch):
    """every front-end replaced by a recorded tensor: the two settings must assemble the same nine tracks"""
    rng = np.random.default_rng(3)
    sr, hop = 24000, 240
    lens = [24000, 12000, 18000]
    B = len(lens)
    lens16 = [n * 2 // 3 for n in lens]
    items = [(C.curves(n // 64 + 1, 11 + b), C.contour(n // 64 + 1, 21 + b)) for b, n in enumerate(lens16)]
    items[1] = (np.full_like(items[1][0], -4.0), items[1][1])  # no note: None
    logits, frames, f0, f0_frames = _batch(items)
    x = torch.from_numpy(rng.standard_normal((B, max(lens))))
    fr = [n // hop + 1 for n in lens]
    mel = [torch.from_numpy(rng.standard_normal((f, 5)).astype(np.float32)) for f in fr]
    loud = [torch.from_numpy(rng.standard_normal(f).astype(np.float32)) for f in fr]
    hid = torch.from_numpy(rng.standard_normal((B, max(fr) + 3, 4)).astype(np.float32))
    f0s = [(torch.from_numpy(rng.random((f + 1, 1))), torch.ones(f + 1, 1)) for f in fr]
    monkeypatch.setattr(preprocess.A, "prepare", lambda *a: (x, lens, torch.zeros(B, max(lens16), dtype=torch.float64),
                                                             lens16))
    monkeypatch.setattr(preprocess, "logmelfilterbank", lambda xs, **kw: torch.stack([mel[lens.index(xs.shape[1])]]))
    monkeypatch.setattr(preprocess, "loudness_extract", lambda xs, *a, **kw: torch.stack([loud[lens.index(xs.shape[1])]]))
    monkeypatch.setattr(preprocess.world, "extract_f0", lambda *a, **kw: f0s)
    monkeypatch.setattr(preprocess, "reference_f0", lambda *a: [f0[b, :f0_frames[b]].numpy() for b in range(B)])
    monkeypatch.setattr(preprocess, "reference_f0_device", lambda *a: (f0, f0_frames))
    cv = lambda w, lengths: (hid, [f + 2 for f in fr])
    tm = lambda w, lengths: (logits, frames)
    config = dict(sampling_rate=sr, hop_size=hop, fft_size=2048, win_length=1200, window="hann", num_mels=5, fmin=80,
                  fmax=7600, shiftms=10)
    seqs = [NOTES, None, None]
    host = preprocess.extract_features(None, sr, config, cv, tm, CFG, note_seqs=seqs)
    dev = preprocess.extract_features(None, sr, config, cv, tm, CFG, note_seqs=seqs, device_decode=True)
    assert [h is None for h in host] == [d is None for d in dev] == [False, True, False]
    for h, d in zip(host, dev):
        if h is None:
            continue
        assert tuple(d) == tuple(h) == preprocess.TRACKS
        for k in preprocess.TRACKS:
            assert d[k].dtype == np.float32 and d[k].shape == h[k].shape and np.array_equal(d[k], h[k]), k
    T = len(host[0]["midi"])
    assert host[0]["gt_lf0_score"].shape == (40, 1) and T > 40  # cropped with [:T] without entering the minimum
    assert np.array_equal(host[0]["gt_lf0_score"], R.gt_score(NOTES, 0.01).astype(np.float32))
    assert host[2]["gt_lf0_score"].shape == (len(host[2]["midi"]), 1, 1)
    with pytest.raises(ValueError, match="note lists"):
        preprocess.extract_features(None, sr, config, cv, tm, CFG, note_seqs=[None])
