"""Float64 restatement of the note decoder and of the note-to-frame tracks, independent of serenade_amd/transcriber.py:
what serenade/modules/phoneme_midi/decoding.py:22-159 and serenade/bin/preprocess.py:206-259, 117-123, 510-528 compute,
written from their closed forms (runs, first maxima, "the last note covering a frame wins") instead of their loops.
The decisions (peaks, onsets, offsets) are taken on float32 activations exactly as the reference takes them; everything
from the f0 contour on is float64 (the reference follows float32 there), which is what srn_note_decode computes.

    activations(logits)                                        float32 sigmoid, torch's on the CPU
    peaks(v, threshold)                                        peak frames of one curve
    decode(act, f0, on_thr, off_thr, mode)                     (intervals (K, 2) int64, pitches (K,) float64)
    note_frames(pitches, intervals, n_samples, scale, shift, sampling_rate)   (midi (n,) int32, lf0 (n,) int32)
    log_hz_table()                                             the int32 log-Hz value of the MIDI numbers 0..127
    gt_score(note_seq, frame_shift)                            the ground-truth log-f0 track (n, 1) float64
"""
import numpy as np
import torch


def activations(logits):
    return torch.sigmoid(torch.as_tensor(np.asarray(logits, dtype=np.float32))).numpy()


def peaks(v, threshold):
    """a run is a maximal stretch v > threshold; a run closed before the last frame gives the first frame attaining the
    maximum over its frames with v > v[0]"""
    v = np.asarray(v, dtype=np.float32)
    n = len(v)
    above = np.concatenate([[0], (v > np.float32(threshold)).astype(np.int8), [0]])
    edge = np.diff(above)
    out = []
    for s, e in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):  # the run is [s, e)
        run = v[s:e]
        ok = run > v[0]
        if e < n and ok.any():
            out.append(s + int(np.flatnonzero(ok & (run == run[ok].max()))[0]))
    return np.asarray(out, dtype=np.int64)


def hann(L):
    """torch.hann_window(L) (periodic) in float64"""
    return np.ones(L) if L == 1 else 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / L)


def pitch(seg, mode):
    seg = np.asarray(seg, dtype=np.float64)
    ok = ~np.isnan(seg)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "median":
            vals = np.sort(seg[ok])
            p = vals[(len(vals) - 1) // 2] if len(vals) else np.nan
        elif mode == "weighted_mean":
            w = hann(len(seg))
            p = (w[ok] * seg[ok]).sum() / w[ok].sum() if len(seg) else np.nan
        else:
            w = np.where(ok, hann(len(seg)), 0.0)
            w = w / w.sum()
            order = np.argsort(seg, kind="stable")  # NaN last
            d, wt = seg[order], w[order]
            cum = np.cumsum(wt)
            p = np.interp(0.5, (cum - 0.5 * wt) / cum[-1], d) if ok.any() and not np.isnan(cum[-1]) else np.nan
    return 0.0 if p != p else float(p)


def midi_pitch(f0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return 12 * (np.log2(np.asarray(f0).astype(np.float32).astype(np.float64)) - np.log2(440.0)) + 69


def offsets(act, on_thr, off_thr):
    """[(onset, offset)] of every onset, emitted or not"""
    act = np.asarray(act, dtype=np.float32)
    n = len(act)
    on, offp, fr = peaks(act[:, 0], on_thr), peaks(act[:, 1], off_thr), act[:, 2]
    out = []
    for k, onset in enumerate(on):
        nxt = int(on[k + 1]) if k + 1 < len(on) else n - 1
        found = []
        cand = offp[(offp >= onset + 2) & (offp < nxt)]
        if len(cand):
            found.append(int(cand[np.argmax(act[cand, 1])]))  # argmax: the first maximum
        i = np.arange(onset + 2, nxt)
        falls = i[(fr[i] >= 0.5) & (fr[i + 1] < 0.5)] if len(i) else i
        conf = []
        for f in falls:
            tail = fr[f + 1:nxt]
            up = np.flatnonzero(tail >= 0.5)
            dip = tail[:up[0]] if len(up) else tail
            conf.append((np.float32(1) - dip).max() if len(dip) else np.float32(0))
        if len(conf) and max(conf) > 0:
            found.append(int(falls[int(np.argmax(conf))]))
        out.append((int(onset), max(found) if found else nxt - 1))
    return out


def decode(act, f0, on_thr, off_thr, mode):
    midi = midi_pitch(f0)
    iv, p = [], []
    for onset, offset in offsets(act, on_thr, off_thr):
        if offset > onset:
            iv.append([onset, offset + 1])
            p.append(pitch(midi[onset:offset + 1], mode))
    return np.asarray(iv, dtype=np.int64).reshape(-1, 2), np.asarray(p, dtype=np.float64)


def log_hz_table():
    m = np.arange(128)
    hz = np.trunc(440.0 * 2.0 ** ((m - 69.0) / 12.0))  # the first truncation: Hz stored into an int32 array
    with np.errstate(divide="ignore"):
        return np.where(m > 0, np.trunc(np.log(np.maximum(hz, 1))), 0).astype(np.int32)  # and the second


def note_frames(pitches, intervals, n_samples, scale, shift, sampling_rate):
    n = int(np.ceil((n_samples / sampling_rate) / shift))
    iv = np.asarray(intervals, dtype=np.float64).reshape(-1, 2)
    midi = np.zeros(n, dtype=np.int32)
    if len(iv):
        start = np.floor((iv[:, 0] * scale) / shift).astype(np.int64)
        end = np.minimum(np.ceil((iv[:, 1] * scale) / shift).astype(np.int64), n)
        value = np.rint(np.asarray(pitches, dtype=np.float64)).astype(np.int32)  # half to even
        f = np.arange(n)
        cover = (start[:, None] <= f) & (f < end[:, None])
        last = len(iv) - 1 - np.argmax(cover[::-1], axis=0)
        midi = np.where(cover.any(axis=0), value[last], 0).astype(np.int32)
    return midi, log_hz_table()[midi]


def gt_score(note_seq, frame_shift):
    """read_midi_json + _midi_to_hz(log_f0=True) on its float64 frames: int() truncation of both ends, later notes
    over earlier ones, no truncation of the values"""
    n = int(np.ceil(max(d["note_end"][-1] for d in note_seq) / frame_shift))
    notes = [(v, int(s / frame_shift), int(e / frame_shift)) for d in note_seq
             for v, s, e in zip(d["note"], d["note_start"], d["note_end"])]
    f = np.arange(n)
    midi = np.zeros(n)
    for v, s, e in notes:  # in order: the later note wins
        midi = np.where((s <= f) & (f < e), float(v), midi)
    with np.errstate(divide="ignore"):
        lf0 = np.where(midi > 0, np.log(440.0 * 2.0 ** ((midi - 69.0) / 12.0)), 0.0)
    return lf0[:, None]
