"""From raw waveforms to the tracks of a preprocessing dump in one call: the loop body of
serenade/bin/preprocess.py:399-611, with ground-truth MIDI (`note_seqs=`) or without (`--skip_gtmidi`), on the GPU.

    extract_features(audio, fs, config, contentvec, transcriber, midi_config, f0_range=(70, 1100), lengths=None,
                     ragged=False, device_decode=False, note_seqs=None)
        -> one dict per utterance {"wave", "hubert", "logmel", "loud", "gt_lf0_score", "est_lf0_score", "f0", "vuv",
           "midi"} of numpy float32 arrays, or None where the reference skips the utterance
    ground_truth_score(note_seq, frame_shift)
        -> the gt_lf0_score track of one GTSinger-style note list (preprocess.py:206-234, :465-468), on the host

Nothing is computed here: audio.prepare, features.logmelfilterbank / loudness_extract, world.extract_f0 (Harvest),
ContentVec, the transcriber with reference_f0 (pYIN), FramewiseDecoder and estimate_score are composed as the
reference composes them.  The ragged front-ends take the whole batch; logmelfilterbank and loudness_extract run once
per group of utterances of equal length by default, and once for the whole batch (`lengths=`) with ragged=True.  The
note decoding and the score tracks run per utterance on the host by default, and in two launches for the whole batch
with device_decode=True (FramewiseDecoder.decode_batch, estimate_score_batch).  The csv / json / yaml handling of the
reference's main() and the writing of the dump are serenade_amd/bin/preprocess.py."""
import numpy as np
import torch

from . import audio as A
from . import world
from .contentvec import _nearest_index
from .features import logmelfilterbank, loudness_extract
from .transcriber import (FramewiseDecoder, _midi_to_hz_librosa, estimate_score, estimate_score_batch, reference_f0,
                          reference_f0_device)

__all__ = ["extract_features", "ground_truth_score", "TRACKS"]

TRACKS = ("wave", "hubert", "logmel", "loud", "gt_lf0_score", "est_lf0_score", "f0", "vuv", "midi")


def _f32(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32)


def ground_truth_score(note_seq, frame_shift):
    """read_midi_json(note_seq, frame_shift) (preprocess.py:206-234) then _midi_to_hz(log_f0=True) on its float64
    frames (:468): note_seq is a list of {"note": [...], "note_start": [...], "note_end": [...]} (seconds); a note
    covers the frames int(start / frame_shift) .. int(end / frame_shift), later notes over earlier ones, a rest (0)
    stays 0.  (frames, 1) float64 -- on float frames nothing is truncated, unlike the estimated score."""
    max_time = max(note["note_end"][-1] for note in note_seq)
    midi = np.zeros(int(np.ceil(max_time / frame_shift)))
    for note in note_seq:
        for value, start, end in zip(note["note"], note["note_start"], note["note_end"]):
            midi[int(start / frame_shift):int(end / frame_shift)] = value
    lf0 = np.zeros_like(midi)
    keep = midi > 0
    lf0[keep] = np.log(_midi_to_hz_librosa(midi[keep]))
    return np.expand_dims(lf0, axis=-1)


@torch.no_grad()
def extract_features(audio, fs, config, contentvec, transcriber, midi_config, f0_range=(70, 1100), lengths=None,
                     ragged=False, device_decode=False, note_seqs=None):
    """audio, fs, lengths: as audio.prepare takes them (a list of utterances or a padded batch; one rate or one per
    item).  config: the recipe's preprocessing config (sampling_rate, trim_*, fft_size, hop_size, win_length, window,
    num_mels, fmin, fmax, shiftms, optional log_base).  contentvec: a loaded ContentVec; transcriber: a loaded
    TranscriptionModel and midi_config its checkpoint's config.  f0_range: (minf0, maxf0) of Harvest, scalars or one
    value per item (preprocess.py:474-483 reads them from a per-speaker file; 70 / 1100 is its fallback).
    ragged: False runs log-mel and loudness once per group of utterances of equal sample count -- after the silence
    trim that is one B = 1 call, with a plan of its own, per utterance; True runs each once for the whole batch with
    per-item lengths.  Every item is still padded, analysed and floored on its own, but srn_conv_gemm decides split-K
    per launch shape, so the STFT of an item inside a batch is not promised to round like its B = 1 call of another
    shape: `logmel` and `loud` agree between the two settings to the fp32 rounding of the STFT (tested to 2e-4, the
    bound of both functions against their float64 restatement), not bit for bit.  The other tracks are the same bits.

    Per item, the tracks preprocess.py:567-611 writes, every one float32 and cropped to
    min(len(loud), len(midi), len(hubert)) frames T except the wave: wave (n,), hubert (T, hidden), logmel
    (T, num_mels), loud / est_lf0_score / f0 / vuv / midi (T, 1), and gt_lf0_score (T, 1, 1) -- without ground-truth
    MIDI the reference expands the estimated score a second time (:532).  None for an utterance in which the decoder
    finds no note: the skip of :512-524 (the reference tests `p is None`, its decoder returns empty lists; an all-zero
    score is of no use to training, so no note is that skip here).

    device_decode: False decodes the notes and builds the score tracks per utterance on the host (one copy of the
    logits per item, FramewiseDecoder.decode, estimate_score).  True does both for the whole batch on the GPU
    (decode_batch, estimate_score_batch, the pYIN contour never leaves the device), crops every track on the device and
    copies each track to the host once per batch.  The GPU's sigmoid and float64 pitch are not promised to equal the
    host's float32 ones in the last bit, so a decision that hangs on the last bit of an activation, or a pitch within
    about 1e-4 of a half-integer, may fall the other way; everything else is the same bits.
    note_seqs: None, or per item None or a GTSinger-style note list (ground_truth_score).  With one, gt_lf0_score is
    the ground-truth track (min(T, its frames), 1): cropped with [:T] without entering the minimum, as
    preprocess.py:545-548 does."""
    sr = config["sampling_rate"]
    x, lens, x16, lens16 = A.prepare(audio, fs, config, lengths)
    B = len(lens)
    # log-mel and loudness (preprocess.py:435-447, :471-472): one call per group of equal length, or one ragged call
    kw = dict(sampling_rate=sr, hop_size=config["hop_size"], fft_size=config["fft_size"],
              win_length=config["win_length"], window=config["window"], num_mels=config["num_mels"],
              fmin=config["fmin"], fmax=config["fmax"], log_base=config.get("log_base", 10.0))
    logmel, loud = [None] * B, [None] * B
    if ragged:
        mel, fr = logmelfilterbank(x, lengths=lens, **kw)
        ld, _ = loudness_extract(x, sr, config["hop_size"], lengths=lens)
        for b in range(B):
            logmel[b], loud[b] = mel[b, :fr[b]], ld[b, :fr[b], None]
    else:
        for n in sorted(set(lens)):
            idx = [b for b in range(B) if lens[b] == n]
            xs = x[idx, :n]
            mel = logmelfilterbank(xs, **kw)
            ld = loudness_extract(xs, sr, config["hop_size"])
            for i, b in enumerate(idx):
                logmel[b], loud[b] = mel[i], ld[i][:, None]
    # Harvest (:485-493)
    f0s = world.extract_f0(x, sr, f0_range[0], f0_range[1], config["shiftms"], lengths=lens)
    # ContentVec at the acoustic frame shift (:495-503) and the transcriber's logits and pYIN contours (:505-507)
    x16f = x16.to(torch.float32)
    shiftms = config["hop_size"] * 1000 / sr
    hid, hid_frames = contentvec(x16f, lengths=lens16)
    scale = (sr / int(sr * shiftms / 1000)) * (160 / 16000)
    logits, frames = transcriber(x16f, lengths=lens16)
    decoder = FramewiseDecoder(midi_config)
    if note_seqs is None:
        note_seqs = [None] * B
    if len(note_seqs) != B:
        raise ValueError(f"extract_features: {len(note_seqs)} note lists for {B} utterances")
    gts = [None if seq is None else ground_truth_score(seq, shiftms / 1000) for seq in note_seqs]
    if device_decode:
        return _finish_on_device(x, lens, logmel, loud, f0s, hid, hid_frames, scale, gts, decoder.decode_batch(
            logits, frames, *reference_f0_device(x16f, lens16, midi_config)), midi_config, sr, config["shiftms"])
    contours = reference_f0(x16f, lens16, midi_config)
    out = []
    for b in range(B):
        pitches, intervals = decoder.decode(logits[b, :frames[b]], f0=contours[b])
        if not pitches:
            out.append(None)
            continue
        midi, est = estimate_score(pitches, intervals, lens[b], midi_config, sampling_rate=sr,
                                   shiftms=config["shiftms"])
        index = torch.from_numpy(_nearest_index(hid_frames[b], scale)).to(hid.device)
        hubert = hid[b].index_select(0, index)
        f0, vuv = f0s[b]
        T = min(len(loud[b]), len(midi), len(hubert))
        out.append({
            "wave": _f32(x[b, :lens[b]]), "hubert": _f32(hubert[:T]), "logmel": _f32(logmel[b][:T]),
            "loud": _f32(loud[b][:T]),
            "gt_lf0_score": _f32((np.expand_dims(est, axis=-1) if gts[b] is None else gts[b])[:T]),
            "est_lf0_score": _f32(est[:T]), "f0": _f32(f0[:T]), "vuv": _f32(vuv[:T]),
            "midi": _f32(np.expand_dims(midi, axis=-1)[:T])})
    return out


def _finish_on_device(x, lens, logmel, loud, f0s, hid, hid_frames, scale, gts, notes, midi_config, sr, shiftms):
    """the tail of extract_features with device_decode=True: score tracks, the crop to T and one host copy per track"""
    B, dev = len(lens), x.device
    counts, intervals, pitches = notes
    midi, est, n_midi = estimate_score_batch(counts, intervals, pitches, lens, midi_config, sampling_rate=sr,
                                             shiftms=shiftms)
    index = [torch.from_numpy(_nearest_index(hid_frames[b], scale)).to(dev) for b in range(B)]
    T = [min(len(loud[b]), n_midi[b], len(index[b])) for b in range(B)]
    per_item = {"wave": [x[b, :lens[b]] for b in range(B)],
                "hubert": [hid[b].index_select(0, index[b][:T[b]]) for b in range(B)],
                "logmel": [logmel[b][:T[b]] for b in range(B)], "loud": [loud[b][:T[b]] for b in range(B)],
                "est_lf0_score": [est[b, :T[b], None] for b in range(B)], "f0": [f0s[b][0][:T[b]] for b in range(B)],
                "vuv": [f0s[b][1][:T[b]] for b in range(B)], "midi": [midi[b, :T[b], None] for b in range(B)]}
    # one copy per track: the items' rows one after another, split again on the host
    host = {k: np.split(_f32(torch.cat([t.reshape(t.shape[0], -1) for t in v])), np.cumsum([len(t) for t in v])[:-1])
            for k, v in per_item.items()}
    found = counts.cpu().tolist()
    out = []
    for b in range(B):
        if not found[b]:
            out.append(None)
            continue
        item = {k: host[k][b].reshape(per_item[k][b].shape) for k in per_item}
        item["gt_lf0_score"] = _f32((item["est_lf0_score"][..., None] if gts[b] is None else gts[b])[:T[b]])
        out.append({k: item[k] for k in TRACKS})
    return out
