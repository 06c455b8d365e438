"""From raw waveforms to the tracks of a preprocessing dump in one call: the loop body of
serenade/bin/preprocess.py:399-611 without ground-truth MIDI (`--skip_gtmidi`), on the GPU.

    extract_features(audio, fs, config, contentvec, transcriber, midi_config, f0_range=(70, 1100), lengths=None,
                     ragged=False)
        -> one dict per utterance {"wave", "hubert", "logmel", "loud", "gt_lf0_score", "est_lf0_score", "f0", "vuv",
           "midi"} of numpy float32 arrays, or None where the reference skips the utterance

Nothing is computed here: audio.prepare, features.logmelfilterbank / loudness_extract, world.extract_f0 (Harvest),
ContentVec, the transcriber with reference_f0 (pYIN), FramewiseDecoder and estimate_score are composed as the
reference composes them.  The ragged front-ends take the whole batch; logmelfilterbank and loudness_extract run once
per group of utterances of equal length by default, and once for the whole batch (`lengths=`) with ragged=True.  The
csv / json / yaml handling of the reference's main() and the hdf5 writing stay with the caller (utils.io.write_hdf5
takes every track as it is returned)."""
import numpy as np
import torch

from . import audio as A
from . import world
from .contentvec import _nearest_index
from .features import logmelfilterbank, loudness_extract
from .transcriber import FramewiseDecoder, estimate_score, reference_f0

__all__ = ["extract_features", "TRACKS"]

TRACKS = ("wave", "hubert", "logmel", "loud", "gt_lf0_score", "est_lf0_score", "f0", "vuv", "midi")


def _f32(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32)


@torch.no_grad()
def extract_features(audio, fs, config, contentvec, transcriber, midi_config, f0_range=(70, 1100), lengths=None,
                     ragged=False):
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
    score is of no use to training, so no note is that skip here)."""
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
    contours = reference_f0(x16f, lens16, midi_config)
    decoder = FramewiseDecoder(midi_config)
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
            "loud": _f32(loud[b][:T]), "gt_lf0_score": _f32(np.expand_dims(est, axis=-1)[:T]),
            "est_lf0_score": _f32(est[:T]), "f0": _f32(f0[:T]), "vuv": _f32(vuv[:T]),
            "midi": _f32(np.expand_dims(midi, axis=-1)[:T])})
    return out
