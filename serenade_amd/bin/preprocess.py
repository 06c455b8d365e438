#!/usr/bin/env python3
"""`serenade-preprocess` for MI355X: stages 1 and 6 of the recipe, from a `wav.scp` to one feature file per utterance.

Mirror of the reference's preprocessing entry point (serenade/bin/preprocess.py:262-611: its flags, the files it
reads, the per-utterance rules and the nine datasets it writes); the arithmetic is serenade_amd.preprocess
.extract_features, N utterances per call:

    python -m serenade_amd.bin.preprocess --wav-scp data/train/wav.scp --dumpdir dump/train/raw \\
        --midi-path data/train/midi.scp --f0-path conf/f0.yaml --config conf/serenade.yaml \\
        --contentvec contentvec.pt [--skip-gtmidi 1] [--batch-utterances 8] [--ragged] [--device-decode]

Files read: `--wav-scp` lists `UTT path.wav` (a path ending in `|` is a command and is rejected; so is `--segments`);
`--midi-path` lists `UTT /path.wav`, the note JSON of UTT being that path with `.wav` -> `.json`; `--f0-path` is a yaml
map speaker -> {minf0, maxf0}; `--config` is the recipe's preprocessing yaml, whose `midi_model_file` names the
transcriber checkpoint ({"config", "model_state_dict"}).  `--contentvec` names a saved HubertModel state dict (the
reference downloads one), bare or as {"config": settings, "state_dict": weights} for another geometry.

Per utterance, as the reference: channels are averaged; samples beyond [-1, 1] are an error; without `--skip-gtmidi` an
utterance whose note JSON is missing is skipped and the others get the ground-truth score of theirs; the Harvest range
comes from the f0 file by the speaker field of the name (`utt_id.split("_")[3].split("-")[1]`), 70 / 1100 otherwise --
a name without that field takes the fallback too, where the reference raises IndexError; an utterance in which the
transcriber finds no note is skipped.  `--skip-gtmidi` keeps the reference's `type=bool`: any non-empty value, "False"
included, turns it on.

Written: `UTT.h5` in `--dumpdir` with the datasets wave, hubert, logmel, loud, gt_lf0_score, est_lf0_score, f0, vuv,
midi (float32), or `UTT.npz` with the same keys where h5py is not installed -- both forms are what compute_statistics
and ssc_decode read.  The exit status is 1 when no utterance was written.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch
import yaml

from serenade_amd import preprocess
from serenade_amd.contentvec import ContentVec
from serenade_amd.transcriber import TranscriptionModel
from serenade_amd.utils.io import read_wav, write_feats

F0_FALLBACK = (70, 1100)  # preprocess.py:482-483


def build_parser():
    p = argparse.ArgumentParser(description="Preprocess audio and extract the features of a dump (MI355X build).")
    p.add_argument("--wav-scp", "--scp", required=True, type=str, help="kaldi-style wav.scp file")
    p.add_argument("--segments", default=None, type=str, help="not supported: kaldi-style segments file")
    p.add_argument("--dumpdir", type=str, required=True, help="directory to dump feature files")
    p.add_argument("--midi-path", type=str, required=True, help="list `UTT /path.wav`; the note JSON lies beside the wav")
    p.add_argument("--f0-path", type=str, required=True, help="yaml file: speaker -> {minf0, maxf0}")
    p.add_argument("--skip-gtmidi", type=bool, default=False,
                   help="skip ground truth MIDI extraction (any non-empty value turns it on, as in the reference)")
    p.add_argument("--config", type=str, required=True, help="yaml format configuration file")
    p.add_argument("--verbose", type=int, default=1, help="0: warnings only, 1: info, 2+: debug (default 1)")
    p.add_argument("--contentvec", type=str, required=True,
                   help="(MI355X build only) saved HubertModel state dict of ContentVec")
    p.add_argument("--batch-utterances", type=int, default=8,
                   help="(MI355X build only) utterances per extract_features call (default 8)")
    p.add_argument("--ragged", action="store_true",
                   help="(MI355X build only) log-mel and loudness once per batch instead of once per length")
    p.add_argument("--device-decode", action="store_true",
                   help="(MI355X build only) decode the notes and build the score tracks of a batch on the GPU")
    return p


def _setup_logging(verbose):
    level = logging.WARN if verbose <= 0 else logging.INFO if verbose == 1 else logging.DEBUG
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    if verbose <= 0:
        logging.warning("Skip DEBUG/INFO messages")


def read_scp(path):
    """[(utt_id, wav path)] of a kaldi-style wav.scp, in file order"""
    out = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            utt_id, _, wav = line.strip().partition(" ")
            wav = wav.strip()
            if not wav or wav.endswith("|"):
                raise SystemExit(f"{path}: `{line.strip()}` is no `UTT path.wav` line (piped commands are not supported)")
            out.append((utt_id, wav))
    return out


def read_midi_list(path):
    """{utt_id: note JSON path} of the reference's `UTT /path.wav` list (pd.read_csv(delimiter=" /") and the "/" it
    puts back, preprocess.py:371, :452-455)"""
    out = {}
    with open(path) as f:
        for line in f:
            if line.strip():
                utt_id, sep, wav = line.rstrip("\n").partition(" /")
                if not sep:
                    raise SystemExit(f"{path}: `{line.strip()}` is no `UTT /path.wav` line")
                out.setdefault(utt_id, "/" + wav.strip().replace(".wav", ".json"))
    return out


def f0_range(utt_id, f0_file):
    """(minf0, maxf0) of Harvest for an utterance (preprocess.py:474-483)"""
    try:
        spk_id = utt_id.split("_")[3].split("-")[1]
    except IndexError:
        logging.info(f"cant find f0 extraction: {utt_id} names no speaker")
        return F0_FALLBACK
    try:
        return float(f0_file[spk_id]["minf0"]), float(f0_file[spk_id]["maxf0"])
    except (KeyError, TypeError, ValueError):
        logging.info(f"cant find f0 extraction: {spk_id}")
        return F0_FALLBACK


def load_contentvec(path, device):
    ckpt = torch.load(path, map_location="cpu")
    if isinstance(ckpt, dict) and "state_dict" in ckpt and "config" in ckpt:
        return ContentVec(device=device, **ckpt["config"]).load_state_dict(ckpt["state_dict"])
    return ContentVec(device=device).load_state_dict(ckpt)


def load_transcriber(path, device):
    """(model, its config) of the checkpoint `midi_model_file` names (preprocess.py:374-383)"""
    ckpt = torch.load(path, map_location="cpu")
    midi_config = ckpt["config"]
    return TranscriptionModel(midi_config, device=device).load_state_dict(ckpt["model_state_dict"]), midi_config


def load_utterance(utt_id, path):
    """(mono float64 samples, rate) of one wav (preprocess.py:399-403)"""
    audio, fs = read_wav(path)
    audio = np.asarray(audio, dtype=np.float64)
    if audio.ndim > 1 and audio.shape[1] > 1:
        audio = np.mean(audio, axis=1)
    audio = audio.reshape(-1)
    if not np.abs(audio).max() <= 1.0:
        raise AssertionError(f"{utt_id} seems to be different from 16 bit PCM.")
    return audio, fs


def _write(dumpdir, utt_id, tracks):
    try:
        import h5py  # noqa: F401
        ext = "h5"
    except ImportError:
        ext = "npz"
    path = os.path.join(dumpdir, f"{utt_id}.{ext}")
    if os.path.exists(path):
        os.remove(path)  # datasets of an earlier run are not merged into this one
    for key in preprocess.TRACKS:
        write_feats(path, key, tracks[key])
    return path


def main(argv=None):
    args = build_parser().parse_args(argv)
    _setup_logging(args.verbose)
    if args.segments is not None:
        raise SystemExit("--segments is not supported: cut the utterances beforehand and list the pieces in --wav-scp")
    if args.batch_utterances < 1:
        raise SystemExit("--batch-utterances must be at least 1")
    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    config.update(vars(args))
    utterances = read_scp(args.wav_scp)
    note_paths = read_midi_list(args.midi_path)
    with open(args.f0_path) as f:
        f0_file = yaml.load(f, Loader=yaml.BaseLoader) or {}
    os.makedirs(args.dumpdir, exist_ok=True)
    device = "cuda" if torch.cuda.is_available() else "cpu"
    contentvec = load_contentvec(args.contentvec, device)
    transcriber, midi_config = load_transcriber(config["midi_model_file"], device)

    todo, skipped = [], 0
    for utt_id, wav in utterances:
        notes = None
        if not args.skip_gtmidi:
            path = note_paths.get(utt_id)
            if path is None or not os.path.exists(path):
                logging.info(f"WARNING: {utt_id} has missing midi information")
                skipped += 1
                continue
            notes = path
        todo.append((utt_id, wav, notes))

    written = 0
    for i in range(0, len(todo), args.batch_utterances):
        group = todo[i:i + args.batch_utterances]
        audio, rates, seqs = [], [], []
        for utt_id, wav, notes in group:
            logging.info(f"processing {utt_id}")
            a, fs = load_utterance(utt_id, wav)
            audio.append(a)
            rates.append(fs)
            if notes is None:
                seqs.append(None)
            else:
                with open(notes) as f:
                    seqs.append(json.load(f))
        ranges = [f0_range(utt_id, f0_file) for utt_id, _, _ in group]
        feats = preprocess.extract_features(
            audio, rates, config, contentvec, transcriber, midi_config,
            f0_range=([r[0] for r in ranges], [r[1] for r in ranges]), ragged=args.ragged,
            device_decode=args.device_decode, note_seqs=None if args.skip_gtmidi else seqs)
        for (utt_id, _, _), tracks in zip(group, feats):
            if tracks is None:
                logging.info(f"skipping {utt_id} since it has no MIDI information")
                skipped += 1
                continue
            for key in preprocess.TRACKS:
                logging.info(f"{key}: {tracks[key].shape}")
            _write(args.dumpdir, utt_id, tracks)
            written += 1
    logging.info(f"wrote {written} utterances to {args.dumpdir}, skipped {skipped}")
    return 0 if written else 1


if __name__ == "__main__":
    sys.exit(main())
