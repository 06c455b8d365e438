"""Writes tests/golden/transcriber_small.npz: seeded weights of a reduced TranscriptionModel (the reference's own
model.py / phonerec_model.py / subnetworks.py, eval mode, non-trivial BatchNorm running statistics), two 16 kHz inputs
(one over 512 frames, so BiLSTM.forward's chunk carry runs; one 40 dB quieter and shorter), and the reference's output
of each on its own (B = 1, float64): the logits and the phoneme model's logits.  Then decoding.py's FramewiseDecoder on
those logits (float32, as on the device) with a seeded f0 contour holding NaN runs, in all three pitch_sum modes, and
preprocess.py's midi_to_frames / _midi_to_hz on the decoded notes and on pitches at exact .5.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_transcriber.py

Absent packages are stubbed: nnAudio's MelSpectrogram and torchaudio's AmplitudeToDB by float64 restatements (reflect
pad, periodic Hann, |rfft|^2, a Slaney mel matrix kept as the float32 `mel_basis` buffer nnAudio registers; 10 log10
with amin 1e-10 and torchaudio's top_db clamp), librosa.hz_to_midi / midi_to_hz and wquantiles.median by restatements,
everything else preprocess.py imports by empty modules (nothing they would compute is captured)."""
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_harness  # noqa: E402

_ref_harness.install()

FRONT = dict(sample_rate=16000, win_length=256, hop_length=64, n_mels=32, fmin=30, fmax=8000)
CONFIG = dict(FRONT, model_complexity=4, onset_threshold=0.5, offset_threshold=0.5, pitch_sum="median",
              lang_model_config=dict(FRONT, model_complexity=4, num_lbl=40))
LENGTHS = (33400, 12000)  # 522 and 188 frames
MODES = ("median", "weighted_mean", "weighted_median")
THRESHOLD_MARGIN = 1e-3


def slaney_mel64(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(norm='slaney', htk=False) in float64"""
    f_sp, brk = 200.0 / 3, 1000.0
    brk_mel, logstep = brk / f_sp, math.log(6.4) / 27.0

    def hz2mel(f):
        return brk_mel + math.log(f / brk) / logstep if f >= brk else f / f_sp

    mels = np.linspace(hz2mel(fmin), hz2mel(fmax), n_mels + 2)
    hz = np.where(mels >= brk_mel, brk * np.exp(logstep * (mels - brk_mel)), f_sp * mels)
    bins = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    w = np.zeros((n_mels, len(bins)))
    for i in range(n_mels):
        lo = (bins - hz[i]) / (hz[i + 1] - hz[i])
        hi = (hz[i + 2] - bins) / (hz[i + 2] - hz[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lo, hi)) * 2.0 / (hz[i + 2] - hz[i])
    return w


class MelSpectrogram(nn.Module):
    """nnAudio.features.MelSpectrogram(center=True, pad_mode='reflect', window='hann', power=2) restated"""

    def __init__(self, sr, n_fft, win_length, n_mels, hop_length, fmin, fmax, center=True, **kw):
        super().__init__()
        assert center and win_length == n_fft
        self.n_fft, self.hop = n_fft, hop_length
        self.mel64 = slaney_mel64(sr, n_fft, n_mels, fmin, fmax)
        self.register_buffer("mel_basis", torch.from_numpy(self.mel64.astype(np.float32)))

    def forward(self, x):
        x = x.reshape(x.shape[0], 1, -1)
        x = F.pad(x, (self.n_fft // 2, self.n_fft // 2), mode="reflect")[:, 0]
        fr = x.unfold(-1, self.n_fft, self.hop)  # (B, T, n_fft)
        n = torch.arange(self.n_fft, dtype=torch.float64)
        win = (0.5 - 0.5 * torch.cos(2 * math.pi * n / self.n_fft)).to(x.dtype)
        spec = torch.fft.rfft(fr * win, dim=-1)
        power = spec.real ** 2 + spec.imag ** 2  # (B, T, bins)
        return torch.matmul(self.mel_basis.to(x.dtype), power.transpose(1, 2))  # (B, n_mels, T)


class AmplitudeToDB(nn.Module):
    """torchaudio.transforms.AmplitudeToDB(stype='power', top_db) restated (ref 1, amin 1e-10; one maximum over the
    packed batch, as torchaudio takes it)"""

    def __init__(self, stype="power", top_db=None):
        super().__init__()
        assert stype == "power"
        self.top_db = top_db

    def forward(self, x):
        x_db = 10.0 * torch.log10(torch.clamp(x, min=1e-10))
        if self.top_db is not None:
            shape = x_db.shape
            packed = shape[-3] if x_db.dim() > 2 else 1
            x_db = x_db.reshape(-1, packed, shape[-2], shape[-1])
            x_db = torch.max(x_db, (x_db.amax(dim=(-3, -2, -1)) - self.top_db).view(-1, 1, 1, 1))
            x_db = x_db.reshape(shape)
        return x_db


def hz_to_midi(f):
    return 12 * (np.log2(np.asanyarray(f)) - np.log2(440.0)) + 69


def midi_to_hz(notes):
    return 440.0 * (2.0 ** ((np.asanyarray(notes) - 69.0) / 12.0))


def quantile_1d(data, weights, q):
    data, weights = np.asarray(data), np.asarray(weights)
    order = np.argsort(data)
    d, wt = data[order], weights[order]
    cum = np.cumsum(wt)
    return np.interp(q, (cum - 0.5 * wt) / cum[-1], d)


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _pyin(*a, **k):
    raise RuntimeError("pyin is not captured: the fixture passes f0")


def install_stubs():
    feats = _module("nnAudio.features", MelSpectrogram=MelSpectrogram)
    _module("nnAudio", features=feats)
    tr = _module("torchaudio.transforms", AmplitudeToDB=AmplitudeToDB)
    _module("torchaudio", transforms=tr)
    _module("librosa", hz_to_midi=hz_to_midi, midi_to_hz=midi_to_hz, pyin=_pyin)
    _module("wquantiles", median=lambda d, w: quantile_1d(d, w, 0.5))
    for n in ("mido", "pyworld", "kaldiio"):
        _module(n)
    _module("transformers", HubertModel=nn.Module)
    _module("serenade.datasets", AudioSCPDataset=None)


def seed_model(model, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("weight") and p.dim() == 4:
                p.copy_(r(*p.shape) * math.sqrt(2.0 / (p.shape[1] * 9)))
            elif "rnn." in name:
                p.copy_(r(*p.shape) / math.sqrt(p.shape[-1] if p.dim() == 2 else 32))
            elif name.endswith("weight") and p.dim() == 2:
                p.copy_(r(*p.shape) / math.sqrt(p.shape[1]))
            elif p.dim() == 1 and "cnn" in name and name.endswith("weight"):  # BN gamma
                p.copy_(1.0 + 0.2 * r(*p.shape))
            else:
                p.copy_(0.1 * r(*p.shape))
        for name, m in model.named_modules():
            if isinstance(m, nn.BatchNorm2d):
                first = name.endswith("cnn.1") and "lang_conv_stack" not in name  # layer 0 of a mel stack: dB inputs
                m.running_mean.copy_((20.0 if first else 0.2) * r(m.num_features))
                m.running_var.copy_((400.0 if first else 0.5) * (1.0 + torch.rand(m.num_features, generator=g,
                                                                                  dtype=torch.float64)))
    return model


def wave(i, n, rng):
    t = np.arange(n) / 16000.0
    f0 = 180.0 * (1 + 0.3 * i) * 2.0 ** (np.floor(t * 6) % 5 / 12.0)  # a note every 1/6 s
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    env = (np.sin(np.pi * (t * 6 % 1.0)) ** 2)
    x = sum(0.3 / k * np.sin(k * ph) for k in (1, 2, 3)) * env + 0.01 * rng.standard_normal(n)
    return (x * (0.01 if i == 1 else 1.0)).astype(np.float32)  # item 1: 40 dB quieter


def f0_contour(rng, T):
    f0 = 200.0 * 2.0 ** (np.cumsum(0.05 * rng.standard_normal(T)) / 12.0)
    for _ in range(max(2, T // 60)):
        a = int(rng.integers(0, T - 10))
        f0[a:a + int(rng.integers(1, 10))] = np.nan
    return f0


def main():
    install_stubs()
    from serenade.bin import preprocess as P
    from serenade.modules.phoneme_midi.decoding import FramewiseDecoder
    from serenade.modules.phoneme_midi.model import TranscriptionModel

    for seed in range(100, 200):
        torch.manual_seed(seed)
        model = seed_model(TranscriptionModel(CONFIG).eval(), seed)
        rng = np.random.default_rng(seed)
        waves = [wave(i, n, rng) for i, n in enumerate(LENGTHS)]
        # random weights leave the logits nearly constant: rescale combined_fc so that on item 0 every output has mean 0
        # and standard deviation 2 (onsets, offsets and note runs then occur)
        with torch.no_grad():
            o = model(torch.from_numpy(waves[0]).view(1, 1, -1))[0].double()
            fc = model.combined_fc
            a = 2.0 / o.std(0)
            fc.bias.copy_(-a * (o.mean(0) - fc.bias.double()))
            fc.weight.mul_(a.view(-1, 1).float())
        m64 = model.double()
        outs, phons = [], []
        torch.set_default_dtype(torch.float64)  # BiLSTM.forward makes its (h, c) with the default dtype
        with torch.no_grad():
            for w in waves:
                x = torch.from_numpy(w).double().view(1, 1, -1)
                outs.append(m64(x)[0].numpy())
                phons.append(m64.lang_model.run_on_batch({"audio": x})["frame"][0].numpy())
        torch.set_default_dtype(torch.float32)
        s = 1.0 / (1.0 + np.exp(-np.concatenate(outs)))
        if np.abs(s - 0.5).min() > THRESHOLD_MARGIN:
            break
    print("seed", seed, "min |sigmoid - 0.5|", np.abs(s - 0.5).min())
    model = model.float()
    out = {"config": np.array(json.dumps(CONFIG)), "seed": np.int64(seed)}
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy()
    out["mel64"] = model.pitch_feat_ext.feat.mel64
    rng = np.random.default_rng(7)
    for i, w in enumerate(waves):
        out[f"wave{i}"] = w
        out[f"ref{i}"] = outs[i]
        out[f"phon{i}"] = phons[i].astype(np.float32)
        T = outs[i].shape[0]
        f0 = f0_contour(rng, T)
        out[f"f0_{i}"] = f0
        pred = torch.from_numpy(outs[i].astype(np.float32)).view(1, T, 3)
        for mode in MODES:
            dec = FramewiseDecoder(dict(CONFIG, pitch_sum=mode))
            p, iv = dec.decode(pred, f0=torch.from_numpy(f0).float())
            assert len(p) >= 3, (i, mode, len(p))
            out[f"pitches{i}_{mode}"] = np.asarray(p, dtype=np.float64)
            out[f"intervals{i}_{mode}"] = np.asarray(iv, dtype=np.int64).reshape(-1, 2)
        print(f"item {i}: {T} frames, {len(p)} notes")
    # preprocess.py:510-528 on the decoded notes of item 0 and on notes whose pitches sit at exact .5
    half = [60.5, 61.5, 62.5, 0.5, 63.4999, 64.5001]
    cases = {"decoded": (list(out["pitches0_weighted_median"]), out["intervals0_weighted_median"].tolist(), 33400 * 1.5),
             "halves": (half, [[3, 40], [41, 90], [100, 101], [120, 150], [160, 200], [190, 260]], 16000 * 1.5)}
    for name, (p, iv, n24) in cases.items():
        time = (np.array(iv) * (CONFIG["hop_length"] / CONFIG["sample_rate"])).reshape(-1, 2)
        notes = np.array([round(v) for v in p])
        frames = P.midi_to_frames(notes, time, n24 / 24000, shift_ms=10)
        out[f"score_{name}_pitches"] = np.asarray(p, dtype=np.float64)
        out[f"score_{name}_intervals"] = np.asarray(iv, dtype=np.int64)
        out[f"score_{name}_n24"] = np.int64(n24)
        out[f"score_{name}_midi"] = frames
        out[f"score_{name}_lf0"] = np.expand_dims(P._midi_to_hz(frames, log_f0=True), axis=-1)
    path = os.path.join(HERE, "transcriber_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
