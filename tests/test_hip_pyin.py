"""pYIN on the MI355X (serenade_amd/pitch.py + pyin.hip) against the float64 restatement tests/_pyin_ref.py: the
transcriber's settings and librosa's defaults on tones, glides, note sequences, octave leaps, noise, silence and short
items; the Viterbi alone; exact ragged batching; a 60 s item; and the transcriber's decoder fed by reference_f0.
Edge geometries, parameters off their defaults and the observation matrix itself: tests/test_zzzz_hip_pyin_sweep.py."""
import json

import numpy as np
import pytest
import torch

from serenade_amd import _lib, pitch
from serenade_amd.transcriber import FramewiseDecoder, TranscriptionModel, reference_f0

from . import _pyin_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRANS = dict(fmin=65, fmax=2093, sr=16000, frame_length=1024, hop_length=320)
DEFAULTS = dict(fmin=65, fmax=2093, sr=22050, frame_length=2048)


def _harm(f, sr, n, amp=0.3, n_harm=5):
    """harmonic signal of instantaneous frequency f (array of n, Hz)"""
    ph = 2 * np.pi * np.cumsum(f) / sr
    return sum(amp / k * np.sin(k * ph + 0.3 * k) for k in range(1, n_harm + 1) if k * f.max() < sr / 2)


def _signals(sr, sec=1.2, seed=0):
    rng = np.random.default_rng(seed)
    n = int(sec * sr)
    t = np.arange(n) / sr
    one = np.ones(n)
    notes = np.repeat([220.0, 0.0, 330.0, 261.6, 0.0, 392.0], -(-n // 6))[:n]
    seq = _harm(np.where(notes > 0, notes, 100.0), sr, n) * (notes > 0)
    leap = np.where(t < sec / 2, 150.0, 300.0)
    sig = {
        "near_fmin": _harm(68.0 * one, sr, n),
        "near_fmax": _harm(2000.0 * one, sr, n, n_harm=1),
        "mid": _harm(440.0 * one, sr, n),
        "vibrato_glide": _harm(200.0 * 2 ** (t / sec + 0.02 * np.sin(2 * np.pi * 5.5 * t)), sr, n),
        "notes_silences": seq,
        "octave_leap": _harm(leap, sr, n),
        "white_noise": 0.1 * rng.standard_normal(n),
        "silence": np.zeros(n),
        "short": _harm(180.0 * np.ones(700), sr, 700),
    }
    for k in ("mid", "vibrato_glide", "octave_leap"):
        sig[k] = sig[k] + 1e-3 * rng.standard_normal(n)
    return {k: v.astype(np.float32) for k, v in sig.items()}


def _batch(waves, fill=1e4):
    """padded batch; the tail holds large values that no valid frame may read"""
    lens = [len(w) for w in waves]
    x = torch.full((len(waves), max(lens)), fill, dtype=torch.float32)
    for i, w in enumerate(waves):
        x[i, :len(w)] = torch.from_numpy(w)
    return x.to(DEV), lens


def _compare(name, got, ref):
    f0, flag, vp = (np.asarray(v) for v in got)
    rf0, rflag, rvp, near = ref
    assert f0.shape == rf0.shape, name
    same = (flag == rflag) & ((f0 == rf0) | (np.isnan(f0) & np.isnan(rf0)))
    bad = ~same
    assert not (bad & ~near).any(), f"{name}: frames {np.nonzero(bad & ~near)[0][:10]} differ and are not near-ties"
    assert bad.mean() < 0.005, f"{name}: {bad.sum()} near-tie frames of {len(bad)}"
    assert np.abs(vp - rvp).max() <= 1e-12, f"{name}: voiced_prob {np.abs(vp - rvp).max():.2e}"


@pytest.mark.parametrize("kw", [TRANS, DEFAULTS], ids=["transcriber", "librosa_defaults"])
def test_signals_against_the_restatement(kw):
    sig = _signals(kw["sr"])
    names = list(sig)
    x, lens = _batch([sig[k] for k in names])
    f0, flag, vp, frames = pitch.pyin(x, lens, **kw)
    torch.cuda.synchronize()
    f0, flag, vp = f0.cpu().numpy(), flag.cpu().numpy(), vp.cpu().numpy()
    hop = kw.get("hop_length", kw["frame_length"] // 4)
    for i, k in enumerate(names):
        n = int(frames[i])
        assert n == 1 + lens[i] // hop
        ref = R.pyin(sig[k], **kw)
        _compare(k, (f0[i, :n], flag[i, :n], vp[i, :n]), ref)
        assert np.isnan(f0[i, n:]).all() and not flag[i, n:].any() and (vp[i, n:] == 0).all()
    v = flag[names.index("mid")]
    assert v[3:int(frames[names.index("mid")]) - 3].all()
    assert not flag[names.index("silence")].any()


def test_ragged_batch_equals_single_calls_and_ignores_padding():
    sig = _signals(16000, sec=0.9, seed=4)
    waves = [sig["vibrato_glide"], sig["short"], sig["notes_silences"][:9000], sig["white_noise"][:5000]]
    outs = []
    for fill in (1e4, -3.0):
        x, lens = _batch(waves, fill)
        outs.append([t.cpu() for t in pitch.pyin(x, lens, **TRANS)[:3]])
    for a, b in zip(*outs):
        assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    f0, flag, vp = outs[0]
    for i, w in enumerate(waves):
        f1, fl1, vp1, fr1 = pitch.pyin(torch.from_numpy(w).to(DEV), **TRANS)
        n = int(fr1[0])
        assert torch.equal(torch.nan_to_num(f0[i, :n], nan=-1.0), torch.nan_to_num(f1.cpu(), nan=-1.0)), i
        assert torch.equal(flag[i, :n], fl1.cpu()) and torch.equal(vp[i, :n], vp1.cpu()), i


def test_viterbi_alone_on_random_observations():
    rng = np.random.default_rng(11)
    n, w, s = 602, 91, 0.01
    B, T = 3, 40
    voiced = rng.random((B, T, n)) ** 8 * (rng.random((B, T, n)) < 0.02)
    vp = np.clip(voiced.sum(-1), 0, 1)
    vp[0, 5:25] = 1.0  # runs where every unvoiced state costs log(tiny)
    voiced[0, 5:15, :] = 0.0
    voiced[0, 5:15, 100] = 1.0
    voiced[0, 15:25, :] = 0.0
    voiced[0, 15:25, 340] = 1.0  # an out-of-band leap inside the run
    voiced[1, 10:20] = 0.0  # exact zeros: no observation at all
    vp[1, 10:20] = 0.0
    frames = [T, T - 7, 1]
    band = torch.from_numpy(pitch.log_band(n, w, s)).to(DEV)
    p_init = np.zeros(2 * n)
    p_init[n:] = 1 / n
    lpi = torch.from_numpy(np.log(p_init + R.TINY)).to(DEV)
    freqs = np.arange(2 * n, dtype=np.float64)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    obs, vpd, fr = d(voiced), d(vp), torch.tensor(frames, dtype=torch.int32, device=DEV)
    ptr = torch.empty(B, T, 2 * n, dtype=torch.int16, device=DEV)
    states = torch.empty(B, T, dtype=torch.int32, device=DEV)
    f0 = torch.empty(B, T, dtype=torch.float64, device=DEV)
    flag = torch.empty(B, T, dtype=torch.uint8, device=DEV)
    lib = _lib.lib()
    _lib.check(lib.srn_pyin_viterbi(obs.data_ptr(), vpd.data_ptr(), fr.data_ptr(), band.data_ptr(), lpi.data_ptr(),
                                    d(freqs).data_ptr(), float(np.log(R.TINY)), float("nan"), 1, ptr.data_ptr(),
                                    states.data_ptr(), f0.data_ptr(), flag.data_ptr(), B, T, n, w, None), "viterbi")
    torch.cuda.synchronize()
    trans = R.transition(n, w, s)
    st = states.cpu().numpy()
    for b in range(B):
        ref = R.viterbi(R.obs_matrix(voiced[b, :frames[b]], vp[b, :frames[b]]), trans, p_init)
        assert np.array_equal(st[b, :frames[b]], ref), b
        assert (st[b, frames[b]:] == -1).all()
    assert st[0, 14] == 100 and st[0, 15] == 340


def test_sixty_second_item():
    sr = 16000
    n = 60 * sr
    t = np.arange(n) / sr
    rng = np.random.default_rng(8)
    f = 180.0 * 2 ** (np.floor(t / 1.5) % 5 / 4)
    y = (_harm(f, sr, n) * (np.sin(2 * np.pi * t / 7) > -0.6) + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    f0, flag, vp, frames = pitch.pyin(torch.from_numpy(y).to(DEV), **TRANS)
    torch.cuda.synchronize()
    assert int(frames[0]) == 3001 and f0.shape == (3001,)
    _compare("60 s", (f0.cpu().numpy(), flag.cpu().numpy(), vp.cpu().numpy()), R.pyin(y, **TRANS))


def test_decoder_with_reference_f0_gives_the_restatement_notes(golden):
    d = golden("transcriber_small")
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    m = TranscriptionModel(cfg, device=DEV).load_state_dict(sd)
    n0, n1 = len(d["wave0"]), len(d["wave1"])
    x = torch.full((2, n0), 5.0)
    x[0] = torch.from_numpy(d["wave0"])
    x[1, :n1] = torch.from_numpy(d["wave1"])
    out, T = m(x.to(DEV), lengths=[n0, n1])
    f0s = reference_f0(x.to(DEV), [n0, n1], cfg)
    torch.cuda.synchronize()
    kw = dict(fmin=65, fmax=2093, sr=cfg["sample_rate"], frame_length=cfg["win_length"], hop_length=cfg["hop_length"])
    for i, w in enumerate((d["wave0"], d["wave1"])):
        ref = R.pyin(w, **kw)
        assert len(f0s[i]) == T[i]
        _compare(f"fixture item {i}", (f0s[i], ~np.isnan(f0s[i]), ref[2]), ref)
        for mode in ("median", "weighted_mean", "weighted_median"):
            dec = FramewiseDecoder(dict(cfg, pitch_sum=mode))
            got = dec.decode(out[i, :T[i]], f0=f0s[i])
            want = dec.decode(out[i, :T[i]], f0=ref[0])
            assert got[1] == want[1] and np.array_equal(np.asarray(got[0]), np.asarray(want[0])), (i, mode)
