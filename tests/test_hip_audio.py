"""Waveform preparation on the MI355X (serenade_amd/audio.py + audio.hip, serenade_amd/preprocess.py) against the
float64 restatement tests/_audio_ref.py: the resampler at the lengths where it can go wrong and against the analytic
truth, exact ragged batching of all three kernels, trim and the window on known signals, prepare against the chain of
its own steps, extract_features against the public calls it composes, and stage 9's load_wave.  Every padded batch is
filled with 1e4 (or NaN) past the items: nothing may read it."""
import json

import numpy as np
import pytest
import torch

from serenade_amd import audio as A
from serenade_amd import preprocess, world
from serenade_amd.contentvec import ContentVec, _nearest_index
from serenade_amd.features import logmelfilterbank, loudness_extract
from serenade_amd.transcriber import FramewiseDecoder, TranscriptionModel, estimate_score, reference_f0

from . import _audio_ref as R
from .test_audio_host import STOPBAND, TRUTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATES = [(24000, 16000), (16000, 24000), (48000, 24000), (12000, 24000), (44100, 24000)]
RAGGED = (4801, 1, 257, 3000)
CONFIG = dict(sampling_rate=24000, trim_silence=True, trim_threshold_in_db=60, trim_frame_size=2048,
              trim_hop_size=512, fft_size=2048, hop_size=240, win_length=1200, window="hann", num_mels=80, fmin=80,
              fmax=7600, shiftms=10)


def _batch(waves, fill=1e4, dtype=torch.float64):
    """padded batch; the tail holds large values that nothing may read"""
    lens = [len(w) for w in waves]
    x = torch.full((len(waves), max(lens)), fill, dtype=dtype)
    for i, w in enumerate(waves):
        x[i, :len(w)] = torch.from_numpy(np.array(w)).to(dtype)
    return x.to(DEV), lens


def _noise(n, seed=0):
    return 0.5 * np.random.default_rng(seed).standard_normal(n)


def _edge_lengths(orig, target):
    """1, 2, shorter than the filter's span, the shortest inputs that give at least 255 / 256 / 257 outputs (the tile
    is 256; not every count is reachable at every ratio), 4801"""
    around = [next(n for n in range(1, 4000) if R.out_length(n, orig, target) >= m)
              for m in (A.TILE - 1, A.TILE, A.TILE + 1)]
    return [1, 2, 100] + sorted(set(around)) + [4801]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_resample_against_the_restatement(rates, dtype):
    lens = _edge_lengths(*rates)
    outs = [R.out_length(n, *rates) for n in lens[3:-1]]
    assert A.TILE - 1 <= min(outs) <= A.TILE < max(outs) <= A.TILE + 2  # both sides of the tile edge
    waves = [_noise(n, seed=i) for i, n in enumerate(lens)]
    x, _ = _batch(waves, dtype=dtype)
    y, out_lens = A.resample(x, *rates, lengths=lens)
    assert y.dtype == dtype and out_lens == [R.out_length(n, *rates) for n in lens] and y.shape == (len(lens), max(out_lens))
    y, xh = y.cpu().numpy(), x.cpu().numpy()
    bound = 1e-12 if dtype == torch.float64 else 1.2e-7
    for b, n in enumerate(lens):
        ref = R.resample(xh[b, :n], *rates)  # the values the kernel saw, in float64
        err = np.abs(y[b, :out_lens[b]] - ref).max() / np.abs(ref).max()
        print(f"{rates} n={n}: {err:.2e} of the peak")
        assert err <= bound, (rates, n)
        assert not y[b, out_lens[b]:].any()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_equal_rates_are_a_copy(dtype):
    x, lens = _batch([_noise(n, seed=n) for n in RAGGED], dtype=dtype)
    y, out_lens = A.resample(x, 24000, 24000, lengths=lens)
    assert out_lens == lens and y.dtype == dtype
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :n], x[b, :n]) and not y[b, n:].any()
    assert torch.equal(A.resample(x[0], 16000, 16000.0), x[0])


@pytest.mark.parametrize("rates", [(24000, 16000), (44100, 24000)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_resample_against_the_truth(rates):
    y = A.resample(torch.from_numpy(R.sines(rates[0], *rates)).to(DEV), *rates).cpu().numpy()
    err = R.truth_error(y, *rates)
    tone = A.resample(R.stopband_tone(*rates), *rates).cpu().numpy()  # numpy input: uploaded
    level = R.stopband_level(tone, *rates)
    print(f"{rates}: truth {err:.2e}, stop band {level:.2e}")
    assert err <= 2 * TRUTH[rates] and level <= 2 * STOPBAND[rates]


# ------------------------------------------------------------------------------------------- exact ragged batching
def _same(a, b):
    return a.shape == b.shape and bool((a.view(torch.int64 if a.dtype == torch.float64 else torch.int32)
                                        == b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)).all())


@pytest.mark.parametrize("fill", [1e4, float("nan")])
@pytest.mark.parametrize("rates", [(24000, 16000), (44100, 24000)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_resample_batch_equals_single_calls(rates, fill):
    waves = [_noise(n, seed=n) for n in RAGGED]
    for dtype in (torch.float64, torch.float32):
        x, lens = _batch(waves, fill, dtype)
        y, out_lens = A.resample(x, *rates, lengths=lens)
        for b, n in enumerate(lens):
            assert _same(y[b, :out_lens[b]], A.resample(x[b, :n].clone(), *rates)), (dtype, b)
    x32, lens = _batch(waves, fill, torch.float32)
    y32, out_lens = A.resample(x32, *rates, lengths=lens)
    y64, _ = A.resample(x32.double(), *rates, lengths=lens)
    for b in range(len(lens)):
        assert _same(y32[b, :out_lens[b]], y64[b, :out_lens[b]].float()), b


@pytest.mark.parametrize("fill", [1e4, float("nan")])
def test_trim_and_window_batch_equal_single_calls(fill):
    rng = np.random.default_rng(2)
    waves = [_noise(n, seed=n) * np.where(np.arange(n) < n // 3, 1e-4, 1.0) * rng.uniform(0.2, 1.0) for n in RAGGED]
    for dtype in (torch.float64, torch.float32):
        x, lens = _batch(waves, fill, dtype)
        for fl, hop in ((2048, 512), (1000, 300)):
            y, n_out, index = A.trim(x, 30, fl, hop, lengths=lens)
            for b, n in enumerate(lens):
                one, idx = A.trim(x[b, :n].clone(), 30, fl, hop)
                assert np.array_equal(idx, index[b]) and _same(one, y[b, :n_out[b]]) and not y[b, n_out[b]:].any()
        starts = [7, 0, 100, 1234]
        counts = [n - s for n, s in zip(lens, starts)]
        y = A._window(x.device, starts, counts, 0).run(x)
        for b in range(len(lens)):
            one = A._window(x.device, starts[b:b + 1], counts[b:b + 1], 0).run(x[b:b + 1, :lens[b]].clone())
            assert _same(one[0], y[b, :counts[b]]) and _same(one[0], x[b, starts[b]:lens[b]])
            assert not y[b, counts[b]:].any()
    # the tail pad needs pad < n: the same batch without its one-sample item
    x, lens = _batch([waves[0], waves[2], waves[3]], fill, torch.float32)
    y, n_out = A.pad_tail(x, 256, lens)
    assert n_out == [n + 256 for n in lens]
    for b, n in enumerate(lens):
        assert _same(y[b, :n_out[b]], A.pad_tail(x[b, :n].clone(), 256)) and not y[b, n_out[b]:].any()
    # float32 decisions are the float64 decisions on the same values
    x32, lens = _batch(waves, fill, torch.float32)
    assert np.array_equal(A.trim_index(x32, 30, lengths=lens), A.trim_index(x32.double(), 30, lengths=lens))


# ---------------------------------------------------------------------------------------------------- trim, window
@pytest.mark.parametrize("fl,hop", [(2048, 512), (1000, 300)])
def test_trim_against_the_restatement(fl, hop):
    sig = R.trim_signals()
    want = {k: R.trim(v, 60, fl, hop) for k, v in sig.items()}
    assert all(len(near) == 0 for _, near in want.values())
    x, lens = _batch(list(sig.values()))
    y, n_out, index = A.trim(x, 60, fl, hop, lengths=lens)
    for b, (name, v) in enumerate(sig.items()):
        (s, e), _ = want[name]
        assert tuple(index[b]) == (s, e) and n_out[b] == e - s, name
        assert np.array_equal(y[b, :n_out[b]].cpu().numpy(), v[s:e]) and not y[b, n_out[b]:].any()
        one, idx = A.trim(torch.from_numpy(np.array(v)).to(DEV), 60, fl, hop)
        assert tuple(idx) == (s, e) and np.array_equal(one.cpu().numpy(), v[s:e]), name
        one, idx = A.trim(np.asarray(v, dtype=np.float32), 60, fl, hop)  # numpy float32: uploaded, float32 out
        assert tuple(idx) == R.trim(np.asarray(v, dtype=np.float32), 60, fl, hop)[0] and one.dtype == torch.float32
    # nothing passes a threshold of 0 dB below the loudest frame: (0, 0) and an empty item
    y, n_out, index = A.trim(x, 0, fl, hop, lengths=lens)
    assert not index.any() and n_out == [0] * len(lens) and not y.any()


def test_window_against_numpy_pad():
    v = _noise(3000, seed=9)
    for dtype in (np.float64, np.float32):
        x = torch.from_numpy(v.astype(dtype)).to(DEV)
        for pad in (512, 2999):
            assert np.array_equal(A.pad_tail(x, pad).cpu().numpy(), np.pad(v.astype(dtype), (0, pad), "reflect"))
        for start, n in ((37, 2000), (2990, 10), (1, 2)):
            for pad in (512, n - 1):
                if pad < n:
                    got = A._window(x.device, [start], [n], pad).run(x[None])[0].cpu().numpy()
                    assert np.array_equal(got, np.pad(v.astype(dtype)[start:start + n], (0, pad), "reflect"))
                    assert np.array_equal(got, R.window(v.astype(dtype), start, n, pad))


# ---------------------------------------------------------------------------------------------------- prepare
def _utterances():
    """a 44.1 kHz stereo item (silence - tone - silence) and a 24 kHz mono item, float64 as soundfile reads them"""
    t = np.arange(30000) / 44100
    left = 0.6 * np.sin(2 * np.pi * 220 * t) * ((t > 0.1) & (t < 0.55))
    right = 0.4 * np.sin(2 * np.pi * 330 * t + 0.5) * ((t > 0.15) & (t < 0.5))
    stereo = np.stack([left, right], axis=1)
    mono = 0.5 * np.sin(2 * np.pi * 196 * np.arange(11000) / 24000) * (np.arange(11000) > 3000)
    return stereo, mono


@pytest.mark.parametrize("trim_silence", [True, False])
def test_prepare_equals_the_chain_of_its_steps(trim_silence):
    stereo, mono = _utterances()
    cfg = dict(CONFIG, trim_silence=trim_silence)
    x, lens, x16, lens16 = A.prepare([stereo, mono], [44100, 24000], cfg)
    assert x.dtype == torch.float64 and x.shape == (2, max(lens)) and x16.shape == (2, max(lens16))
    for b, (item, fs) in enumerate(((torch.from_numpy(stereo).mean(dim=1), 44100), (torch.from_numpy(mono), 24000))):
        y = item.to(DEV)
        if fs != 24000:
            y = A.resample(y, fs, 24000)
            assert len(y) == A.resample_length(len(item), fs, 24000)
        if trim_silence:
            before = len(y)
            y, (s, e) = A.trim(y, 60, 2048, 512)
            assert 0 < s and len(y) == e - s < before  # the trim did something
        y = A.pad_tail(y, cfg["fft_size"])
        assert lens[b] == len(y) and _same(x[b, :lens[b]], y) and not x[b, lens[b]:].any()
        y16 = A.resample(y, 24000, 16000)
        assert lens16[b] == len(y16) == A.resample_length(lens[b], 24000, 16000)
        assert _same(x16[b, :lens16[b]], y16) and not x16[b, lens16[b]:].any()
    # the same utterances as a padded float32 batch at one rate
    xb, n = _batch([mono, mono[:9000]], dtype=torch.float32)
    x, lens, x16, lens16 = A.prepare(xb, 24000, cfg, lengths=n)
    one = A.prepare([mono[:9000].astype(np.float32)], 24000, cfg)
    assert x.dtype == torch.float32 and lens[1] == one[1][0] and _same(x[1, :lens[1]], one[0][0])
    assert _same(x16[1, :lens16[1]], one[2][0])


# ---------------------------------------------------------------------------------------------------- the dump
def _state(d):
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}


@pytest.fixture(scope="module")
def models(golden):
    dc, dt = golden("contentvec_small"), golden("transcriber_small")
    cv = ContentVec(device=DEV, **json.loads(str(dc["config"]))).load_state_dict(_state(dc))
    midi_config = json.loads(str(dt["config"]))
    return cv, TranscriptionModel(midi_config, device=DEV).load_state_dict(_state(dt)), midi_config


def _songs():
    t = np.arange(14400) / 24000  # 0.6 s
    tone = sum(np.sin(2 * np.pi * 220 * k * t) / k for k in (1, 2, 3)) * 0.3
    t = np.arange(9600) / 24000  # 0.4 s
    gap = 0.5 * np.sin(2 * np.pi * 262 * t) * ((t < 0.15) | (t > 0.25))
    return [tone, gap]


def test_extract_features_composes_the_public_calls(models):
    cv, tm, midi_config = models
    songs = _songs()
    x, lens, x16, lens16 = A.prepare(songs, 24000, CONFIG)
    x16f = x16.float()
    hid, hid_frames = cv(x16f, lengths=lens16)
    logits, frames = tm(x16f, lengths=lens16)
    contours = reference_f0(x16f, lens16, midi_config)
    f0s = world.extract_f0(x, 24000, 70, 1100, CONFIG["shiftms"], lengths=lens)
    # thresholds: the fixture's own, one inside item 0's onset curve (so that notes exist) and one nothing can reach
    onset0 = torch.sigmoid(logits[0, :frames[0], 0]).cpu()
    inside = float(onset0.median())
    some = False
    for threshold in (midi_config["onset_threshold"], inside, 1.5):
        mc = dict(midi_config, onset_threshold=threshold)
        got = preprocess.extract_features(songs, 24000, CONFIG, cv, tm, mc)
        assert len(got) == 2
        for b in range(2):
            p, i = FramewiseDecoder(mc).decode(logits[b, :frames[b]], f0=contours[b])
            if not p:
                assert got[b] is None
                continue
            some = True
            midi, est = estimate_score(p, i, lens[b], mc, sampling_rate=24000, shiftms=CONFIG["shiftms"])
            mel = logmelfilterbank(x[b:b + 1, :lens[b]], 24000, fft_size=2048, hop_size=240, win_length=1200,
                                   num_mels=80, fmin=80, fmax=7600)[0]
            loud = loudness_extract(x[b:b + 1, :lens[b]], 24000, 240)[0]
            scale = (24000 / 240) * (160 / 16000)
            hubert = hid[b, torch.from_numpy(_nearest_index(hid_frames[b], scale)).to(DEV)]
            T = min(len(loud), len(midi), len(hubert))
            want = {"wave": x[b, :lens[b]], "hubert": hubert[:T], "logmel": mel[:T], "loud": loud[:T, None],
                    "gt_lf0_score": est[:T, :, None], "est_lf0_score": est[:T], "f0": f0s[b][0][:T],
                    "vuv": f0s[b][1][:T], "midi": midi[:T, None]}
            assert tuple(got[b]) == preprocess.TRACKS
            for k, v in want.items():
                v = (v.cpu().numpy() if isinstance(v, torch.Tensor) else v).astype(np.float32)
                assert got[b][k].dtype == np.float32 and got[b][k].shape == v.shape, k
                assert np.array_equal(got[b][k], v, equal_nan=True), k
            D = got[b]["hubert"].shape[1]
            assert {k: v.shape for k, v in got[b].items()} == {
                "wave": (lens[b],), "hubert": (T, D), "logmel": (T, 80), "loud": (T, 1), "gt_lf0_score": (T, 1, 1),
                "est_lf0_score": (T, 1), "f0": (T, 1), "vuv": (T, 1), "midi": (T, 1)}
        if threshold == 1.5:
            assert got == [None, None]
    assert some


# ---------------------------------------------------------------------------------------------------- stage 9
def test_load_wave_resamples_other_rates(tmp_path):
    from serenade_amd.bin.ssc_postprocessing import load_wave
    from serenade_amd.utils.io import read_wav, write_wav_pcm16
    v = 0.5 * np.sin(2 * np.pi * 200 * np.arange(5000) / 16000)
    write_wav_pcm16(str(tmp_path / "a16.wav"), v, 16000)
    write_wav_pcm16(str(tmp_path / "a24.wav"), v, 24000)
    x, sr = read_wav(str(tmp_path / "a16.wav"))
    assert sr == 16000 and len(x) == 5000
    got = load_wave(str(tmp_path / "a16.wav"), 24000, torch.device(DEV))
    want = A.resample(torch.from_numpy(np.asarray(x, dtype=np.float64)).to(DEV), 16000, 24000)
    assert got.shape == (1, A.resample_length(5000, 16000, 24000)) and got.dtype == torch.float32
    assert _same(got[0], want.float())
    same = load_wave(str(tmp_path / "a24.wav"), 24000, torch.device(DEV))
    x24, _ = read_wav(str(tmp_path / "a24.wav"))
    assert _same(same[0], torch.from_numpy(np.asarray(x24, dtype=np.float32)).to(DEV))
