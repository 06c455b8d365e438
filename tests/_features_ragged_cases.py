"""TEST-ONLY: the cases of the ragged log-mel / loudness front-end (features.logmelfilterbank / loudness_extract with
`lengths=`), shared by the CPU run through the C-ABI emulator (tests/test_features_ragged_emulated.py) and the run on
the GPU (tests/test_hip_features_ragged.py): same shapes, same reference, same bound.

Reference: oracle/features_oracle.py (float64) on the unpadded item x[b, :n_b].  Bound: max abs error < 2e-4, the bound
tests/test_features.py holds both functions to.  Each reference is computed once per process and never written to.
"""
import functools

import numpy as np
import torch

from oracle import features_oracle as FO
from serenade_amd import features

SR, FFT, WIN, HOP, MELS, FMIN, FMAX = 24000, 512, 480, 240, 80, 63, 12000  # conf/serenade.yaml:4-21
MEL_KW = dict(fft_size=FFT, hop_size=HOP, win_length=WIN, window="hann", num_mels=MELS, fmin=FMIN, fmax=FMAX)
TOL = 2e-4
LOUD_FFT = 2048

# Lengths that straddle a frame boundary (k hop - 1, k hop, k hop + 1: the frame count steps between the first two) and
# the pad reach, the longest item off the hop grid, and the shortest legal item: 257 for log-mel (reflect pad 256), 2
# for loudness with zero padding, 1025 for loudness with reflect padding (pad 1024).  Reflect padding of 1024 refuses
# the 4 hop +- 1 items themselves (961 <= 1024), so that batch straddles the next boundary up, 5 hop, under a longer
# n_max.
EDGE = {"mel": (5 * HOP + 17, 4 * HOP - 1, 4 * HOP, 4 * HOP + 1, 257),
        "constant": (5 * HOP + 17, 4 * HOP - 1, 4 * HOP, 4 * HOP + 1, 2),
        "reflect": (6 * HOP + 17, 5 * HOP - 1, 5 * HOP, 5 * HOP + 1, 1025)}
LOG_BASES = (10.0, 2.0, None)
PAD_MODES = ("constant", "reflect")


@functools.lru_cache(maxsize=None)
def wave(n, seed, gain=1.0):
    """two tones + noise with a near-silent start (eps / amin / the top_db floor), float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 3300.0 * t + 1.0) + 0.02 * rng.standard_normal(n)
    x[: n // 7] *= 1e-3
    x = (gain * x).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def quiet_wave(n, seed):
    """at least 80 dB below full scale: noise of sigma 3e-5 (bin powers about 7e-7, above amin = 1e-10) plus tones
    scaled by 0.5e-4"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.5e-4 * (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 3300.0 * t + 1.0))
    x = (x + 3e-5 * rng.standard_normal(n)).astype(np.float32)
    x.setflags(write=False)
    return x


def _frozen(a):
    a.setflags(write=False)
    return a


def ref_mel(x, log_base):
    return _ref_mel(x.tobytes(), log_base)


def ref_loud(x, pad_mode):
    return _ref_loud(x.tobytes(), pad_mode)


@functools.lru_cache(maxsize=None)
def _ref_mel(raw, log_base):
    return _frozen(FO.logmelfilterbank(np.frombuffer(raw, dtype=np.float32), SR, log_base=log_base, **MEL_KW))


@functools.lru_cache(maxsize=None)
def _ref_loud(raw, pad_mode):
    return _frozen(FO.loudness_extract(np.frombuffer(raw, dtype=np.float32), SR, HOP, pad_mode=pad_mode))


def batch(waves, fill, dev):
    """padded (B, n_max) float32 batch whose tail holds `fill`, which nothing may read"""
    lens = [len(w) for w in waves]
    x = torch.full((len(waves), max(lens)), fill, dtype=torch.float32)
    for b, w in enumerate(waves):
        x[b, :len(w)] = torch.from_numpy(np.array(w))
    return x.to(dev), lens


def edge_waves(kind):
    return [wave(n, seed) for seed, n in enumerate(EDGE[kind])]


def run_edge(dev, fill):
    """every variant on its edge batch -> {name: (result on the host, frames, waves)}"""
    out = {}
    waves = edge_waves("mel")
    x, lens = batch(waves, fill, dev)
    for base in LOG_BASES:
        mel, frames = features.logmelfilterbank(x, SR, log_base=base, lengths=lens, **MEL_KW)
        out["mel", base] = (mel.cpu(), frames, waves)
    for mode in PAD_MODES:
        waves = edge_waves(mode)
        x, lens = batch(waves, fill, dev)
        loud, frames = features.loudness_extract(x, SR, HOP, pad_mode=mode, lengths=torch.tensor(lens))  # a tensor too
        out["loud", mode] = (loud.cpu(), frames, waves)
    return out


def check_against_oracle(res, verbose=True):
    """frames == [1 + n_b // hop], live frames within TOL of the oracle on the unpadded item, the rest exactly 0"""
    for (what, opt), (got, frames, waves) in res.items():
        lens = [len(w) for w in waves]
        assert frames == [1 + n // HOP for n in lens], (what, opt)
        assert got.shape[:2] == (len(waves), 1 + max(lens) // HOP) and got.dtype == torch.float32
        assert got.shape[2:] == ((MELS,) if what == "mel" else ())
        for b, w in enumerate(waves):
            ref = ref_mel(w, opt) if what == "mel" else ref_loud(w, opt)
            assert len(ref) == frames[b]
            err = float(np.abs(got[b, :frames[b]].numpy().astype(np.float64) - ref).max())
            if verbose:
                print(f"ragged {what} {opt} item {b} (n = {lens[b]}): max abs err {err:.3e}")
            assert err < TOL, (what, opt, b, err)
            assert not got[b, frames[b]:].any(), (what, opt, b)  # exact zeros (NaN would count as nonzero)


def check_fill_independent(res_a, res_b):
    """the live frames of two runs whose padding differs are the same bits, and finite"""
    assert res_a.keys() == res_b.keys()
    for k, (a, frames, _) in res_a.items():
        b = res_b[k][0]
        for i, T in enumerate(frames):
            assert torch.isfinite(a[i, :T]).all() and torch.equal(a[i, :T], b[i, :T]), (k, i)
        assert torch.equal(a, b), k  # and the zero rows with them


def check_items_do_not_see_each_other(dev):
    """a full-scale item beside one 80 dB and more below it: the quiet item keeps its own top_db floor"""
    n_loud, n_quiet = 10 * HOP + 17, 8 * HOP + 5
    quiet = quiet_wave(n_quiet, 7)
    rms = lambda v: float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))
    for mode in PAD_MODES:
        ref = ref_loud(quiet, mode)
        rows = []
        for seed, gain in ((3, 2.0), (4, 2.2)):  # two loud neighbours of the same length
            loud = wave(n_loud, seed, gain)
            assert np.abs(loud).max() > 0.8 and 20 * np.log10(rms(loud) / rms(quiet)) >= 80.0  # full scale is 1
            for order in ((loud, quiet), (quiet, loud)):
                x, lens = batch(list(order), 1e4, dev)
                got, frames = features.loudness_extract(x, SR, HOP, pad_mode=mode, lengths=lens)
                q = 0 if order[0] is quiet else 1
                row = got[q, :frames[q]].cpu()
                err = float(np.abs(row.numpy().astype(np.float64) - ref).max())
                print(f"quiet item beside a loud one, {mode}, position {q}: max abs err {err:.3e}")
                assert err < TOL, (mode, err)
                # a batch-wide maximum would lift the quiet item's floor above all of its bins
                batch_floor = 10 * np.log10(np.abs(FO.stft(loud, LOUD_FFT, HOP, pad_mode=mode)).max() ** 2) - 80.0
                own_top = 10 * np.log10(np.abs(FO.stft(quiet, LOUD_FFT, HOP, pad_mode=mode)).max() ** 2)
                assert own_top < batch_floor
                rows.append((q, row))
        for q in (0, 1):
            same = [r for p, r in rows if p == q]
            assert len(same) == 2 and torch.equal(same[0], same[1]), (mode, q)  # the neighbour's content changed


def check_anchored_to_dense(dev):
    """every length = n: the ragged call is the dense call, bit for bit"""
    n = 10 * HOP + 17
    for B in (1, 3):
        x, lens = batch([wave(n, 20 + b) for b in range(B)], 0.0, dev)
        assert lens == [n] * B
        for base in LOG_BASES:
            dense = features.logmelfilterbank(x, SR, log_base=base, **MEL_KW)
            assert isinstance(dense, torch.Tensor)
            got, frames = features.logmelfilterbank(x, SR, log_base=base, lengths=lens, **MEL_KW)
            assert frames == [1 + n // HOP] * B and torch.equal(got, dense), ("mel", B, base)
        for mode in PAD_MODES:
            dense = features.loudness_extract(x, SR, HOP, pad_mode=mode)
            assert isinstance(dense, torch.Tensor)
            got, frames = features.loudness_extract(x, SR, HOP, pad_mode=mode, lengths=lens)
            assert frames == [1 + n // HOP] * B and torch.equal(got, dense), ("loud", B, mode)
