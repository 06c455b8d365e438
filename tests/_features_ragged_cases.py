"""TEST-ONLY: the cases of the ragged log-mel / loudness front-end (features.logmelfilterbank / loudness_extract with
`lengths=`), shared by the CPU run through the C-ABI emulator (tests/test_features_ragged_emulated.py) and the run on
the GPU (tests/test_hip_features_ragged.py): same shapes, same reference, same bound.

Reference: oracle/features_oracle.py (float64) on the unpadded item x[b, :n_b].  Bound: max abs error < 2e-4, the bound
tests/test_features.py holds both functions to.  Each reference is computed once per process and never written to.

Below the recipe's cases: a list of other geometries (GEOMETRIES, LOUD_HOPS) that give the STFT plan its other shapes,
dense and ragged, to a bound derived from the fp32 CPU statement's own error (GEOM_TOL); on the GPU they run in
tests/test_zzz_hip_features_geometry.py.  One of them has an odd
n_fft - win_length (401 in 512): there the oracle and the product agree on centring the window with
lp = (n_fft - win_length) // 2 on the left; no librosa run backs that choice here, so this is agreement with the
oracle, not parity with librosa.
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


# ------------------------------------------------------------------------------------------------ other geometries
# The recipe's geometry above gives the STFT plan (features._Stft) one shape: signal rows every c = 16 samples, 32 wide,
# two tap groups.  These reach its other branches, dense and ragged, against the same oracle.
#   (fft, hop, win, mels): (row stride c = gcd(fft, hop, 16), tap width cw, tap groups of SRN_MAX_TAPS chained by RES_ADD)
GEOMETRIES = {
    (1024, 256, 1024, 80): (16, 32, 2),    # logmelfilterbank's own defaults
    (2048, 240, 1200, 80): (16, 32, 4),    # the preprocessing config's: 64 taps
    (512, 128, 400, 128): (16, 32, 1),     # exactly one group of 16 taps
    (512, 100, 401, 160): (4, 4, 8),       # the generic contraction kernel, 128 taps, odd fft - win, empty mel filters
    (256, 120, 200, 40): (8, 8, 2),
    (64, 16, 64, 130): (16, 32, 1),        # 2 taps; more mels than srn_logmel's workgroup and than bins
    (1024, 320, 1024, 229): (16, 32, 2),   # the transcriber's hop; the mel loop's second trip
}
LOUD_HOPS = {100: (4, 4, 32), 120: (8, 8, 16), 256: (16, 32, 4), 512: (16, 32, 4)}  # n_fft 2048
# The odd window difference (win 401 in fft 512) rests on the oracle and the product agreeing on the left padding of the
# window, lp = (n_fft - win) // 2; librosa is not installed, so no librosa run backs that choice here.
#
# Bound: 4 x the worst error of the fp32 CPU statement of the C ABI (the emulator) over the list, rounded up to two
# digits; `python -m tests._features_ragged_cases` prints the measured column again, tests/
# test_features_ragged_emulated.py holds the emulator to a quarter of the bound.  "mel" and "loud" are never looser than
# TOL above.  "mel-ill": the log-mel elements that mel_conditioning (below, from the oracle alone) puts above ILL_COND,
# held to 4 x what the emulator reaches on them.  There are two among the 33 000 of the list, both in the 911-sample
# item of (512, 100, 401, 160): mel 34 is bin 16 alone, which in frame 6 holds 6.8e-5 of the frame's largest bin in
# magnitude (-83 dB), so that half a float32 spacing of the largest bin is 1.7e-4 of it whatever the order of the sum.
#   what: (measured fp32 baseline, bound)
GEOM_TOL = {
    "mel": (9.764e-06, 4.0e-05),
    "mel-ill": (7.449e-05, 3.0e-04),
    "loud": (2.203e-07, 8.9e-07),
}
# A geometry with a bound of its own for the GPU run: (fp32 baseline that adds in the contraction's order, 4 x that).
# (1024, 320, 1024, 229) on the MI355X: 4.333e-05 in the 513-sample item, frame 0 (the near-silent start), mel 7, which
# is bin 5 alone at 1.0e-3 of the frame's largest bin in magnitude (-59.7 dB), while the kernels' own sweep
# (tests/test_zzz_hip_frontend_sweep.py) passes and every other geometry stays under 4.0e-05.  A plan bug or the order of an
# fp32 sum of 1024 terms?  logmel_in_kernel_order (below) restates the STFT as one fma chain per tap group, the order of
# the contraction kernel: it errs by 4.428e-05 in that same element, within 1e-6 of the GPU's result there (the
# emulator's blocked sums: 8.7e-06 over the geometry), and by 8.048e-05 at worst (mel 54: bin 35 alone at -75.4 dB).  So
# it is the order, and the geometry is held to 4 x what that restatement reaches, as the list is to 4 x the emulator;
# `python -m tests._features_ragged_cases` prints the figure again.  The emulator is held to the list's bound here too.
GEOM_OWN = {
    (1024, 320, 1024, 229): (8.048e-05, 3.3e-04),
}


def geometry_lengths(fft, hop):
    """the dense item, and the two a ragged batch adds: one hop and 18 samples shorter, and the shortest that reflect
    padding of fft / 2 takes"""
    return 5 * hop + 17 + fft, 4 * hop - 1 + fft, fft // 2 + 1


def plan_shape(st):
    """(c, cw, tap groups) of a features._Stft"""
    convs = [op for op in st.ops if isinstance(op, features.ops.ConvOp)]
    assert all(op.kw["ld_in0"] == convs[0].kw["ld_in0"] and op.kw["C_in"] == convs[0].kw["C_in"] for op in convs)
    assert all(("res_mode" in op.kw) == (k > 0) for k, op in enumerate(convs))  # every group after the first adds
    return convs[0].kw["ld_in0"], convs[0].kw["C_in"], len(convs)


@functools.lru_cache(maxsize=None)
def _ref_geom(raw, what, geom):
    x = np.frombuffer(raw, dtype=np.float32)
    if what == "mel":
        fft, hop, win, mels = geom
        return _frozen(FO.logmelfilterbank(x, SR, fft_size=fft, hop_size=hop, win_length=win, num_mels=mels))
    hop, mode = geom
    return _frozen(FO.loudness_extract(x, SR, hop, pad_mode=mode))


ILL_COND = 1e4


def mel_conditioning(w, geom):
    """(frames, mels), from the oracle alone: what filter m would pass if every bin under it were as large as frame
    t's largest, over what it does pass.  An fp32 DFT errs in every bin by a fraction of the spacing of the frame's
    LARGEST bin whatever the order of its sum, so this is the factor by which that error grows in log-mel (t, m).  Above
    ILL_COND = 1e4 (a mel sum 80 dB below the frame's peak: beyond librosa's own top_db) the element is ill-conditioned
    and held to a bound of its own, as tests/_rowop_cases.py holds its low-variance GroupNorm elements."""
    fft, hop, win, mels = geom
    spc = np.abs(FO.stft(w, fft, hop, win)).T
    fb = FO.mel_filterbank(SR, fft, mels, 0, SR / 2)
    mel = spc @ fb.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mel > 0, fb.sum(1)[None, :] * spc.max(1)[:, None] / mel, 0.0)  # an empty filter: log(eps), exact


def _item_errors(got, w, what, geom, errs, key):
    ref = _ref_geom(w.tobytes(), what, geom)
    assert len(ref) == len(got)
    d = np.abs(got.numpy().astype(np.float64) - ref)
    ill = mel_conditioning(w, geom) > ILL_COND if what == "mel" else np.zeros(d.shape, dtype=bool)
    errs[key] = max(errs.get(key, 0.0), float(d[~ill].max()))
    if ill.any():
        errs[key + "-ill"] = max(errs.get(key + "-ill", 0.0), float(d[ill].max()))


def _geom_errors(call, what, geom, fft, hop, dev):
    """{'dense' | 'ragged' (| '...-ill': over the ill-conditioned elements): worst abs error against the oracle on the
    unpadded item}; frame counts, shapes and the exact zeros past an item are asserted here"""
    n0, n1, n2 = geometry_lengths(fft, hop)
    errs = {}
    waves = [wave(n0, 30), wave(n0, 31)]
    x, _ = batch(waves, 0.0, dev)
    got = call(x).cpu()
    assert got.shape[:2] == (2, 1 + n0 // hop) and got.dtype == torch.float32
    for b, w in enumerate(waves):
        _item_errors(got[b], w, what, geom, errs, "dense")
    waves = [wave(n0, 30), wave(n1, 32), wave(n2, 33)]
    x, lens = batch(waves, float("nan"), dev)
    got, frames = call(x, lengths=lens)
    got = got.cpu()
    assert frames == [1 + n // hop for n in lens] and got.shape[:2] == (3, 1 + n0 // hop)
    for b, w in enumerate(waves):
        _item_errors(got[b, :frames[b]], w, what, geom, errs, "ragged")
        assert not got[b, frames[b]:].any(), (what, geom, b)  # exact zeros (NaN would count as nonzero)
    return errs


def logmel_in_kernel_order(w, geom):
    """float32 restatement of logmelfilterbank on one item that adds in the order of the STFT's contraction: one fma
    chain over the samples of a tap group in order (SRN_MAX_TAPS taps of the plan's tap width), the groups added to the
    spectrum one after the other (RES_ADD), then magnitude, mel sum and log as the fp32 emulator has them.  Used to
    derive the bound of a geometry whose error on the GPU is the order of the sum (GEOM_OWN)."""
    fft, hop, win, mels = geom
    nb = 1 + fft // 2
    y = np.pad(np.asarray(w, dtype=np.float32), fft // 2, mode="reflect")
    idx = np.arange(fft)[None, :] + hop * np.arange(1 + len(w) // hop)[:, None]
    fr = y[idx].astype(np.float64)                                     # (frames, fft)
    basis = features._dft_basis(fft, win, 2 * nb).astype(np.float64)   # (2 nb, fft), float32 values
    group = features._lib.SRN_MAX_TAPS * GEOMETRIES[geom][1]
    spec = np.zeros((fr.shape[0], 2 * nb), dtype=np.float32)
    for g0 in range(0, fft, group):
        acc = np.zeros_like(spec)
        for k in range(g0, min(g0 + group, fft)):  # the product of two float32 is exact in float64: one rounding, an fma
            acc = (fr[:, k:k + 1] * basis[None, :, k] + acc).astype(np.float32)
        spec = spec + acc
    mag = torch.from_numpy(np.sqrt(spec[:, :nb] ** 2 + spec[:, nb:] ** 2))
    mel_t = torch.from_numpy(np.ascontiguousarray(features._slaney_mel(SR, fft, mels, 0, SR / 2).T, dtype=np.float32))
    return torch.log10(torch.clamp(mag @ mel_t, min=1e-10))


def kernel_order_baseline(geom):
    """worst abs error of logmel_in_kernel_order against the oracle over the items of the geometry's two batches
    (ordinary elements; the ill-conditioned ones have GEOM_TOL['mel-ill'])"""
    ns = geometry_lengths(geom[0], geom[1])
    errs = {}
    for n, seed in ((ns[0], 30), (ns[0], 31), (ns[1], 32), (ns[2], 33)):
        w = wave(n, seed)
        _item_errors(logmel_in_kernel_order(w, geom), w, "mel", geom, errs, "order")
    return errs["order"]


def geometry_mel_errors(geom, dev):
    fft, hop, win, mels = geom
    kw = dict(fft_size=fft, hop_size=hop, win_length=win, num_mels=mels)
    return _geom_errors(lambda x, **k: features.logmelfilterbank(x, SR, **kw, **k), "mel", geom, fft, hop, dev)


def geometry_loud_errors(hop, mode, dev):
    return _geom_errors(lambda x, **k: features.loudness_extract(x, SR, hop, pad_mode=mode, **k), "loud", (hop, mode),
                        LOUD_FFT, hop, dev)


def check_geometry(what, key, errs, share=1.0, own=True):
    """every figure printed, then held to `share` of its bound; own: a geometry listed in GEOM_OWN by that bound"""
    assert GEOM_TOL[what][1] <= TOL
    bounds = {k: GEOM_TOL[what + "-ill" if k.endswith("-ill") else what][1] for k in errs}
    if own and what == "mel" and key in GEOM_OWN:
        bounds = {k: max(v, GEOM_OWN[key][1]) for k, v in bounds.items()}
    for k, e in errs.items():
        print(f"{what} {key} {k}: max abs err {e:.3e} (bound {bounds[k]:.1e})")
    assert all(e <= share * bounds[k] for k, e in errs.items()), (what, key, errs, bounds)


def empty_filters(geom):
    """how many mel filters of a geometry cover no bin: their column is log10(eps) in the oracle and in the product"""
    fft, _, _, mels = geom
    return int((FO.mel_filterbank(SR, fft, mels, 0, SR / 2).sum(1) == 0).sum())


def _main():
    from tests import _emulator as E
    from tests._rowop_cases import _round_up
    from tests.test_features_ragged_emulated import emul_features
    cpu = torch.device("cpu")
    with E.installed():
        features.ops.CallOp.__call__ = lambda self_, stream=None: emul_features(self_.name, self_.targs)
        features._PLANS.clear()
        mels = [geometry_mel_errors(g, cpu) for g in GEOMETRIES]
        louds = [geometry_loud_errors(h, m, cpu) for h in LOUD_HOPS for m in PAD_MODES]
    features._PLANS.clear()
    worst = lambda lst, ill: max(v for e in lst for k, v in e.items() if k.endswith("-ill") == ill)  # noqa: E731
    for what, v in (("mel", worst(mels, False)), ("mel-ill", worst(mels, True)), ("loud", worst(louds, False))):
        print(f'    "{what}": ({v:.3e}, {_round_up(4 * v):.1e}),')
    for geom in GEOM_OWN:
        v = kernel_order_baseline(geom)
        print(f"    {geom}: ({v:.3e}, {_round_up(4 * v):.1e}),")


if __name__ == "__main__":
    _main()
