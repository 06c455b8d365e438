"""The cases of tests/_world_cases.py are fit to be judged: no GPU here, only the float64 oracle against itself.

tests/test_hip_world_sweep.py holds CheapTrick and D4C to 1e-6 of oracle/world_oracle.py and asserts the Love-Train
decision frame by frame.  Both only judge the kernels if (a) the oracle's own output is far steadier than the bound
on these inputs -- it differences running sums, so a badly conditioned input would turn summation order into an
"error" -- and (b) no asserted decision sits on its threshold.  These are conditions on the inputs: a case that misses
one is replaced (another seed, another noise level), never excused, and no bound moves.

Measured when the cases were chosen (largest movement of the oracle under x -> x (1 + 1e-15 randn)): log envelope
2.6e-9 over the 0.4 s signals (fs 16000 / 24000, transforms 512 / 1024 / 2048), 2.5e-13 over the signals shorter than
a window; band aperiodicity 1.9e-10 dB over the pulse trains, 1.0e-10 dB at fs = 12000; smallest distance of a
Love-Train share from 0.85: 0.147 on the pulse trains, 0.030 on the noise.  The one frame of the two-sample signal is
a step: D4C calls it voiced (share 0.987) and its aperiodicity is a ratio of rounding residues that moves by 1e-7 dB
whatever the seed, so its values are not compared (its decision and the properties are)."""
import numpy as np
import pytest

from oracle import world_oracle as W
from tests import _world_cases as C
from tests.test_world import song


@pytest.mark.parametrize("case", C.CT_CASES, ids=repr)
def test_cheaptrick_cases_are_well_conditioned(case):
    sp, mc = C.ct_ref(case)
    n = len(case.x) // (case.fs // 200) + 1
    assert sp.shape == (n, (case.fft_size or 1024) // 2 + 1) and mc.shape == (n, C.ORDER + 1)
    assert np.isfinite(sp).all() and (sp > 0).all()
    moved = C.ct_moved(case)
    print(f"{case}: the oracle's log envelope moves by {moved:.2e}")
    assert moved < C.MOVE, (case, moved)


def test_cheaptrick_cases_reach_the_branches_they_are_named_for():
    by = {c.name: c for c in C.CT_CASES}
    floor = C.ct_floor(C.FS, 1024)
    default = W.cheaptrick_frame  # F0 at or below the floor is analysed at WORLD's default F0
    for name in ("ct-24k-zero", "ct-24k-floor"):
        c = by[name]
        assert (c.f0 <= floor).all()
        assert np.array_equal(C.ct_ref(c)[0][7], default(c.x, c.fs, W.DEFAULT_F0, c.t[7], 1024))
    c = by["ct-24k-floor_next"]
    assert (c.f0 > floor).all() and c.f0[0] - floor < 1e-13
    assert not np.array_equal(C.ct_ref(c)[0][7], default(c.x, c.fs, W.DEFAULT_F0, c.t[7], 1024))
    # the largest windows that fit their transforms
    assert 2 * W.matlab_round(1.5 * C.FS / 70.6) + 1 == 1021 and 2 * W.matlab_round(1.5 * C.FS / 35.3) + 1 == 2041
    assert 2 * W.matlab_round(1.5 * C.FS / float(c.f0[0])) + 1 <= 1024
    assert 141.0 < C.ct_floor(C.FS, 512) < 141.5 and 35.0 < C.ct_floor(C.FS, 2048) < 35.3
    assert list(by["ct-24k-alternating"].f0[:4]) == [0.0, 70.6, 5999.0, 0.0]
    # shorter than a window: 1 frame up to 119 samples, 2 from 120 on; one sample -> the additive floor at every bin
    assert [len(by[f"ct-short-{L}-71"].t) for L in (1, 2, 60, 119, 120, 121)] == [1, 1, 1, 1, 2, 2]
    for v in ("0", "71", "5999"):
        assert np.abs(np.log(C.ct_ref(by[f"ct-short-1-{v}"])[0]) + 36.27).max() < 0.01


@pytest.mark.parametrize("case", C.D4C_CASES, ids=repr)
def test_d4c_cases_are_decided_and_well_conditioned(case):
    bap, share = C.d4c_ref(case)
    bap_p, share_p = C.d4c_moved(case)
    voiced, voiced_p = C.voiced_rows(bap), C.voiced_rows(bap_p)
    decided, compared = C.d4c_decided(case), C.d4c_compared(case)
    moves = C.d4c_frame_moves(case)
    print(f"{case}: {int(voiced.sum())} of {len(share)} frames voiced, share at least {np.abs(share - C.THRESHOLD).min():.3f} "
          f"off the threshold, the oracle's bands move by {moves[compared].max(initial=0.0):.2e} dB on the compared frames "
          f"({moves.max():.2e} dB on all)")
    assert np.isfinite(bap).all()
    assert np.array_equal(voiced[decided], voiced_p[decided])  # a decision off the threshold does not flip
    assert (share > C.THRESHOLD)[voiced].all()
    if case.kind == "pulses":  # no frame may be left out, and every one is voiced
        assert decided.all() and compared.all() and voiced.all()
    elif case.kind == "unvoiced":
        assert decided.all() and not voiced.any()
    assert moves[compared].max(initial=0.0) < C.MOVE


def test_ragged_batch_is_decided():
    b = C.ragged_batch()
    assert b["frames"] == [81, 2, 1] and [len(f) for f in b["lf0"]] == [41, 3, 1]
    for i in range(3):
        ref = C.ragged_ref(i)
        assert ref["ok"] and len(ref["f0"]) == b["frames"][i]
        live = ref["f0"] > 0
        assert live.any() and C.off_threshold(ref["share"][live]).all(), (i, ref["share"])
    assert (C.ragged_ref(0)["f0"] == 0).any()


def test_clamped_love_train():
    """Below fs = 15.8 kHz the 7.9 kHz limit of the Love Train lies past Nyquist: the oracle stops at Nyquist there (it
    used to raise) and is unchanged, bit for bit, where the limit fits."""
    def unclamped(x, fs, f0, position):  # the function as it stood before the clamp
        fft_size = 2 ** (1 + int(np.log(3.0 * fs / 40.0 + 1) / np.log(2.0)))
        b0, b1, b2 = (int(np.ceil(f * fft_size / fs)) for f in (100.0, 4000.0, 7900.0))
        spec = np.fft.rfft(W._d4c_windowed(x, fs, max(f0, 40.0), position, "blackman", 3.0), fft_size)
        p = spec.real ** 2 + spec.imag ** 2
        p[:b0 + 1] = 0.0
        c = np.cumsum(p)
        return 0.0 if c[b2] <= 0.0 else c[b1] / c[b2]
    x, f0 = song(0.5)
    t = W.harvest_time_axis(len(x), 24000)
    live = np.nonzero(f0)[0]
    assert len(live) > 50
    for i in live:
        assert W.d4c_love_train(x, 24000, float(f0[i]), t[i]) == unclamped(x, 24000, float(f0[i]), t[i])
    y = C.pulses(12000, 200.0, 0.4)
    with pytest.raises(IndexError):
        unclamped(y, 12000, 200.0, 0.1)
    assert 0.99 < W.d4c_love_train(y, 12000, 200.0, 0.1) <= 1.0  # all of 100 Hz .. Nyquist over itself, less 4 .. 6 kHz
    assert 0.3 < W.d4c_love_train(C.noise(4800, 3), 12000, 200.0, 0.1) < 0.85


def test_contour_and_excitation_cases_cross_a_chunk():
    assert {len(f) for _, f in C.cont_items()} == set(C.CONT_LENGTHS) and max(C.CONT_LENGTHS) > 2 * 256
    refs = dict(zip((label for label, _ in C.cont_items()), C.cont_refs()))
    assert not refs["zero-600"][2] and refs["gap-600"][2] and refs["voiced-1"][2]
    gap = refs["gap-600"][1]
    assert (np.diff(gap[199:402], 2).__abs__() < 1e-9).all() and gap[300] > 0  # one straight line across the gap
    for f, ref, (n_in, n_out) in zip(C.match_inputs(), C.match_refs(), C.MATCH_PAIRS):
        assert ref.shape == (n_out,) and (f.min() < 0) and ((ref.min() < 0) == (n_in == n_out))
        assert n_in == n_out or n_out < 5 or (ref == 0).any()  # the clamp at 0 bites
    e = C.excitation_batch()
    assert e["f0"].shape == (5, 600) and (e["f0"][0, 250:262] == 0).all() and (e["cf0"][0, :600] > 0).all()
