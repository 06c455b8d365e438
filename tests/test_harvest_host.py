"""Host-side checks of Harvest (serenade_amd/harvest.py) that need no GPU: geometry, the host-built tables, argument
checks, the restatement tests/_harvest_ref.py against the ground truth of synthetic signals, and the near-tie condition
that tests/test_hip_harvest.py relies on."""
import numpy as np
import pytest
import scipy.signal
import torch

from serenade_amd import harvest as H
from serenade_amd import world

from . import _harvest_ref as R

FS = 24000


def test_channel_and_candidate_counts():
    g = H.harvest_geometry(FS, 71.0, 800.0)
    assert g["n_ch"] == 152 and g["n_base"] == 15 and g["n_cand"] == 15 * 7 == 105
    assert H.harvest_geometry(FS, 70.0, 1100.0)["n_ch"] == 171
    for k in ("n_ch", "n_cand", "ratio", "actual_fs", "voice_range_minimum", "half_len"):
        assert g[k] == R.geometry(FS, 71.0, 800.0)[k], k
    assert np.array_equal(g["boundary"], R.geometry(FS, 71.0, 800.0)["boundary"])


@pytest.mark.parametrize("fs,ratio,actual", [(8000, 1, 8000.0), (16000, 2, 8000.0), (24000, 3, 8000.0),
                                             (44100, 6, 7350.0)])
def test_decimation_ratio(fs, ratio, actual):
    g = H.harvest_geometry(fs)
    assert g["ratio"] == ratio and g["actual_fs"] == actual


@pytest.mark.parametrize("n,fs,period", [(12000, 24000, 5.0), (12001, 24000, 1.0), (7, 8000, 5.0), (44100, 44100, 10.0),
                                         (14400, 24000, 5.0)])
def test_frame_counts_time_axis_and_pick(n, fs, period):
    assert H.harvest_frames(n, fs, period) == world.harvest_frame_count(n, fs, period) == R.frame_count(n, fs, period)
    F, F1 = H.harvest_frames(n, fs, period), H.harvest_frames(n, fs, 1.0)
    t = world.harvest_time_axis(n, fs, period)
    assert len(t) == F
    pick = H.harvest_pick(F, F1, period)
    assert pick.tolist() == [min(F1 - 1, int(1000.0 * v + 0.5)) for v in t]
    assert pick.max() <= F1 - 1 and (np.diff(pick) >= 0).all()


def test_filter_tables_are_scipy_bitwise():
    b, a = H.smoothing_table()
    rb, ra = scipy.signal.butter(2, 0.06)
    assert np.array_equal(b, rb) and np.array_equal(a, ra)
    for r in (2, 3, 6, 12):
        b, a = H.decimation_table(r)
        rb, ra = scipy.signal.cheby1(3, 0.05, 0.8 / r)
        assert np.array_equal(b, rb) and np.array_equal(a, ra)


@pytest.mark.parametrize("floor,ceil", R.PARAMETER_SETS)
def test_channel_taps_equal_the_restatement(floor, ceil):
    g = H.harvest_geometry(FS, floor, ceil)
    for bf, hl in zip(g["boundary"], g["half_len"]):
        taps = H.channel_taps(bf, g["actual_fs"])
        assert len(taps) == 2 * hl + 1 and np.array_equal(taps, R.channel_taps(bf, g["actual_fs"]))


def test_longest_filter_fits_the_kernels_at_floor_40():
    g = H._check(FS, 40.0, 800.0, 5.0)
    assert 2 * max(g["half_len"]) + 1 <= H.MAX_TAPS and g["max_window"] <= H.MAX_WINDOW and g["n_cand"] <= H.MAX_CAND
    with pytest.raises(ValueError, match="limits"):
        H._check(FS, 20.0, 800.0, 5.0)


@pytest.mark.parametrize("kw", [dict(f0_floor=0.0), dict(f0_floor=-5.0), dict(f0_floor=800.0, f0_ceil=800.0),
                                dict(f0_floor=900.0), dict(f0_ceil=3700.0), dict(frame_period=0.0),
                                dict(frame_period=-1.0), dict(f0_floor=20.0), dict(lengths=[5]), dict(lengths=[0, 1]),
                                dict(f0_floor=[71.0, 80.0])])
def test_argument_checks_raise_before_the_device(kw):
    x = torch.zeros(4)  # a CPU tensor: a check that passed would raise RuntimeError ("no CPU path") instead
    with pytest.raises(ValueError):
        H.harvest(x, FS, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.harvest(x, FS)
    with pytest.raises(ValueError):
        world.extract_f0(x, FS, 300.0, 200.0, 5.0)


@pytest.mark.parametrize("name", list(R.TRUTH_RECORDED))
def test_restatement_against_ground_truth(name):
    x, truth, check = R.signals(FS)[name]
    ref = R.reference(name)
    voiced, err = R.truth_error(ref["f0"], truth, check)
    print(f"{name}: largest |f0 - true| / true = {err:.3e} over {check.sum()} frames (recorded {R.TRUTH_RECORDED[name]:.3e})")
    assert check.sum() >= 200 and voiced
    assert err <= 2 * R.TRUTH_RECORDED[name]
    if name.startswith("tone"):
        assert err <= 0.01  # a condition on the restatement, not a measurement


def test_restatement_on_silence_is_all_zero():
    x = R.signals(FS)["silence"][0]
    for period in (1.0, 5.0):
        f0, t, near = R.harvest(x, FS, frame_period=period)
        assert len(f0) == world.harvest_frame_count(len(x), FS, period) and not f0.any() and not near
    assert not R.reference("silence")["raw"].any()


def test_restatement_picks_the_requested_period_from_the_1ms_contour():
    x = R.signals(FS)["glide"][0]
    f1 = R.reference("glide")["f0"]
    for period in (5.0, 10.0):
        f0, t, _ = R.harvest(x, FS, frame_period=period)
        assert np.array_equal(f0, f1[H.harvest_pick(len(f0), len(f1), period)])
        assert np.array_equal(t, world.harvest_time_axis(len(x), FS, period))


def test_near_ties_are_rare_on_the_gpu_signal_set():
    """tests/test_hip_harvest.py skips a signal whose restatement reports a near-tie; at most 1 signal in 8 may"""
    names = list(R.signals(FS, extra=True))
    flagged = [(n, p) for p in R.PARAMETER_SETS for n in names if R.reference(n, FS, *p)["near"]]
    print("flagged:", flagged)
    for p in R.PARAMETER_SETS:
        assert 8 * sum(1 for f in flagged if f[1] == p) <= len(names), flagged
