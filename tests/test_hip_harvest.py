"""Harvest on the MI355X (serenade_amd/harvest.py + harvest.hip) against the float64 restatement tests/_harvest_ref.py:
every stage fed by the restatement's previous stage, end to end on tones, glides, vibrato, note sequences, an octave
leap, noise, silence and a short item at three parameter sets, the ground truth of the synthetic signals, other sampling
rates, exact ragged batching, the frame-period pick, a 6 s item and extract_f0.  Signals the restatement flags as
carrying a near-tie are left out of the end-to-end comparison; tests/test_harvest_host.py bounds how many may be.
Tile-boundary lengths, chunked launches and synthetic inputs of every stage: tests/test_zzzz_hip_harvest_sweep.py."""
import numpy as np
import pytest
import torch

from serenade_amd import harvest as H
from serenade_amd import world

from . import _harvest_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FS = 24000


def _batch(waves, fill=1e4, dtype=torch.float64):
    """padded batch; the tail holds large values that nothing may read"""
    lens = [len(w) for w in waves]
    x = torch.full((len(waves), max(lens)), fill, dtype=dtype)
    for i, w in enumerate(waves):
        x[i, :len(w)] = torch.from_numpy(np.asarray(w)).to(dtype)
    return x.to(DEV), lens


def _relmax(got, ref, where):
    return float((np.abs(got - ref)[where] / np.abs(ref[where])).max()) if where.any() else 0.0


def _plan1(x, floor=71.0, ceil=800.0):
    n = len(x)
    plan = H._plan(torch.device(DEV), 1, n, (n,), (float(FS), floor, ceil, 1.0, True))
    return plan, torch.cuda.current_stream().cuda_stream


def _put(buf, a):
    buf.copy_(torch.from_numpy(np.ascontiguousarray(a))[None].to(DEV))


@pytest.mark.parametrize("name", ["tone220", "glide", "notes", "noise", "short"])
def test_stage_by_stage(name):
    """each stage gets the restatement's output of the stage before, so no stage's rounding reaches the next"""
    x = R.signals(FS, extra=True)[name][0]
    ref = R.reference(name)
    plan, st = _plan1(x)
    # decimation
    plan.decimate(torch.from_numpy(x).to(DEV)[None], st)
    y = plan.y[0].cpu().numpy()
    err = np.abs(y - ref["y"]).max() / np.abs(ref["y"]).max()
    print(f"{name}: decimated {err:.2e} of the peak")
    assert err <= 1e-12
    # raw candidates
    _put(plan.y, ref["y"])
    plan.channels(st)
    raw, near = plan.raw[0].cpu().numpy(), ref["near_raw"]
    both = (raw > 0) & (ref["raw"] > 0)
    print(f"{name}: raw {_relmax(raw, ref['raw'], both & ~near):.2e}, {near.sum()} of {near.size} flagged")
    assert raw.shape == ref["raw"].shape and near.mean() < 0.01
    assert not (((raw > 0) != (ref["raw"] > 0)) & ~near).any()
    assert _relmax(raw, ref["raw"], both & ~near) <= 1e-9
    # official + overlapped candidates
    _put(plan.raw, ref["raw"])
    plan.candidates(st)
    cand = plan.cand[0].cpu().numpy()
    assert np.array_equal(cand > 0, ref["cand"] > 0)
    assert _relmax(cand, ref["cand"], ref["cand"] > 0) <= 1e-9
    # refinement
    _put(plan.cand, ref["cand"])
    plan.refine(st)
    refined, score, near = plan.refined[0].cpu().numpy(), plan.score[0].cpu().numpy(), ref["near_ref"]
    both = (refined > 0) & (ref["refined"] > 0)
    print(f"{name}: refined {_relmax(refined, ref['refined'], both):.2e}, score {_relmax(score, ref['score'], both):.2e}")
    assert not (((refined > 0) != (ref["refined"] > 0)) & ~near).any()
    assert not (((score > 0) != (ref["score"] > 0)) & ~near).any()
    assert _relmax(refined, ref["refined"], both) <= 1e-9 and _relmax(score, ref["score"], both) <= 1e-6
    # contour from identical candidates and scores
    _put(plan.refined, ref["refined"])
    _put(plan.score, ref["score"])
    plan.contour(st)
    c = ref["contour"]
    un, sm = plan.unsmoothed[0].cpu().numpy(), plan.smoothed[0].cpu().numpy()
    assert plan.status.tolist() == [0]
    assert np.array_equal(plan.cand2[0].cpu().numpy(), c["cand"]) and np.array_equal(plan.score2[0].cpu().numpy(), c["score"])
    assert np.array_equal(un, c["unsmoothed"])  # every decision and every value before smoothing, bit for bit
    assert np.array_equal(sm > 0, c["smoothed"] > 0)
    assert _relmax(sm, c["smoothed"], c["smoothed"] > 0) <= 1e-12
    assert np.array_equal(plan.f0[0].cpu().numpy() > 0, c["f0"] > 0)


_E2E = {}


def _end_to_end(floor, ceil):
    """the whole signal set as one ragged batch at 1 ms frames (computed once per parameter set)"""
    if (floor, ceil) not in _E2E:
        sig = R.signals(FS, extra=True)
        x, lens = _batch([v[0] for v in sig.values()])
        f0, t = H.harvest(x, FS, floor, ceil, 1.0, lengths=lens)
        _E2E[(floor, ceil)] = (list(sig), lens, f0.cpu().numpy(), t)
    return _E2E[(floor, ceil)]


@pytest.mark.parametrize("floor,ceil", R.PARAMETER_SETS)
def test_end_to_end(floor, ceil):
    names, lens, f0, t = _end_to_end(floor, ceil)
    assert f0.shape == (len(names), max(world.harvest_frame_count(n, FS, 1.0) for n in lens))
    assert np.array_equal(t, world.harvest_time_axis(max(lens), FS, 1.0))
    compared = 0
    for b, name in enumerate(names):
        ref = R.reference(name, FS, floor, ceil)
        F = world.harvest_frame_count(lens[b], FS, 1.0)
        assert len(ref["f0"]) == F and not f0[b, F:].any(), name
        if ref["near"]:
            continue
        compared += 1
        got = f0[b, :F]
        assert np.array_equal(got > 0, ref["f0"] > 0), f"{name}: voiced flags differ at {np.nonzero((got > 0) != (ref['f0'] > 0))[0][:10]}"
        err = _relmax(got, ref["f0"], ref["f0"] > 0)
        print(f"{name} ({floor}, {ceil}): {err:.2e}")
        assert err <= 1e-9, name
    assert 8 * (len(names) - compared) <= len(names)


@pytest.mark.parametrize("name", list(R.TRUTH_RECORDED) + ["silence"])
def test_ground_truth(name):
    names, lens, f0, _ = _end_to_end(71.0, 800.0)
    x, truth, check = R.signals(FS, extra=True)[name]
    got = f0[names.index(name), :len(truth)]
    if name == "silence":
        assert not got.any()
        return
    voiced, err = R.truth_error(got, truth, check)
    print(f"{name}: {err:.3e} (recorded for the restatement: {R.TRUTH_RECORDED[name]:.3e})")
    assert voiced and err <= 2 * R.TRUTH_RECORDED[name]
    assert not name.startswith("tone") or err <= 0.01


@pytest.mark.parametrize("fs", [8000, 16000, 44100])
def test_sampling_rates(fs):
    """the copy path (ratio 1) and two other decimation ratios"""
    for name in ("tone220", "glide"):
        x = R.signals(fs, extra=True)[name][0]
        ref = R.reference(name, fs)
        assert not ref["near"], "pick another seed: this signal carries a near-tie"
        f0, t = H.harvest(torch.from_numpy(x).to(DEV), fs, frame_period=1.0)
        got = f0.cpu().numpy()
        assert got.shape == ref["f0"].shape and np.array_equal(got > 0, ref["f0"] > 0), name
        assert _relmax(got, ref["f0"], ref["f0"] > 0) <= 1e-9, name


def test_ragged_batching_is_exact():
    sig = R.signals(FS, extra=True)
    waves = [sig["notes"][0], sig["glide"][0][:9001], sig["tone440"][0][:5000], sig["short"][0]]
    x, lens = _batch(waves, 1e4)
    a, _ = H.harvest(x, FS, lengths=lens)
    b, _ = H.harvest(_batch(waves, -3.0)[0], FS, lengths=lens)
    assert torch.equal(a, b) and (a[0] > 0).any()
    for i, w in enumerate(waves):
        one, t = H.harvest(torch.from_numpy(w).to(DEV), FS)
        F = world.harvest_frame_count(len(w), FS, 5.0)
        assert one.shape == (F,) and len(t) == F
        assert torch.equal(a[i, :F], one) and not a[i, F:].any(), i
    # float32 widens exactly
    x32, _ = _batch([w.astype(np.float32) for w in waves], 1e4, torch.float32)
    c, _ = H.harvest(x32, FS, lengths=lens)
    d, _ = H.harvest(x32.double(), FS, lengths=lens)
    assert torch.equal(c, d)
    # per-item ranges: two groups, each equal to its own call
    floors, ceils = [71.0, 196.0, 71.0, 196.0], [800.0, 700.0, 800.0, 700.0]
    e, _ = H.harvest(x, FS, floors, ceils, lengths=lens)
    for i, w in enumerate(waves):
        one, _ = H.harvest(torch.from_numpy(w).to(DEV), FS, floors[i], ceils[i])
        assert torch.equal(e[i, :len(one)], one) and not e[i, len(one):].any(), i


def test_frame_periods_are_picks_of_the_1ms_contour():
    x = torch.from_numpy(R.signals(FS)["vibrato"][0]).to(DEV)
    f1, _ = H.harvest(x, FS, frame_period=1.0)
    assert (f1 > 0).any()
    for period in (5.0, 10.0):
        f, t = H.harvest(x, FS, frame_period=period)
        assert len(f) == world.harvest_frame_count(len(x), FS, period)
        pick = torch.from_numpy(H.harvest_pick(len(f), len(f1), period)).to(DEV)
        assert torch.equal(f, f1[pick])
        assert np.array_equal(t, world.harvest_time_axis(len(x), FS, period))


def test_six_second_item():
    """6 001 internal frames and 48 000 decimated samples: indices beyond one tile and one block"""
    x, truth, check = R.long_signal(FS)
    xt = torch.from_numpy(x).to(DEV)
    f1, _ = H.harvest(xt, FS, frame_period=1.0)
    voiced, err = R.truth_error(f1.cpu().numpy(), truth, check)
    print(f"6 s item: {err:.3e} (recorded for the restatement: {R.LONG_RECORDED:.3e})")
    assert len(f1) == 6001 and voiced and err <= 2 * R.LONG_RECORDED
    other = R.signals(FS)["glide"][0]
    pair, lens = _batch([x, other])
    f2, _ = H.harvest(pair, FS, frame_period=1.0, lengths=lens)
    assert torch.equal(f2[0], f1)


def test_extract_f0():
    x = R.signals(FS)["notes"][0]
    xt = torch.from_numpy(x.astype(np.float32)).to(DEV)
    f0, vuv = world.extract_f0(xt, FS, 70, 1100, 5.0)
    T = int(1000 * len(x) / FS / 5.0) + 1
    assert f0.shape == (T, 1) and f0.dtype == torch.float64 and vuv.shape == (T, 1) and vuv.dtype == torch.float32
    assert torch.equal(vuv, (f0 != 0).float()) and vuv.any()
    z0, zv = world.extract_f0(torch.zeros_like(xt), FS, 70, 1100, 5.0)  # a zero signal has no edges: all unvoiced
    assert z0.shape == (T, 1) and not z0.any() and zv.dtype == torch.float32 and not zv.any()
    ref, _ = H.harvest(xt, FS, 70, 1100, 5.0)
    assert torch.equal(f0[:, 0], ref)
    pairs = world.extract_f0(torch.stack([xt, xt]), FS, 70, 1100, 5.0, lengths=[len(x), 6000])
    assert torch.equal(pairs[0][0], f0) and pairs[1][0].shape == (int(1000 * 6000 / FS / 5.0) + 1, 1)
