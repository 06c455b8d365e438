"""The Harvest kernels on the MI355X (csrc/harvest.hip through serenade_amd/harvest.py) at the edge cases of
tests/_harvest_cases.py against the float64 restatement tests/_harvest_ref.py, one stage at a time and every stage on
ragged batches: the decimator at five ratios and at lengths of 1, 2 and ratio +- 1 samples and around its 1024-sample
tile; the channel kernel at lengths around its 256-sample tile; the channel launches split into ranges and the batch
split into items under patched budgets (bit-equal to the unsplit call); official candidates from synthetic runs of 9,
10 and 11 channels; refinement of hand-placed candidates (windows of 341, 65, 63 samples, one clamped at both ends,
6 and 5 harmonics); the contour from synthetic candidates with sections, gaps and dropouts on the constants of steps
2 - 4.  tests/test_harvest_cases_host.py proves on the CPU that each input is decided and reaches its branch.

The kernel's header claims every rounding is the restatement's, so each case also prints its largest difference and
whether it was bit-equal.

The file is named to sort after every other test file (like the test_zz_ / test_zzz_ files before it), so that the
suite that was there before runs in the order and from the state it ran in without it."""
import numpy as np
import pytest
import torch

from serenade_amd import harvest as H
from tests import _harvest_cases as C
from tests import _harvest_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(items, fill, dtype=torch.float64, extra=0):
    """(B, longest + extra) with every tail holding `fill`, which nothing may read"""
    lens = [len(v) for v in items]
    x = torch.full((len(items), max(lens) + extra), fill, dtype=dtype)
    for i, v in enumerate(items):
        x[i, :len(v)] = torch.from_numpy(np.array(v)).to(dtype)
    return x.to(DEV), lens


def _plan(lens, fs=C.FS8, floor=71.0, ceil=800.0, f64=True):
    H._check(fs, floor, ceil, 1.0)
    return H._plan(torch.device(DEV), len(lens), max(lens), tuple(lens), (float(fs), float(floor), float(ceil), 1.0, f64))


def _fill(buf, rows, fill):
    """rows[b] into buf[b, :len], `fill` everywhere else (buf is (B, n, ...) and rows[b] is (len_b, ...))"""
    buf.fill_(fill)
    for b, a in enumerate(rows):
        buf[b, :len(a)] = torch.from_numpy(np.array(a)).to(DEV)


def _rel(got, ref, where):
    return float((np.abs(got - ref)[where] / np.abs(ref[where])).max()) if where.any() else 0.0


def _say(what, err, got, ref):
    print(f"{what}: {err:.2e} ({'bit-equal' if np.array_equal(got, ref) else 'not bit-equal'})")


# ------------------------------------------------------------------------------------------------ 1. decimation
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("fs", C.DEC_FS)
def test_decimation(fs, dtype):
    items, refs = C.dec_items(fs, dtype), C.dec_ref(fs, dtype)
    tdt = getattr(torch, dtype)
    plan = _plan([len(v) for v in items], fs, f64=dtype == "float64")
    ratio = plan.g["ratio"]
    outs = []
    for fill, extra in ((1e4, 0), (float("nan"), 0), (1e4, 29)):  # the last: a view wide[:, :N] of a wider tensor
        x, lens = _batch(items, fill, tdt, extra)
        x = x[:, :max(lens)]
        assert (x.stride(0) > x.shape[1]) == (extra > 0)
        plan.y.fill_(float("nan"))
        plan.decimate(x, None)
        torch.cuda.synchronize()
        outs.append(plan.y.cpu().numpy().copy())
    worst = 0.0
    for b, (v, ref) in enumerate(zip(items, refs)):
        got = outs[0][b, :len(ref)]
        assert len(ref) == -(-len(v) // ratio)
        err = np.abs(got - ref).max() / np.abs(np.asarray(v, dtype=np.float64)).max()
        worst = max(worst, err)
        assert err <= C.DEC_TOL, (fs, len(v), err)
        for o in outs[1:]:
            assert np.array_equal(o[b, :len(ref)], got), (fs, len(v))
    assert outs[0][0, 0] == 0.0  # one sample: exactly nothing is left after the mean is taken
    print(f"fs {fs} {dtype}, ratio {ratio}, lengths {[len(v) for v in items]}: {worst:.2e} of the peak "
          f"({'bit-equal' if all(np.array_equal(outs[0][b, :len(r)], r) for b, r in enumerate(refs)) else 'not bit-equal'})")


# ------------------------------------------------------------------------------------------------ 2. raw candidates
def test_raw_candidates_around_the_tile_of_256():
    ys, refs = C.raw_items(), C.raw_ref()
    plan = _plan([len(y) for y in ys], C.FS8, *C.RAW_RANGE)
    assert plan.g["ratio"] == 1 and plan.ylens == [len(y) for y in ys]
    _fill(plan.y, ys, 1e4)
    plan.raw.fill_(float("nan"))
    plan.channels(None)
    torch.cuda.synchronize()
    raw = plan.raw.cpu().numpy()
    for b, (y, (ref, near)) in enumerate(zip(ys, refs)):
        F = ref.shape[1]
        got = raw[b, :, :F]
        both = (got > 0) & (ref > 0) & ~near
        assert not (((got > 0) != (ref > 0)) & ~near).any(), len(y)
        err = _rel(got, ref, both)
        _say(f"raw candidates, {len(y)} samples, {int(both.sum())} compared", err, got, ref)
        assert err <= C.REL_TOL
        assert not raw[b, :, F:].any()  # frames past the item
        assert len(y) >= 255 or not got.any()


# ------------------------------------------------------------------------------------------------ 3. chunked launches
def _two_items():
    sig = R.signals(24000, extra=True)
    return _batch([sig["notes"][0], sig["glide"][0][:9001]], 1e4)


def test_channel_ranges_are_bit_equal(monkeypatch):
    x, lens = _two_items()
    H._PLANS.clear()
    try:
        f0, _ = H.harvest(x, 24000, frame_period=1.0, lengths=lens)
        plan = next(reversed(H._PLANS.values()))
        assert len(plan._channels) == 1 and plan.ch_chunk == 152 and (f0 > 0).any()
        raw0, f00 = plan.raw.clone(), f0.clone()
        for chunk, launches in ((60, 3), (1, 152)):
            H._PLANS.clear()
            monkeypatch.setattr(H, "EVENT_BUDGET", chunk * len(lens) * 4 * plan.ev_cap * 8)
            f1, _ = H.harvest(x, 24000, frame_period=1.0, lengths=lens)
            p = next(reversed(H._PLANS.values()))
            assert p.ch_chunk == chunk and len(p._channels) == launches
            assert torch.equal(p.raw, raw0) and torch.equal(f1, f00), chunk
    finally:
        H._PLANS.clear()


def test_item_chunks_are_bit_equal(monkeypatch):
    sig = R.signals(24000, extra=True)
    x, lens = _batch([sig["notes"][0], sig["glide"][0][:9001], sig["tone440"][0][:5000]], 1e4)
    H._PLANS.clear()
    try:
        f0, _ = H.harvest(x, 24000, frame_period=1.0, lengths=lens)
        assert len(H._PLANS) == 1 and (f0[:2] > 0).any(1).all()
        H._PLANS.clear()
        monkeypatch.setattr(H, "WORKSPACE_BUDGET", H._sizes(H.harvest_geometry(24000), lens, 24000)[4])
        f1, _ = H.harvest(x, 24000, frame_period=1.0, lengths=lens)
        assert len(H._PLANS) == 3 and all(p.B == 1 for p in H._PLANS.values())
        assert torch.equal(f1, f0)
    finally:
        H._PLANS.clear()


# ------------------------------------------------------------------------------------------------ 4. official candidates
@pytest.mark.parametrize("frames", C.OFF_BATCHES, ids=str)
def test_official_candidates_from_synthetic_runs(frames):
    lens = [C.frames_to_samples(F) for F in frames]
    plan = _plan(lens)
    assert plan.frames == list(frames)
    raws = [C.synthetic_raw(F, seed)[0] for seed, F in enumerate(frames)]
    plan.raw.fill_(777.0)  # frames past an item hold a candidate in every channel: nothing may read them
    for b, r in enumerate(raws):
        plan.raw[b, :, :r.shape[1]] = torch.from_numpy(np.array(r)).to(DEV)
    plan.cand.fill_(float("nan"))
    plan.candidates(None)
    torch.cuda.synchronize()
    cand = plan.cand.cpu().numpy()
    for b, r in enumerate(raws):
        ref = C.official_ref(r)
        got = cand[b, :frames[b]]
        assert np.array_equal(got > 0, ref > 0), (frames, b)
        err = _rel(got, ref, ref > 0)
        _say(f"official candidates, {frames[b]} frames of {frames}, {int((ref > 0).sum())} compared", err, got, ref)
        assert err <= C.REL_TOL
        assert not cand[b, frames[b]:].any()


def test_official_candidates_at_the_minimal_geometry():
    raw = C.minimal_raw()
    plan = _plan([C.frames_to_samples(2)], C.FS8, *C.MINIMAL_RANGE)
    assert plan.g["n_ch"] == 12 and plan.g["n_base"] == 1 and plan.frames == [2]
    plan.raw[0].copy_(torch.from_numpy(np.array(raw)).to(DEV))
    plan.candidates(None)
    torch.cuda.synchronize()
    got, ref = plan.cand[0].cpu().numpy(), C.official_ref(raw)
    assert np.array_equal(got > 0, ref > 0) and _rel(got, ref, ref > 0) <= C.REL_TOL
    assert got[0, 0] > 0 and got[1, 0] == 0  # ten channels in a row make a candidate, nine do not


# ------------------------------------------------------------------------------------------------ 5. refinement
def test_refinement_of_hand_placed_candidates():
    ys, cands, refs = C.refine_signals(), C.refine_cand(), C.refine_ref()
    plan = _plan([len(y) for y in ys])
    _fill(plan.y, ys, 1e4)
    _fill(plan.cand, cands, 333.0)  # frames past an item hold candidates: nothing may refine them
    plan.refined.fill_(float("nan"))
    plan.score.fill_(float("nan"))
    plan.refine(None)
    torch.cuda.synchronize()
    refined, score = plan.refined.cpu().numpy(), plan.score.cpu().numpy()
    for b, (ref, sref, near) in enumerate(refs):
        F = len(ref)
        r, s = refined[b, :F], score[b, :F]
        assert not near.any()
        assert np.array_equal(r > 0, ref > 0) and np.array_equal(s > 0, sref > 0), b
        e_r, e_s = _rel(r, ref, ref > 0), _rel(s, sref, sref > 0)
        _say(f"item {b}: refined F0 of {int((ref > 0).sum())} candidates", e_r, r, ref)
        _say(f"item {b}: score", e_s, s, sref)
        assert e_r <= C.REL_TOL and e_s <= C.SCORE_TOL
        assert not refined[b, F:].any() and not score[b, F:].any()
    for name, item, fr, f, col in C.refine_entries():
        print(f"  {name}: {f} Hz at frame {fr} -> {refined[item, fr, col]:.6f} Hz, score {score[item, fr, col]:.4f}")


# ------------------------------------------------------------------------------------------------ 6. contour
def _contour(frames, seeds):
    lens = [C.frames_to_samples(F) for F in frames]
    plan = _plan(lens)
    assert plan.frames == list(frames)
    ins = [C.contour_input(F, s) for F, s in zip(frames, seeds)]
    _fill(plan.refined, [c for c, _ in ins], 222.0)  # frames past an item hold a candidate with a score everywhere
    _fill(plan.score, [s for _, s in ins], 50.0)
    plan.contour(None)
    torch.cuda.synchronize()
    assert plan.status.tolist() == [0] * len(frames)
    out = []
    for b, (F, s) in enumerate(zip(frames, seeds)):
        c = C.contour_ref(F, s)
        c2, s2 = plan.cand2[b, :F].cpu().numpy(), plan.score2[b, :F].cpu().numpy()
        un, sm = plan.unsmoothed[b, :F].cpu().numpy(), plan.smoothed[b, :F].cpu().numpy()
        f0 = plan.f0[b, :F].cpu().numpy()
        assert np.array_equal(c2, c["cand"]) and np.array_equal(s2, c["score"]), (frames, b)
        assert np.array_equal(un, c["unsmoothed"]), (frames, b, np.nonzero(un != c["unsmoothed"])[0][:10])
        assert np.array_equal(sm > 0, c["smoothed"] > 0) and np.array_equal(f0 > 0, c["f0"] > 0)
        err = max(_rel(sm, c["smoothed"], c["smoothed"] > 0), _rel(f0, c["f0"], c["f0"] > 0))
        _say(f"contour, {F} frames of {frames}: unsmoothed bit-equal, {int((un > 0).sum())} voiced frames, smoothed", err,
             sm, c["smoothed"])
        assert err <= C.SMOOTH_TOL
        assert not plan.f0[b, F:].any()
        out.append((un, sm, f0))
    return out


@pytest.mark.parametrize("batch", range(len(C.CONTOUR_BATCHES)), ids=lambda b: str(C.CONTOUR_BATCHES[b]))
def test_contour_from_synthetic_candidates(batch):
    frames = C.CONTOUR_BATCHES[batch]
    seeds = [C.contour_seed(batch, i) for i in range(3)]
    together = _contour(frames, seeds)
    for i in range(3):  # each item alone gives what it gives in the batch
        alone = _contour(frames[i:i + 1], seeds[i:i + 1])[0]
        assert all(np.array_equal(a, b) for a, b in zip(alone, together[i])), (frames, i)
