"""The cases of tests/_harvest_cases.py are fit to be judged: no GPU here, only the float64 restatement against itself.

tests/test_zzzz_hip_harvest_sweep.py holds every stage of harvest.hip to tests/_harvest_ref.py on inputs made for one stage
each.  That only judges a kernel if the restatement decides the input (few or no near-ties) and if the input reaches
the branch it was made for: an event next to a tile boundary, a run of exactly 10 channels beside one of exactly 9, a
window clamped at both ends, a section dropped and one kept, a gap filled and one left, an extension that gives up
after four misses, an overlap merged each way.  A case that misses a condition is replaced, never excused.

Measured when the cases were chosen: no near-tie in any raw-candidate, refinement or contour case; the contour items of
1500 / 700 / 257 frames leave 15 / 7 / 3 voiced sections; STEP4_GAP = 8 would change 32 frames of their reference and
EXTEND_MISSES = 3 would change 20."""
import numpy as np
import pytest

from tests import _harvest_cases as C
from tests import _harvest_ref as R


# ------------------------------------------------------------------------------------------------ 1. decimation
def test_decimation_lengths_sit_on_the_tile_of_1024():
    want = {16000: (2, 140), 32000: (4, 140), 40000: (5, 140), 44100: (6, 144), 96000: (12, 144)}
    for fs in C.DEC_FS:
        ratio, lag = C.dec_geometry(fs)
        assert (ratio, lag) == want[fs]
        lens = C.dec_lengths(fs)
        walked = [n + 2 * lag + 18 for n in lens]
        assert {1023, 1024, 1025} <= set(walked) and {1, 2, ratio, ratio + 1} <= set(lens) and ratio - 1 in lens + [0]
        assert ({2048, 2049} <= set(walked)) == (ratio == 2)
        for dtype in ("float64", "float32"):
            for x, y in zip(C.dec_items(fs, dtype), C.dec_ref(fs, dtype)):
                assert len(y) == -(-len(x) // ratio) and np.isfinite(y).all()
            assert C.dec_ref(fs, dtype)[0][0] == 0.0  # one sample: nothing is left after the mean is taken
        print(f"fs {fs}: ratio {ratio}, lag {lag}, lengths {lens}")


# ------------------------------------------------------------------------------------------------ 2. raw candidates
def test_raw_candidate_items_are_decided_and_have_events_at_the_tile_boundary():
    g = R.geometry(C.FS8, *C.RAW_RANGE)
    kinds = np.zeros(4, dtype=bool)
    for y, (raw, near) in zip(C.raw_items(), C.raw_ref()):
        share = near.mean()
        chans = int(((raw > 0) & ~near).any(1).sum())
        print(f"{len(y)} samples: near share {share:.4f}, channels with a decided candidate {chans}")
        assert share < 0.01
        if len(y) < 255:
            assert not raw.any()
            continue
        assert chans >= 10
        for b in g["boundary"]:
            f = R.filtered_signal(y, b, float(C.FS8))
            d = f[1:] - f[:-1]  # g[:-1] - g[1:] with g = -f
            for k, v in enumerate((f, -f, d, -d)):
                e = R._events(v)
                e = e[e >= 200.0]
                kinds[k] |= bool((np.abs(e - C.CH_TILE * np.round(e / C.CH_TILE)) <= 1.0).any())
    assert kinds.all(), kinds


# ------------------------------------------------------------------------------------------------ 4. official candidates
def test_synthetic_raw_has_the_runs_it_is_named_for():
    g = R.geometry(C.FS8)
    assert (g["n_ch"], g["n_base"], g["n_cand"], g["voice_range_minimum"]) == (152, 15, 105, 29)
    raw, runs = C.synthetic_raw(257, 0)
    off = R.official_candidates(np.asarray(raw))[:, :15]
    found = (off > 0).sum(1)
    want = np.array([sum(r >= 10 for r in fr) for fr in runs])
    print(f"official candidates per frame: up to {found.max()}; runs of 9 / 10 / 11 over all frames: "
          f"{[sum(fr.count(n) for fr in runs) for n in (9, 10, 11)]}")
    assert np.array_equal(found, want)
    assert found[0] == 13 and found[1] == 2 and found[2] == 0 and found[3] == 4
    assert all(any(n in fr for fr in runs[4:]) for n in C.RUN_LENGTHS)
    assert (np.asarray(raw) < 0).any() and raw[0, 2] > 0 and raw[151, 2] > 0
    m = C.minimal_raw()
    cand = R.official_candidates(np.asarray(m))
    assert cand.shape == (2, 7) and cand[0, 0] > 0 and cand[1, 0] == 0  # ten channels make a candidate, nine do not
    assert cand[1, 1] == cand[0, 0] and cand[0, 4] == 0  # frame 1 takes frame 0's; frame 0 finds nothing in frame 1


# ------------------------------------------------------------------------------------------------ 5. refinement
def test_refinement_groups_survive_and_are_decided(monkeypatch):
    refs, cands = C.refine_ref(), C.refine_cand()
    assert cands[0].shape == (1001, 105) and cands[1].shape == (13, 105)
    alive = {name: 0 for name in C.REF_GROUPS}
    for name, item, fr, f, col in C.refine_entries():
        refined, score, near = refs[item]
        assert cands[item][fr, col] == f and not near[fr, col], (name, fr)
        alive[name] += int(score[fr, col] > 0)
        print(f"{name}: item {item} frame {fr} {f} Hz -> {refined[fr, col]:.3f} Hz, score {score[fr, col]:.2f}")
    assert alive.pop("far") == 0 and min(alive.values()) >= 1, alive
    assert sum((c > 0).sum() for c in cands) == len(C.refine_entries()) and not any(r[2].any() for r in refs)
    fs = float(C.FS8)
    hw = lambda f: int(R.REFINE_WINDOW_PERIODS * fs / f + 1.0)
    assert [2 * hw(f) + 1 for f in (71.0, 387.0, 387.2, 100.0)] == [341, 65, 63, 243]
    assert [min(int(fs / 2 / f), 6) for f in (660.0, 666.0, 666.7, 670.0)] == [6, 6, 5, 5]
    # the far candidate dies by its score, not by the range: with the threshold off it is refined inside the range
    (_, item, fr, f, col), = [e for e in C.refine_entries() if e[0] == "far"]
    monkeypatch.setattr(R, "SCORE_THRESHOLD", 0.0)
    r, s, _ = R.refine(np.asarray(C.refine_signals()[item]), fs, np.asarray(cands[item]), 71.0, 800.0)
    print(f"far: raw score {s[fr, col]:.3f}, refined {r[fr, col]:.2f} Hz")
    assert 0.0 < s[fr, col] < 2.4 and 71.0 < r[fr, col] < 800.0


# ------------------------------------------------------------------------------------------------ 6. contour
def _merge_branches(f0, cand, score):
    """R._fix_step3 once more, recording what it does: (output, sections whose extension gave up after EXTEND_MISSES
    empty frames, list of merge branches taken)"""
    ties = R._Ties()
    F = len(f0)
    secs, gave_up = [], 0
    for st, ed in R._boundaries(f0):
        ext = np.zeros(F)
        ext[st:ed + 1] = f0[st:ed + 1]
        lim = min(F - 2, ed + R.EXTEND_FRAMES)
        ed2 = R._extend(ext, F, ed, lim, 1, cand, ties)
        gave_up += int(ed2 + R.EXTEND_MISSES <= lim and not ext[ed2 + 1:ed2 + 1 + R.EXTEND_MISSES].any())
        st2 = R._extend(ext, F, st, max(1, st - R.EXTEND_FRAMES), -1, cand, ties)
        secs.append((st2, ed2, ext))
    kept, mean_f0 = [], 0.0
    for st, ed, ext in secs:
        for j in range(st, ed):
            mean_f0 += ext[j]
        mean_f0 /= ed - st
        if R.EXTEND_MEAN_RULE / mean_f0 < ed - st:
            kept.append((st, ed, ext))
    branches = []
    if not kept:
        return f0.copy(), gave_up, branches
    kept.sort(key=lambda s: s[0])
    st1, ed1, first = kept[0]
    out = first.copy()
    for st2, ed2, f2 in kept[1:]:
        if st2 - ed1 > 0:
            branches.append("apart")
            out[st2:ed2 + 1] = f2[st2:ed2 + 1]
            ed1 = ed2
        elif st1 <= st2 and ed1 >= ed2:
            branches.append("inside")
        else:
            s1 = sum(R._search_score(out[i], cand[i], score[i]) for i in range(st2, ed1 + 1))
            s2 = sum(R._search_score(f2[i], cand[i], score[i]) for i in range(st2, ed1 + 1))
            branches.append("first wins" if s1 > s2 else "second wins")
            lo = ed1 if s1 > s2 else st2
            out[lo:ed2 + 1] = f2[lo:ed2 + 1]
            ed1 = ed2
    return out, gave_up, branches


def _stages(F1, seed):
    cand, score = (np.asarray(a) for a in C.contour_input(F1, seed))
    ties = R._Ties()
    c2, s2 = R.remove_unreliable(cand, score, ties)
    best = np.argmax(s2, axis=1)
    base = np.where(s2[np.arange(F1), best] > 0.0, c2[np.arange(F1), best], 0.0)
    f1 = R._fix_step1(base, ties)
    f2 = R._fix_step2(f1, 29)
    f3, gave_up, branches = _merge_branches(f2, c2, s2)
    assert np.array_equal(f3, R._fix_step3(f2, c2, s2, ties))
    f4 = R._fix_step4(f3)
    assert np.array_equal(f4, C.contour_ref(F1, seed)["unsmoothed"])
    return dict(cand=cand, base=base, f1=f1, f2=f2, f3=f3, f4=f4, gave_up=gave_up, branches=branches)


@pytest.mark.parametrize("batch,i", [(b, i) for b in range(len(C.CONTOUR_BATCHES)) for i in range(3)])
def test_contour_items_are_decided(batch, i):
    F1, seed = C.CONTOUR_BATCHES[batch][i], C.contour_seed(batch, i)
    c = C.contour_ref(F1, seed)
    sections = len(R._boundaries(np.asarray(c["unsmoothed"])))
    print(f"{F1} frames (seed {seed}): {c['ties']} ties, {sections} sections, {int((c['unsmoothed'] > 0).sum())} voiced frames")
    assert c["ties"] == 0
    assert F1 < 700 or sections >= 5
    cand = C.contour_input(F1, seed)[0]
    assert ((cand > 0).sum(1) <= 105).all() and cand.shape == (F1, 105)


def test_contour_items_start_and_end_at_the_edges():
    seeds = [C.contour_seed(b, i) for b in range(len(C.CONTOUR_BATCHES)) for i in range(3)]
    assert {s % 3 for s in seeds[:3]} == {0, 1, 2} and {s % 2 for s in seeds[:3]} == {0, 1}
    for (F1, seed) in zip(C.CONTOUR_BATCHES[0], seeds):
        cand = np.asarray(C.contour_input(F1, seed)[0])
        live = np.nonzero(cand.any(1))[0]
        assert live[0] <= seed % 3 and cand[seed % 3].any() and live[-1] >= F1 - 1 - seed % 2 and cand[F1 - 1 - seed % 2].any()


def test_contour_branches_are_taken(monkeypatch):
    dropped = kept = filled = left = gave_up = 0
    branches = []
    lengths, gaps = set(), set()
    for F1, i in ((1500, 0), (700, 1)):
        st = _stages(F1, C.contour_seed(0, i))
        for a, b in R._boundaries(st["f1"]):
            lengths.add(b - a + 1)
            dropped += b - a < 29
            kept += b - a >= 29
        bd = R._boundaries(st["f3"])
        for (a0, b0), (a1, b1) in zip(bd[:-1], bd[1:]):
            gaps.add(a1 - b0 - 1)
            filled += a1 - b0 - 1 < R.STEP4_GAP
            left += a1 - b0 - 1 >= R.STEP4_GAP
        gave_up += st["gave_up"]
        branches += st["branches"]
    print(f"step 2: {dropped} sections dropped, {kept} kept (lengths {sorted(lengths)}); step 3: {gave_up} extensions gave up, "
          f"merges {sorted(set(branches))}; step 4: {filled} gaps filled, {left} left (gaps {sorted(gaps)})")
    assert dropped and kept and {29, 30} <= lengths  # 29 frames: ed - st = 28 < voice_range_minimum, 30 frames: kept
    assert filled and left and {8, 9} <= gaps
    assert gave_up and {"first wins", "second wins", "apart"} <= set(branches)
    # the cases sit on the two constants: moving either changes the reference
    for name, value in (("STEP4_GAP", 8), ("EXTEND_MISSES", 3)):
        moved = 0
        for F1, i in ((1500, 0), (700, 1)):
            seed = C.contour_seed(0, i)
            cand, score = (np.asarray(a) for a in C.contour_input(F1, seed))
            with monkeypatch.context() as m:
                m.setattr(R, name, value)
                wrong = R.contour(cand, score, 71.0, 1.0)["unsmoothed"]
            moved += int(np.count_nonzero(wrong != C.contour_ref(F1, seed)["unsmoothed"]))
        print(f"{name} = {value}: {moved} frames of the reference change")
        assert moved > 0, name
    assert np.array_equal(R.contour(cand, score, 71.0, 1.0)["unsmoothed"], C.contour_ref(F1, seed)["unsmoothed"])
