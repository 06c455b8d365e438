"""The ragged SiFiGAN's host logic on the CPU, through the C-ABI emulator plus the executable specification of the ragged
gather (tests/_sifigan_ragged_emul.py): the ragged SiFiGANPlan (per-rate lengths, len_in on every conv, bucketed capacity,
plan reuse, a cache the dense plan() leaves alone), `forward(lengths=)` / `inference_ragged`, and the CLI option.
The kernel itself is tests/test_zz_hip_sifigan_ragged.py (GPU)."""
import numpy as np
import pytest
import torch

from oracle import sifigan_oracle as SO
from serenade_amd import sifigan
from serenade_amd.bin import ssc_postprocessing as PP
from tests import _emulator, _sifigan_ragged_emul
from tests.test_sifigan import SMALL, _inputs, _model, nerr
from tests.test_zz_hip_sifigan_ragged import branchy_r

LENS = (11, 4, 1, 7)
# What rows past an item's end hold here.  Finite, because the emulator's conv masks its input by a product: junk that a
# missing len_in lets through shows in the result, but a path that multiplied by 0 where it must select would not.  NaN
# behind every item, which tells the two apart, is the GPU file's part (the kernels select).
JUNK = 1.0e3
TOL = 1e-4    # tests/test_sifigan.py's bound against the restatement


def _items(cfg, lens, seed=0):
    """[(x (1, 1, T*hop), c (1, in_ch, T), [d_i])], each item drawn on its own"""
    return [_inputs(cfg, 1, T, seed=seed + 10 * b) for b, T in enumerate(lens)]


def _padded(cfg, items, T=None):
    """the items side by side in dense (B, ., T) tensors, JUNK behind every item's end"""
    T = max(c.shape[2] for _, c, _ in items) if T is None else T
    hop = items[0][0].shape[2] // items[0][1].shape[2]
    ups = [d.shape[2] // items[0][1].shape[2] for d in items[0][2]]
    B = len(items)
    x = torch.full((B, 1, T * hop), JUNK)
    c = torch.full((B, cfg["in_channels"], T), JUNK)
    ds = [torch.full((B, 1, T * u), JUNK) for u in ups]
    for b, (xb, cb, db) in enumerate(items):
        n = cb.shape[2]
        x[b, :, :n * hop], c[b, :, :n] = xb[0], cb[0]
        for dst, src, u in zip(ds, db, ups):
            dst[b, :, :n * u] = src[0]
    return x, c, ds


def _check_items(g, w, cfg, items, outs):
    for (x, c, d), (y, e) in zip(items, outs):
        y_ref, e_ref = SO.sifigan_forward(w, x, c, d, cfg)
        assert y.shape == e.shape == (c.shape[2] * g.hop,)
        assert nerr(y, y_ref.view(-1)) < TOL and nerr(e, e_ref.view(-1)) < TOL, f"item of {c.shape[2]} frames"


def test_ragged_generator_equals_the_restatement_per_item_and_has_zero_tails():
    g, w = _model(SMALL)
    items = _items(SMALL, LENS, seed=3)
    x, c, d = _padded(SMALL, items)
    with _sifigan_ragged_emul.installed():
        outs = g.inference_ragged(items)
        yb, eb = g(x, c, d, lengths=LENS)
        singles = [g(*it) for it in items]
    _check_items(g, w, SMALL, items, outs)
    assert yb.shape == eb.shape == (len(LENS), 1, max(LENS) * g.hop)
    for n, (y, e), (y1, e1), yrow, erow in zip(LENS, outs, singles, yb, eb):
        assert nerr(y, y1.view(-1)) < TOL and nerr(e, e1.view(-1)) < TOL
        assert torch.equal(yrow[0, :n * g.hop], y) and torch.equal(erow[0, :n * g.hop], e)
        assert bool((yrow[0, n * g.hop:] == 0).all()) and bool((erow[0, n * g.hop:] == 0).all())


def test_ragged_plan_is_bucketed_reused_and_masks_stale_rows():
    g, w = _model(SMALL)
    with _sifigan_ragged_emul.installed():
        assert g.plan_ragged(2, 64).T == 64 and g.plan_ragged(2, 65).T == 128
        assert g.plan_ragged(2, 64) is not g.plan_ragged(2, 65)
        assert g.plan_ragged(2, 65, bucket=1).T == 65
        g._invalidate()
        long_, short = _items(SMALL, (40, 33), seed=1), _items(SMALL, (5, 11), seed=2)
        g.inference_ragged(long_)
        pl = g.plan_ragged(2, 40)
        outs = g.inference_ragged(short)
        assert g.plan_ragged(2, 11) is pl and pl.T == 64
        assert pl.lens.tolist() == [[5 * s, 11 * s] for s in pl.scales] and pl.scales == [1, 3, 6]
        _check_items(g, w, SMALL, short, outs)
        # a miss in the dense plan() clears the dense cache, not this one; _invalidate() clears both
        g(*short[0])
        g(*short[1])
        assert g.plan_ragged(2, 11) is pl and len(g._plans) == 1
        g._invalidate()
        assert not g._ragged_plans and not g._plans


def test_length_validation_comes_before_any_plan():
    g, w = _model(SMALL)
    x, c, d = _padded(SMALL, _items(SMALL, (5, 11)))
    with _sifigan_ragged_emul.installed():
        for bad in ((5,), (5, 11, 3), (0, 11), (5, 12)):
            with pytest.raises(ValueError):
                g(x, c, d, lengths=bad)
        with pytest.raises(ValueError):
            g.inference_ragged([])
    assert not g._ragged_plans and not g._plans


def test_batch_utterances_below_one_is_rejected():
    base = ["generator=sifigan", "in_dir=/nowhere", "stats=s.joblib", "checkpoint_path=m.pkl"]
    assert PP.parse_overrides(base)["batch_utterances"] == 1
    assert PP.parse_overrides(base + ["batch_utterances=3"])["batch_utterances"] == 3
    for bad in ("0", "-2", "1.5", "true", ""):
        with pytest.raises(SystemExit):
            PP.parse_overrides(base + [f"batch_utterances={bad}"])
        with pytest.raises(SystemExit):
            PP.main(base + [f"batch_utterances={bad}"])


def test_dense_plan_is_op_for_op_what_build_without_lengths_gives():
    """one walk builds both plans: the ragged one differs from the dense one only in the gather, the output stage and
    the lengths it hands to the same convs (tests/test_vocoder_oplists_emulated.py holds both to their recorded op
    lists)"""
    g, w = _model(SMALL)
    with _emulator.installed():
        dense = sifigan.SiFiGANPlan(g, 2, 11)
        ragged = sifigan.SiFiGANPlan(g, 2, 11, ragged=True)
    name = lambda op: getattr(op, "name", type(op).__name__)
    names = [name(op) for op in dense.ops]
    assert "srn_pd_gather" in names and "srn_out_conv_tanh" in names and not any("ragged" in n for n in names)
    swap = {"srn_pd_gather": "srn_pd_gather_ragged", "srn_out_conv_tanh": "srn_out_conv_tanh_ragged"}
    assert [name(op) for op in ragged.ops] == [swap.get(n, n) for n in names]
    for op_d, op_r in zip(dense.ops, ragged.ops):
        if name(op_d) == "srn_conv_gemm":
            assert op_d.kw.get("len_in") is None and op_r.kw.get("len_in") is not None


def test_branchy_r_reaches_every_branch():
    """the host side of the GPU file's gather cases: an item of >= 7 rows meets every branch the kernel has"""
    for L in (9, 36, 70):
        for dil in (1, 4):
            prod, d = branchy_r(L, dil, 0)
            assert np.array_equal(d.astype(np.float64) * dil, prod)  # exact: the kernel's product is this value
            r, t = np.rint(prod).astype(int), np.arange(L)
            assert (r == 0).any() and (t - r == 0).any() and (t - r == -1).any() and (r > L).any()
            assert (t + r == L - 1).any() and (t + r == L).any()
            ties = prod % 1 == 0.5
            assert ties.any() and (L < 36 or {0.5, 1.5, 2.5} <= set(prod[ties]))  # half-even: 0.5 -> 0, 1.5 and 2.5 -> 2
