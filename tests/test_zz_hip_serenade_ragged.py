"""GPU tests of Serenade with lengths as data: from the two kernels up to `Serenade.inference_ragged(bucket=)`.

* srn_zero_rows_ragged: +0.0 exactly in rows [n_rows[b], rows_cap) of every item and the prefilled sentinel's bits
  everywhere else -- the row before the edge, the gap between items and the guard bands included -- at row widths that
  take the 16-byte stores, the single stores and both, from aligned and misaligned bases;
* srn_gru_recur_last_ragged: every item BIT FOR BIT what srn_gru_recur_last gives on the item's own rows; rows of gi past
  an item's step count hold NaN;
* StyleEncoder.forward(lengths=): across the conv launches agreement is to fp32 summation order (srn_conv_gemm may pick
  another tile or K split for (B, H_cap) than for (1, H_b)), so every item is held against its own B = 1 forward at the
  bound the style encoder is held to against its golden vector (5e-5 of the tensor's maximum, tests/test_hip_parity.py),
  the golden vector itself included; then short prompts on the same plan, behind them the long batch's rows;
* the model: every item of a bucketed batch against its own B = 1 `inference` with the same noise at the bound the
  shape-keyed ragged plan is held to (2e-5, tests/test_hip_configs.py); stale rows of a reused plan, a captured graph
  replayed over new lengths (bit-equal to the eager run), the bucket's edges, a batch of one.

The file's name sorts it behind every other test file: these cases run after the suite that was there before them.
"""
import ctypes

import numpy as np
import pytest
import torch

from serenade_amd import _lib, models, ops
from serenade_amd.utils.synth import SERENADE_PARAMS, synth_inputs
from tests._weights import serenade_weights

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # a quiet NaN with a payload: "never written", and poison if it were read as data
GUARD = 64             # floats of guard band on either side of a buffer
GST_TOL = 5e-5         # tests/test_hip_parity.py: the style encoder against its golden vector
RAGGED_TOL = 2e-5      # tests/test_hip_configs.py: the shape-keyed ragged plan against B = 1 inference
KEYS = ("x", "midi", "lft", "ref_x", "ref_logmel", "ref_midi", "ref_lft")
LONG = [(200, 96), (131, 160), (257, 33), (64, 64)]   # longest R + T = 296: L_cap 320
SHORT = [(190, 70), (40, 9), (250, 47), (12, 5)]      # longest 297: the same bucket


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    m = models.Serenade(**SERENADE_PARAMS)
    m.load_state_dict(serenade_weights())
    return m.eval().to(dev)


def rnd(*s, seed=0, scale=1.0):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal(s)).astype(np.float32))


def nerr(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("misalign", [0, 1, 2])
@pytest.mark.parametrize("n_rows", [(0, 1, 8, 9), (12, 8, 1, 0), (9, 12, 9, 8)])
@pytest.mark.parametrize("n_cols", [1, 3, 4, 80 * 4, 130])
def test_zero_rows_ragged_writes_zeros_behind_the_item_and_nothing_else(dev, n_cols, n_rows, misalign):
    B, cap = 4, 9
    for bs in (cap * n_cols, cap * n_cols + 7):  # items back to back; a gap (and item bases of every alignment)
        total = 2 * GUARD + misalign + B * bs
        buf = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
        ops.zero_rows_ragged_op((buf.view(torch.float32), GUARD + misalign), bs, n_cols,
                                torch.tensor(n_rows, dtype=torch.int32, device=dev), B, cap)()
        want = torch.full((total,), SENTINEL, dtype=torch.int32)
        for b, n in enumerate(n_rows):
            base = GUARD + misalign + b * bs
            want[base + min(n, cap) * n_cols: base + cap * n_cols] = 0  # the bits of +0.0
        assert torch.equal(buf.cpu(), want), (n_cols, n_rows, misalign, bs)


def test_zero_rows_ragged_more_than_one_chunk_per_item(dev):
    """an item wider than a workgroup's span: chunks wholly before the edge return, the edge's chunk is split, the rest
    are whole"""
    B, cap, n_cols = 2, 40, 100  # 4000 floats per item
    n_rows = (27, 3)
    buf = torch.full((B * cap * n_cols,), SENTINEL, dtype=torch.int32, device=dev)
    ops.zero_rows_ragged_op(buf.view(torch.float32), cap * n_cols, n_cols,
                            torch.tensor(n_rows, dtype=torch.int32, device=dev), B, cap)()
    got = buf.cpu().view(B, cap, n_cols)
    for b, n in enumerate(n_rows):
        assert bool((got[b, :n] == SENTINEL).all()) and bool((got[b, n:] == 0).all())


@pytest.mark.parametrize("H", [128, 8])
def test_gru_recur_last_ragged_is_the_dense_call_on_each_items_rows_bit_for_bit(dev, H):
    T_cap, n_steps = 5, (1, 2, 5, 5, 3)
    B = len(n_steps)
    gi = rnd(B, T_cap, 3 * H, seed=H)
    w = (rnd(H, 3 * H, seed=H + 1) / H ** 0.5).to(dev)
    bh = rnd(3 * H, seed=H + 2, scale=0.1).to(dev)
    poisoned = gi.clone()
    for b, n in enumerate(n_steps):
        poisoned[b, n:] = float("nan")
    h = torch.full((B, H), float("nan"), device=dev)
    ops.gru_recur_last_ragged_op(poisoned.to(dev), w, bh, h, torch.tensor(n_steps, dtype=torch.int32, device=dev), B,
                                 T_cap, H)()
    for b, n in enumerate(n_steps):
        ref = torch.full((1, H), float("nan"), device=dev)
        ops.gru_recur_last_op(gi[b:b + 1, :n].contiguous().to(dev), w, bh, ref, 1, n, H)()
        assert not bool(torch.isnan(ref).any()) and torch.equal(h[b:b + 1], ref), (H, b, n)
    # a step count past the cap is the cap
    h2 = torch.full((B, H), float("nan"), device=dev)
    ops.gru_recur_last_ragged_op(gi.to(dev), w, bh, h2, torch.tensor((9, 5, 6, 5, 7), dtype=torch.int32, device=dev), B,
                                 T_cap, H)()
    ref = torch.empty(B, H, device=dev)
    ops.gru_recur_last_op(gi.to(dev), w, bh, ref, B, T_cap, H)()
    assert torch.equal(h2, ref)


def test_bad_arguments_are_refused(dev):
    lib = _lib.lib()
    x = torch.zeros(4 * 9 * 4, device=dev)
    n = torch.zeros(4, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(x=p(x), bs=36, n_cols=4, n_rows=p(n), B=4, rows_cap=9)
    assert lib.srn_zero_rows_ragged(*good.values(), stream()) == 0
    for bad in (dict(x=None), dict(n_rows=None), dict(n_cols=0), dict(B=0), dict(rows_cap=0), dict(n_cols=-4),
                dict(bs=35)):
        assert lib.srn_zero_rows_ragged(*{**good, **bad}.values(), stream()) != 0, bad
        assert b"zero_rows_ragged" in lib.srn_last_error()
    H = 8
    gi, w, bh, h = (torch.zeros(s, device=dev) for s in ((2, 5, 3 * H), (H, 3 * H), (3 * H,), (2, H)))
    ns = torch.ones(2, dtype=torch.int32, device=dev)
    good = dict(gi=p(gi), w=p(w), bh=p(bh), h=p(h), n_steps=p(ns), B=2, T_cap=5, H=H)
    assert lib.srn_gru_recur_last_ragged(*good.values(), stream()) == 0
    for bad in (dict(gi=None), dict(w=None), dict(bh=None), dict(h=None), dict(n_steps=None), dict(B=0), dict(T_cap=0),
                dict(H=0), dict(H=342)):
        assert lib.srn_gru_recur_last_ragged(*{**good, **bad}.values(), stream()) != 0, bad
        assert b"gru_recur_last_ragged" in lib.srn_last_error()
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        ops.zero_rows_ragged_op(x, 36, 4, n.to(torch.int64), 4, 9)
    with pytest.raises(TypeError):
        ops.gru_recur_last_ragged_op(gi, w, bh, h, ns[:1], 2, 5, H)


# ------------------------------------------------------------------------------------------------ style encoder
def _check_style_items(gst, speech, lens, out, what):
    worst = 0.0
    for b, n in enumerate(lens):
        e = nerr(out[b:b + 1], gst(speech[b:b + 1, :n].contiguous()))
        print(f"style encoder, {what}: item {b} of {n} rows: nerr {e:.3e}")
        worst = max(worst, e)
    assert worst < GST_TOL, (what, worst)


def test_style_encoder_lengths_equal_each_prompt_alone(dev, model):
    """33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1 is odd at five layers and 65 at the first, so a missing mask at any layer
    shows; 1 and 5 are shorter than the stack is deep; 128 fills the cap.  Then short prompts on the same plan: the rows
    behind them hold the long batch (staging buffer, image and every layer's output)"""
    gst = model.gst
    gst._plans.clear()
    lens = (33, 64, 65, 5, 1, 128)
    speech = rnd(len(lens), 128, 80, seed=11).to(dev)
    out = gst(speech, lengths=lens)
    (plan,) = gst._plans.values()
    _check_style_items(gst, speech, lens, out, "long batch")
    short = (7, 2, 31, 3, 16, 1)
    out = gst(speech, lengths=torch.tensor(short))
    assert list(gst._plans.values()) == [plan]
    _check_style_items(gst, speech, short, out, "short batch on the same plan")
    for bad in ((33, 64, 65, 5, 1), (33, 64, 65, 5, 1, 129), (33, 64, 65, 5, 0, 128)):
        with pytest.raises(ValueError):
            gst(speech, lengths=bad)


def test_style_encoder_golden_items_between_dummies(dev, model, golden):
    g = golden("gst")
    sp = torch.from_numpy(g["speech"]).to(dev)  # (2, 70, 80)
    cap = 100
    batch = rnd(4, cap, 80, seed=12).to(dev)
    batch[1, :70], batch[2, :70] = sp[0], sp[1]
    out = model.gst(batch, lengths=(41, 70, 70, cap))
    e = nerr(out[1:3], g["style"])
    print(f"style encoder, golden items in a ragged batch: nerr {e:.3e}")
    assert e < GST_TOL


# ------------------------------------------------------------------------------------------------ model
def _items(shapes, seed, dev):
    ds = [synth_inputs(1, t, T_ref=r, seed=seed + i) for i, (t, r) in enumerate(shapes)]
    items = [tuple(d[k][0].to(dev) for k in KEYS) for d in ds]
    return ds, items, [d["z"][0].to(dev) for d in ds]


def _singles(model, ds, dev):
    g = lambda d, k: d[k].to(dev)
    return [model.inference(g(d, "x"), d["lengths"], g(d, "midi"), g(d, "lft"), g(d, "ref_x"), d["ref_lengths"],
                            g(d, "ref_logmel"), g(d, "ref_midi"), g(d, "ref_lft"), noise=g(d, "z")) for d in ds]


@pytest.fixture(scope="module")
def batches(dev, model):
    """the two batches of one bucket with their B = 1 results, computed once"""
    long_, short = _items(LONG, 500, dev), _items(SHORT, 600, dev)
    return dict(long=long_, short=short, long_ref=_singles(model, long_[0], dev),
                short_ref=_singles(model, short[0], dev))


def _bucket_plans(model):
    return {k: v for k, v in model._plans.items() if k[0] == "ragged-bucket"}


def _check_items(shapes, outs, refs, what):
    worst = 0.0
    for i, ((t, r), o, s) in enumerate(zip(shapes, outs, refs)):
        assert o.shape == (t, 80)
        e = nerr(o, s)
        print(f"bucketed plan, {what}: item {i} (T {t}, R {r}): nerr {e:.3e}")
        worst = max(worst, e)
    assert worst < RAGGED_TOL, (what, worst)


def test_bucketed_batch_equals_b1_runs_then_a_short_batch_on_the_same_plan(dev, model, batches):
    model._plans.clear()
    _, items, noises = batches["long"]
    outs = model.inference_ragged(items, noises=noises, bucket=models.RAGGED_BUCKET)
    ((key, plan),) = _bucket_plans(model).items()
    assert key[:3] == ("ragged-bucket", 4, 320)
    _check_items(LONG, outs, batches["long_ref"], "long batch")
    _, items, noises = batches["short"]
    outs = model.inference_ragged(items, noises=noises, bucket=models.RAGGED_BUCKET)
    assert _bucket_plans(model) == {key: plan}
    _check_items(SHORT, outs, batches["short_ref"], "short batch on the same plan")


def test_captured_graph_is_replayed_over_new_lengths(dev, model, batches):
    """graphs on: eager warm-up, capture, then the SAME graph replayed over the short batch and the long batch's
    leftovers -- bit-equal to the eager run of that sequence"""
    (_, long_items, long_z), (_, short_items, short_z) = batches["long"], batches["short"]
    run = lambda items, z: model.inference_ragged(items, noises=z, bucket=models.RAGGED_BUCKET)
    model._plans.clear()
    model.cfm_decoder.estimator._plans.clear()
    run(long_items, long_z)
    eager = run(short_items, short_z)
    ops.set_graphs(True)
    try:
        model._plans.clear()
        model.cfm_decoder.estimator._plans.clear()
        run(long_items, long_z)            # eager warm-up of a new plan
        first = run(long_items, long_z)    # captured
        ((_, plan),) = _bucket_plans(model).items()
        replay = run(short_items, short_z)  # replayed over new lengths
        assert list(_bucket_plans(model).values()) == [plan]
        assert plan._runner._graph is not None and plan.pl._runner._graph is not None
    finally:
        ops.set_graphs(False)
        model._plans.clear()
        model.cfm_decoder.estimator._plans.clear()
    for a, b in zip(replay, eager):
        assert torch.equal(a, b)
    _check_items(LONG, first, batches["long_ref"], "captured")
    _check_items(SHORT, replay, batches["short_ref"], "replayed")


def test_bucket_edges_and_a_batch_of_one(dev, model):
    """a batch whose longest item has exactly 320 rows keeps the 320 plan, 321 rows build the 384 one"""
    model._plans.clear()
    run = lambda items, z: model.inference_ragged(items, noises=z, bucket=models.RAGGED_BUCKET)
    cases = [([(200, 96), (10, 20)], 320), ([(224, 96), (10, 20)], 320), ([(225, 96), (10, 20)], 384)]
    done = []
    for i, (shapes, cap) in enumerate(cases):
        ds, items, noises = _items(shapes, 700 + 10 * i, dev)
        done.append((shapes, ds, run(items, noises)))
        plans = _bucket_plans(model)
        assert list(plans)[-1][:3] == ("ragged-bucket", 2, cap)
        if i == 0:
            first = plans[list(plans)[-1]]
        assert len(plans) == (1 if cap == 320 else 2) and first in plans.values()
    # (the B = 1 plans come last: they share the model's LRU with the plans counted above)
    for shapes, ds, outs in done:
        _check_items(shapes, outs, _singles(model, ds, dev), f"longest {sum(shapes[0])}")
    model._plans.clear()
    ds, items, noises = _items([(131, 160)], 800, dev)
    outs = model.inference_ragged(items, noises=noises, bucket=models.RAGGED_BUCKET)
    assert next(iter(_bucket_plans(model)))[:3] == ("ragged-bucket", 1, 320)
    _check_items([(131, 160)], outs, _singles(model, ds, dev), "a batch of one")
    # the same draw as the B = 1 call when no noise is given
    torch.manual_seed(3)
    a = model.inference_ragged(items, bucket=models.RAGGED_BUCKET)
    torch.manual_seed(3)
    d = ds[0]
    g = lambda k: d[k].to(dev)
    b = model.inference(g("x"), d["lengths"], g("midi"), g("lft"), g("ref_x"), d["ref_lengths"], g("ref_logmel"),
                        g("ref_midi"), g("ref_lft"))
    assert nerr(a[0], b) < RAGGED_TOL
    with pytest.raises(ValueError):
        model.inference_ragged([], bucket=models.RAGGED_BUCKET)
    model._plans.clear()
