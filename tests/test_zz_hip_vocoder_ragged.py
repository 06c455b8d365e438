"""GPU tests of the ragged vocoder: lengths as data from the two kernels up to HiFiGANGenerator / Vocoder.

* srn_hifigan_resunit_ragged: every item of a ragged batch is BIT FOR BIT the dense entry point's n_batch = 1 call on
  that item alone, in every form (resunit_f32.hip, the shared fp32 form, bf16x3); rows past an item's end are neither
  read (they hold NaN) nor written (they hold a sentinel NaN pattern, as do guard bands around the output);
* srn_out_conv_tanh_ragged: the same scheme for both kernels of the output stage, with an exactly zero tail;
* the generator and the Vocoder: across contraction launches agreement is to fp32 summation order (srn_conv_gemm may
  pick another tile or K split for T_cap than for T_b), so items are held to the bound the existing parity tests use for
  the generator against its golden vectors (KTOL.model of tests/test_hip_parity.py: 1e-4 of the tensor's maximum, 1e-3
  in bf16x3), the golden vectors themselves included; stale rows of a reused plan and the bucket edges likewise.

The file's name sorts it behind every other test file: these cases run after the suite that was there before them.
"""
import ctypes

import numpy as np
import pytest
import torch

import serenade_amd
from serenade_amd import _lib, _shapes, ops, vocoder
from serenade_amd.utils.synth import fill_state_dict
from tests._weights import hifigan_weights
from tests.test_hip_parity import MEL_RTOL

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # a quiet NaN with a payload: "never written", and poison if it were read as data
GUARD = 256            # floats of guard band on either side of an output
BMI = {32: 256, 64: 128}  # srn_resunit_bmi: intermediate rows per tile (checked against the route below)
LENS = (3, 17, 32, 9)  # mel frames of the generator tests


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def rnd(*s, seed=0, scale=1.0):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal(s)).astype(np.float32))


def bits(t):
    return t.contiguous().view(torch.int32)


def sentinel(n, dev):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def is_sentinel(t):
    return bool((bits(t) == SENTINEL).all())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- residual unit
FORMS = {"f32": (_lib.PREC_FP32, 0, _lib.RESUNIT_FORM_F32),
         "shared": (_lib.PREC_FP32, _lib.RESUNIT_ROUTE_SHARED, _lib.RESUNIT_FORM_SHARED_F32),
         "bf16x3": (_lib.PREC_BF16X3, 0, _lib.RESUNIT_FORM_BF16X3)}


@pytest.mark.parametrize("inplace", [False, True], ids=["plain", "res2_is_out_div3"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k,d", [(3, 1), (3, 5), (7, 5), (11, 5)])
@pytest.mark.parametrize("C", [32, 64])
def test_resunit_ragged_is_the_dense_b1_call_bit_for_bit(dev, C, k, d, form, inplace):
    precision, route, want_form = FORMS[form]
    slope = 0.1
    BMo = BMI[C] - (k - 1)
    T = 2 * BMo + 3
    lens = (1, (k - 1) * (d + 1) // 2, BMo - 1, BMo, BMo + 1, T)  # < halo, three sides of a tile edge, multi-tile
    B = len(lens)
    w1 = ops.pack_conv_weight(rnd(C, C, k, seed=2, scale=1.0 / np.sqrt(C * k)).to(dev))
    w2 = ops.pack_conv_weight(rnd(C, C, k, seed=3, scale=1.0 / np.sqrt(C * k)).to(dev))
    b1, b2 = rnd(C, seed=4, scale=0.1).to(dev), rnd(C, seed=5, scale=0.1).to(dev)
    x_full = rnd(B, T, C, seed=1).to(dev)
    run_sum = rnd(B, T, C, seed=6).to(dev)  # what `out` holds on entry when res2 is out (the stage's running sum)
    x = x_full.clone()
    for b, L in enumerate(lens):
        x[b, L:] = float("nan")
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    common = dict(w1=w1, b1=b1, w2=w2, b2=b2, C=C, k=k, dilation=d, slope=slope, precision=precision, route=route,
                  post_div=3.0 if inplace else 0.0)

    def out_buffer(n_batch, t, valid):
        """sentinel everywhere (guard bands included); the running sum in the valid rows when res2 is out"""
        buf = sentinel(2 * GUARD + n_batch * t * C, dev)
        o = buf[GUARD:GUARD + n_batch * t * C].view(n_batch, t, C)
        if inplace:
            for b, (src, L) in enumerate(valid):
                o[b, :L] = src[:L]
        return buf, o

    def ragged(lens_t, xin):
        buf, o = out_buffer(B, T, [(run_sum[b], L) for b, L in enumerate(lens_t.tolist())])
        op = ops.ResUnitOp(x=xin, out=(buf, GUARD), res2=(buf, GUARD) if inplace else None, n_batch=B, T=T,
                           lens=lens_t, **common)
        op()
        torch.cuda.synchronize()
        return buf, o, op

    buf, out, op = ragged(lens_dev, x)
    # the form under test, through the ragged route query, which answers what the dense one answers
    got, dense_route = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
    assert _lib.lib().srn_hifigan_resunit_ragged_route(ctypes.byref(op.p), None, got) == 0
    assert _lib.lib().srn_hifigan_resunit_route(ctypes.byref(op.p), dense_route) == 0
    assert list(got) == list(dense_route) and got[0] == want_form and got[1] == 3  # T = 2 BMo + 3: three tiles an item

    for b, L in enumerate(lens):
        xb = x_full[b, :L].contiguous()  # a compact copy: nothing behind the item
        rbuf, ref = out_buffer(1, L, [(run_sum[b], L)])
        ops.ResUnitOp(x=xb, out=(rbuf, GUARD), res2=(rbuf, GUARD) if inplace else None, n_batch=1, T=L, **common)()
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(bits(out[b, :L]), bits(ref[0])), f"item {b} (L = {L}) differs from its dense B = 1 call"
        assert is_sentinel(out[b, L:]), f"item {b}: rows past its end were written"
    assert is_sentinel(buf[:GUARD]) and is_sentinel(buf[-GUARD:])

    buf2, out2, _ = ragged(lens_dev.clone(), x.clone())  # run to run
    assert torch.equal(bits(buf2), bits(buf))

    # every length = T: the dense batched call
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    fbuf, fout, _ = ragged(full, x_full)
    dbuf, dout = out_buffer(B, T, [(run_sum[b], T) for b in range(B)])
    ops.ResUnitOp(x=x_full, out=(dbuf, GUARD), res2=(dbuf, GUARD) if inplace else None, n_batch=B, T=T, **common)()
    torch.cuda.synchronize()
    assert torch.equal(bits(fbuf), bits(dbuf))

    # validation: no lengths / no params -> the error, nothing launched, nothing written
    vbuf, vout = out_buffer(B, T, [])
    before = vbuf.clone()
    vop = ops.ResUnitOp(x=x, out=(vbuf, GUARD), n_batch=B, T=T, lens=lens_dev, **dict(common, post_div=0.0))
    fn = _lib.lib().srn_hifigan_resunit_ragged
    assert fn(ctypes.byref(vop.p), None, stream()) == -1 and b"null lens" in _lib.lib().srn_last_error()
    assert fn(None, ctypes.c_void_p(lens_dev.data_ptr()), stream()) == -1
    assert b"null params" in _lib.lib().srn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(vbuf), bits(before))


def test_resunit_tile_height_is_the_librarys(dev):
    """BMI above is srn_resunit_bmi: T = BMo fills one tile, BMo + 1 needs two"""
    for C in (32, 64):
        for k in (3, 11):
            x, o = torch.zeros(1, 600, C, device=dev), torch.zeros(1, 600, C, device=dev)
            w, b = torch.zeros(C, k * C, device=dev), torch.zeros(C, device=dev)
            for T, tiles in ((BMI[C] - (k - 1), 1), (BMI[C] - (k - 1) + 1, 2)):
                op = ops.ResUnitOp(x=x, w1=w, b1=b, w2=w, b2=b, out=o, n_batch=1, T=T, C=C, k=k, dilation=1, slope=0.1,
                                   precision=_lib.PREC_FP32)
                r = (ctypes.c_int32 * 3)()
                assert _lib.lib().srn_hifigan_resunit_route(ctypes.byref(op.p), r) == 0 and r[1] == tiles


# ---------------------------------------------------------------------------------------------------- output stage
@pytest.mark.parametrize("C,k", [(32, 7), (8, 3)], ids=["specialised_7x32", "generic_3x8"])
def test_out_conv_tanh_ragged_is_the_dense_b1_call_bit_for_bit(dev, C, k):
    lens = (1, 3, 255, 256, 257, 515)  # the workgroup tile is 256 outputs
    B, T = len(lens), 515
    x_full = rnd(B, T, C, seed=1).to(dev)
    x = x_full.clone()
    for b, L in enumerate(lens):
        x[b, L:] = float("nan")
    w, bias = rnd(k, C, seed=2, scale=1.0 / np.sqrt(C * k)).to(dev), rnd(1, seed=3, scale=0.1).to(dev)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    buf = sentinel(2 * GUARD + B * T, dev)
    y = buf[GUARD:GUARD + B * T].view(B, T)
    ops.out_conv_tanh_op(x, w, bias, (buf, GUARD), B, T, C, k, 0.01, lens=lens_dev)()
    torch.cuda.synchronize()
    for b, L in enumerate(lens):
        ref = sentinel(L, dev)
        ops.out_conv_tanh_op(x_full[b, :L].contiguous(), w, bias, ref, 1, L, C, k, 0.01)()
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(bits(y[b, :L]), bits(ref)), f"item {b} (L = {L})"
        assert bool((bits(y[b, L:]) == 0).all()), f"item {b}: the tail must be exactly zero"
    assert is_sentinel(buf[:GUARD]) and is_sentinel(buf[-GUARD:])
    fn = _lib.lib().srn_out_conv_tanh_ragged
    before = buf.clone()
    assert fn(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), None, B, T, C, k, 0.01, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(before))


# ---------------------------------------------------------------------------------------------------- generator / Vocoder
@pytest.fixture(params=["fp32", "bf16x3", "bf16x6"])
def model_tol(request):
    """the arithmetic modes of the existing vocoder parity tests, with their bound for the generator (KTOL.model)"""
    serenade_amd.set_precision(request.param)
    yield MEL_RTOL if request.param == "bf16x3" else 1e-4
    serenade_amd.set_precision("fp32")


def nerr(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def make_gen(dev, small):
    w, params = hifigan_weights(seed=1 if small else 0, small=small)
    gen = vocoder.HiFiGANGenerator(**dict(params, use_weight_norm=False))
    gen.load_state_dict(w)
    return gen.eval().to(dev)


def mels_of(lens, dev, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal((n, 80)).astype(np.float32)).to(dev) for n in lens]


def nan_padded(mels, T=None):
    T = max(m.shape[0] for m in mels) if T is None else T
    c = torch.full((len(mels), T, 80), float("nan"), device=mels[0].device)
    for b, m in enumerate(mels):
        c[b, :m.shape[0]] = m
    return c


def check_items(gen, mels, outs, tol, what):
    for m, o in zip(mels, outs):
        one = gen.inference_batch(m.unsqueeze(0)).view(-1)
        assert o.shape == one.shape and torch.isfinite(o).all(), what
        assert nerr(o, one) < tol, f"{what}: item of {m.shape[0]} frames vs its own B = 1 call"


@pytest.mark.parametrize("small", [True, False], ids=["small", "full"])
def test_generator_ragged_equals_b1_runs(dev, model_tol, small):
    gen = make_gen(dev, small)
    mels = mels_of(LENS, dev, seed=11)
    outs = gen.inference_ragged(mels)
    c = nan_padded(mels)
    yb = gen.inference_batch(c, lengths=LENS)
    check_items(gen, mels, outs, model_tol, "inference_ragged")
    assert yb.shape == (len(LENS), 1, max(LENS) * gen.hop)
    for n, o, y in zip(LENS, outs, yb):
        assert torch.equal(y[0, :n * gen.hop], o) and bool((bits(y[0, n * gen.hop:]) == 0).all())


def test_vocoder_decode_ragged_equals_decode(dev, model_tol):
    gen = make_gen(dev, small=False)
    rng = np.random.default_rng(3)
    one = np.ones(80, dtype=np.float32)
    stats = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one + 0.1}
    trg = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one * 0.9}
    voc = vocoder.Vocoder.from_generator(gen, {"sampling_rate": 24000}, stats, dev, trg_stats=trg)
    mels = mels_of(LENS, dev, seed=12)
    waves = voc.decode_ragged(mels)
    wb = voc.decode_batch(nan_padded(mels), lengths=LENS)
    hop = voc.model.hop
    for n, m, o, y in zip(LENS, mels, waves, wb):
        assert nerr(o, voc.decode(m)[0]) < model_tol
        assert torch.equal(y[:n * hop], o) and bool((bits(y[n * hop:]) == 0).all())


@pytest.mark.parametrize("name,small", [("hifigan", False), ("hifigan_small", True)])
def test_golden_items_in_a_ragged_batch_meet_the_golden_bound(dev, model_tol, golden, name, small):
    """the golden batch's items between a shorter and a longer dummy item: same vectors, same bound as the dense tests"""
    g = golden(name)
    if small:
        gen = make_gen(dev, True)
    else:  # the weight-normed parameters the golden was made from (tests/test_hip_parity.py, `voc`)
        w, params = hifigan_weights()
        gen = vocoder.HiFiGANGenerator(**params)
        gen.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**params, weight_norm=True)), seed=0))
        gen = gen.eval().to(dev)
    c = torch.from_numpy(np.asarray(g["c"])).to(dev)  # (B, 80, T)
    Tg = c.shape[2]
    items = mels_of((Tg - 5,), dev, seed=1) + [c[b].t().contiguous() for b in range(c.shape[0])] \
        + mels_of((Tg + 9,), dev, seed=2)
    outs = gen.inference_ragged(items)
    y = torch.stack(outs[1:-1]).unsqueeze(1)
    assert nerr(y, g["y"]) < model_tol


def test_short_batch_after_a_long_one_reuses_the_plan_and_ignores_stale_rows(dev, model_tol):
    """the case a missing mask hides: rows past an item's end hold the PREVIOUS batch's data, not zeros.  Same bucket,
    so the same plan object -- and, with graphs on, the same captured graph replayed over new lengths"""
    gen = make_gen(dev, small=False)
    long_, short = mels_of((60, 50, 64, 33), dev, seed=21), mels_of(LENS, dev, seed=22)
    gen.inference_ragged(long_)
    pl = gen.plan_ragged(len(LENS), 64)
    outs = gen.inference_ragged(short)
    assert gen.plan_ragged(len(LENS), max(LENS)) is pl and pl.T == 64
    check_items(gen, short, outs, model_tol, "eager")
    ops.set_graphs(True)
    try:
        gen._plans.clear()
        gen.inference_ragged(long_)            # eager warm-up of a new plan
        first = gen.inference_ragged(long_)    # captured
        pl = gen.plan_ragged(len(LENS), 64)
        replay = gen.inference_ragged(short)   # replayed over new lengths and the long batch's leftovers
        assert gen.plan_ragged(len(LENS), max(LENS)) is pl
    finally:
        ops.set_graphs(False)
        gen._plans.clear()
    for a, b in zip(replay, outs):
        assert torch.equal(a, b)
    check_items(gen, long_, first, model_tol, "captured")


def test_bucket_edges_and_length_validation(dev, model_tol):
    gen = make_gen(dev, small=True)
    for top, cap in ((64, 64), (65, 128)):
        mels = mels_of((top, 7), dev, seed=top)
        outs = gen.inference_ragged(mels)
        assert gen.plan_ragged(2, top).T == cap
        check_items(gen, mels, outs, model_tol, f"batch maximum {top}")
    gen._plans.clear()
    c = nan_padded(mels_of((5, 11), dev))
    for bad in ((5,), (5, 11, 3), (0, 11), (5, 12)):
        with pytest.raises(ValueError):
            gen.inference_batch(c, lengths=bad)
    assert not gen._plans, "validation comes before any plan is built or launched"
