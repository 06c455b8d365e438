"""GPU tests of the causal vocoder: the two new kernels against a float64 statement of their contract, then the causal
generator one-shot, streamed and streamed under hipGraph replay.

* srn_hifigan_resunit_causal, both exact-fp32 forms: per element against tests/_vocoder_causal_emul.causal_unit in
  float64 (the header's contract: the unit on the utterance that begins v_b = clamp(lead[b], 0, H) rows before the
  call), under the bound the sweep of the dense unit applies -- |got - ref| <= tol (|ref| + s), tol imported from
  tests/_mfma_cases.py, s the size of the terms summed.  Input rows before H - v_b hold NaN, the output sits between
  guard bands of a NaN sentinel, and a second call on the same inputs must give the same bits.
* srn_out_conv_tanh_causal, both kernels: the same scheme.  Its bound is the forward error of the kernel's arithmetic:
  one fp32 fmaf chain of n = k C terms on top of the bias carries at most n u s (u = 2^-24, s = |bias| + sum |w| |x|;
  Higham, Accuracy and Stability, eq. 3.5 with gamma_n ~ n u), tanh has slope <= 1 and tanhf is held to 4 u more.
* the model (small configuration and the full HIFIGAN_PARAMS at T = 5): one-shot against the reference's output at the
  waveform gate of 1e-4, the stream against the one-shot result at the same gate (bit equality between chunkings is not
  required: srn_conv_gemm may tile (B, chunk) differently from (B, T); the measured maxima are printed), and with
  graphs on -- chunk 1 eager, chunk 2 captured, later chunks replayed -- torch.equal to the eager stream.

The file's name sorts it behind the suite that was there before it.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from serenade_amd import _lib, ops, vocoder
from serenade_amd.utils.synth import HIFIGAN_PARAMS, fill_state_dict
from tests import _vocoder_causal_emul as E
from tests._mfma_cases import TOL
from tests._weights import hifigan_weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-4            # the project's waveform gate (README)
SENTINEL = 0x7FC12345  # a quiet NaN with a payload: "never written"
GUARD = 256            # floats of guard band on either side of an output
U = 2.0 ** -24
UNIT_TOL = TOL["resunit-fp32"][1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def rnd(*s, seed=0, scale=1.0):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal(s)).astype(np.float32))


def bits(t):
    return t.contiguous().view(torch.int32)


def sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32)


def is_sentinel(t):
    return bool((bits(t) == SENTINEL).all())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- residual unit
FORMS = {"f32": (0, _lib.RESUNIT_FORM_F32), "shared": (_lib.RESUNIT_ROUTE_SHARED, _lib.RESUNIT_FORM_SHARED_F32)}


def unit_route(p):
    r = (ctypes.c_int32 * 3)()
    _lib.check(_lib.lib().srn_hifigan_resunit_causal_route(ctypes.byref(p), None, r), "srn_hifigan_resunit_causal_route")
    return list(r)


def unit_kw(C, k, d, T, lead, route, epi, seed):
    """host tensors of one call: x (3, H + T, C) with NaN before each item's first row, out between guard bands"""
    H, B = (k - 1) * (d + 1), len(lead)
    x = rnd(B, H + T, C, seed=seed)
    for b, v in enumerate(lead):
        x[b, :H - max(0, min(v, H))] = float("nan")
    w1 = ops.pack_conv_weight(rnd(C, C, k, seed=seed + 1, scale=1.0 / np.sqrt(C * k)))
    w2 = ops.pack_conv_weight(rnd(C, C, k, seed=seed + 2, scale=1.0 / np.sqrt(C * k)))
    b1 = 1.5 + 0.5 * rnd(C, seed=seed + 3)  # order 1 with a mean: an intermediate not zeroed before row 0 shows
    b2 = rnd(C, seed=seed + 4)
    buf = sentinel(2 * GUARD + B * T * C)
    kw = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, out=(buf, GUARD), n_batch=B, T=T, C=C, k=k, dilation=d, slope=0.1,
              precision=_lib.PREC_FP32, route=route, lead=torch.tensor(lead, dtype=torch.int32), post_div=0.0)
    if epi == "inplace-div2":  # res2 is out: the stage's running sum, then the mean
        buf[GUARD:GUARD + B * T * C] = rnd(B * T * C, seed=seed + 5)
        kw.update(res2=(buf, GUARD), post_div=2.0)
    return kw, buf


def to_dev(kw, dev):
    moved = {}

    def mv(v):
        if isinstance(v, torch.Tensor):
            if id(v) not in moved:
                moved[id(v)] = v.to(dev)
            return moved[id(v)]
        if isinstance(v, tuple) and isinstance(v[0], torch.Tensor):
            return (mv(v[0]), v[1])
        return v
    return {k: mv(v) for k, v in kw.items()}


def tile_height(dev, C, k, d, route):
    """output rows per tile of the form, from the route call: the largest T that one tile per item covers"""
    z = torch.zeros(4, device=dev)
    lead = torch.zeros(1, dtype=torch.int32, device=dev)
    tiles = lambda T: unit_route(ops.ResUnitOp(x=z, w1=z, b1=z, w2=z, b2=z, out=z[1:], n_batch=1, T=T, C=C, k=k,
                                               dilation=d, slope=0.1, precision=_lib.PREC_FP32, route=route,
                                               lead=lead).p)[1]
    T = 1
    while tiles(T + 1) == 1:
        T += 1
    assert T < 512 and tiles(2 * T) == 2 and tiles(2 * T + 1) == 3
    return T


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k,d", [(3, 1), (3, 2), (5, 6), (11, 5)])
@pytest.mark.parametrize("C", [32, 64])
def test_resunit_causal_against_fp64(dev, C, k, d, form):
    route, want_form = FORMS[form]
    H = (k - 1) * (d + 1)
    bmo = tile_height(dev, C, k, d, route)
    worst = 0.0
    leads = ((0, k - 1, H), (1, H - 1, H + 7))  # {0, 1, k - 1, H - 1, H, H + 7}, mixed inside batches of 3
    for T in sorted({1, 2, H - 1, H, H + 1, bmo - 1, bmo, bmo + 1}):
        for i, lead in enumerate(leads):
            for epi in ("plain", "inplace-div2"):
                kw, buf = unit_kw(C, k, d, T, lead, route, epi, seed=100 * T + 10 * i)
                ref = E.causal_unit(kw, torch.float64)  # from the host tensors, before anything runs
                outs = []
                for _ in range(2):
                    dkw = to_dev(kw, dev)
                    op = ops.ResUnitOp(**dkw)
                    assert unit_route(op.p)[:2] == [want_form, -(-T // bmo)]
                    op()
                    torch.cuda.synchronize()
                    outs.append(dkw["out"][0].cpu())
                got = outs[0]
                assert torch.equal(bits(outs[0]), bits(outs[1])), "a second call on the same inputs differs"
                assert is_sentinel(got[:GUARD]) and is_sentinel(got[-GUARD:]), "a guard band was written"
                o = got[GUARD:-GUARD].view(len(lead), T, C).double()
                for b, (y, s) in enumerate(ref):
                    assert torch.isfinite(o[b]).all(), f"T {T} lead {lead[b]} {epi}: a row before the utterance was read"
                    excess = ((o[b] - y).abs() / (y.abs() + s)).max().item()
                    worst = max(worst, excess)
                    assert excess <= UNIT_TOL, f"T {T} lead {lead[b]} {epi}: {excess:.3e} of (|ref| + s), tol {UNIT_TOL:.1e}"
    print(f"CAUSAL unit {form} C{C} k{k} d{d}: tile {bmo} rows, worst error {worst:.3e} of (|ref| + s), tol {UNIT_TOL:.1e}")


@pytest.mark.parametrize("C,k,d", [(32, 3, 2), (64, 11, 5)])
def test_resunit_causal_forms_agree(dev, C, k, d):
    """resunit_f32.hip's causal instance and the shared form's: the same bits, as their dense instances"""
    H = (k - 1) * (d + 1)
    outs = []
    for route in (0, _lib.RESUNIT_ROUTE_SHARED):
        kw, _ = unit_kw(C, k, d, 300, (0, H // 2, H), route, "inplace-div2", seed=3)
        dkw = to_dev(kw, dev)
        ops.ResUnitOp(**dkw)()
        torch.cuda.synchronize()
        outs.append(dkw["out"][0].cpu())
    assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_resunit_causal_validation(dev):
    kw, buf = unit_kw(32, 3, 2, 40, (0, 3, 6), 0, "plain", seed=7)
    dkw = to_dev(kw, dev)
    before = dkw["out"][0].clone()
    op = ops.ResUnitOp(**dkw)
    fn = _lib.lib().srn_hifigan_resunit_causal
    assert fn(ctypes.byref(op.p), None, stream()) == -1 and b"null lead" in _lib.lib().srn_last_error()
    assert fn(None, ctypes.c_void_p(dkw["lead"].data_ptr()), stream()) == -1
    op.p.k = 4
    assert fn(ctypes.byref(op.p), ctypes.c_void_p(dkw["lead"].data_ptr()), stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(dkw["out"][0]), bits(before)), "a refused call wrote"
    # the split-bf16 precisions run the exact-fp32 form: the same bits, no weight planes asked for
    op.p.k = 3
    op()
    x3 = ops.ResUnitOp(**dict(dkw, out=(before.clone(), GUARD), precision=_lib.PREC_BF16X3))
    assert unit_route(x3.p)[0] == _lib.RESUNIT_FORM_F32 and not x3.p.w1_hi
    x3()
    torch.cuda.synchronize()
    assert torch.equal(bits(x3.kw["out"][0]), bits(dkw["out"][0]))


# ---------------------------------------------------------------------------------------------------- output stage
@pytest.mark.parametrize("C,k", [(32, 7), (16, 3), (32, 3), (16, 7)])
def test_out_conv_tanh_causal_against_fp64(dev, C, k):
    slope, B = 0.01, 3
    worst = 0.0
    for T in (1, 2, 255, 256, 257, 300):
        x = rnd(B, k - 1 + T, C, seed=T)
        x[0, :k - 1] = 0.0  # item 0 begins here: zero history is the causal padding
        w, bias = rnd(k, C, seed=T + 1, scale=1.0 / np.sqrt(k * C)), rnd(1, seed=T + 2)
        ref, s = E.out_conv_tanh_causal(x, w, bias, B, T, C, k, slope, torch.float64)
        outs = []
        for _ in range(2):
            buf = sentinel(2 * GUARD + B * T).to(dev)
            ops.out_conv_tanh_causal_op(x.to(dev), w.to(dev), bias.to(dev), (buf, GUARD), B, T, C, k, slope)()
            torch.cuda.synchronize()
            outs.append(buf.cpu())
        assert torch.equal(bits(outs[0]), bits(outs[1])), "a second call on the same inputs differs"
        assert is_sentinel(outs[0][:GUARD]) and is_sentinel(outs[0][-GUARD:]), "a guard band was written"
        got = outs[0][GUARD:-GUARD].view(B, T).double()
        bound = k * C * U * s + 4 * U
        ratio = ((got - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"T {T}: {ratio:.3f} of the bound"
    print(f"CAUSAL out conv C{C} k{k}: worst error {worst:.3f} of the bound k C u s + 4 u")
    z = torch.zeros(8, device=dev)
    assert _lib.lib().srn_out_conv_tanh_causal(None, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, 4, 3, 0.01, stream()) == -1
    assert _lib.lib().srn_out_conv_tanh_causal(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, 4, 4, 0.01,
                                               stream()) == -1


def test_replicate_first_row(dev):
    B, n = 3, 300
    x = rnd(B, 4, n, seed=5).to(dev)
    want = x.clone()
    want[0, 0], want[2, 0] = x[0, 1], x[2, 1]
    lead = torch.tensor([0, 1, -3], dtype=torch.int32, device=dev)
    ops.replicate_first_row_op(x, 4 * n, n, lead, B)()
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(want))
    assert _lib.lib().srn_replicate_first_row(x.data_ptr(), n, n, lead.data_ptr(), B, stream()) == -1  # items overlap


# ---------------------------------------------------------------------------------------------------- the model
def _gen(dev, full):
    params = dict(HIFIGAN_PARAMS if full else hifigan_weights(small=True)[1], use_causal_conv=True)
    g = vocoder.HiFiGANGenerator(**params)
    g.load_state_dict(fill_state_dict(vocoder.hifigan_state_shapes(**params, weight_norm=True), seed=0 if full else 1))
    g.remove_weight_norm()
    return g.eval().to(dev)


@pytest.fixture(scope="module")
def models(dev):
    """(generator, golden c (B, 80, T), golden y (B, T hop), one-shot result) for the small and the full configuration:
    built and run once, shared and left unchanged"""
    out = {}
    for name, fixture in (("small", "hifigan_causal_small"), ("full", "hifigan_causal")):
        gold = dict(np.load(os.path.join(GOLDEN, fixture + ".npz")))
        g = _gen(dev, name == "full")
        c = torch.from_numpy(gold["c"]).to(dev)
        out[name] = (g, c, torch.from_numpy(gold["y"])[:, 0], g(c)[:, 0].cpu())
    return out


def err(a, b):
    return float((a.cpu() - b.cpu()).abs().max())


@pytest.mark.parametrize("name", ["small", "full"])
def test_model_one_shot_against_the_reference(models, name):
    g, c, gold, one = models[name]
    e = err(one, gold)
    print(f"CAUSAL model {name}: one-shot vs reference {e:.3e} (gate {GATE:.0e})")
    assert one.shape == gold.shape and e < GATE
    assert torch.equal(g(c)[:, 0].cpu(), one), "the one-shot plan left state behind"
    names = [op.name for op in g.plan(*c.shape[::2]).ops]
    assert names.count("srn_hifigan_resunit_causal") == (18 if name == "full" else 5)
    assert "srn_hifigan_resunit" not in names and names[-1] == "srn_out_conv_tanh_causal"


def _streamed(g, c, chunk_frames):
    cl = c.transpose(1, 2).contiguous()
    s = g.stream(cl.shape[0], chunk_frames)
    return torch.cat([s.push(cl[:, t:t + chunk_frames]) for t in range(0, cl.shape[1], chunk_frames)], dim=1).cpu()


@pytest.mark.parametrize("name,chunk_frames", [("small", 4), ("small", 1), ("small", 3), ("full", 2), ("full", 1)])
def test_model_stream_against_one_shot(models, name, chunk_frames):
    g, c, gold, one = models[name]
    got = _streamed(g, c, chunk_frames)
    print(f"CAUSAL model {name} chunks of {chunk_frames}: vs one-shot {err(got, one):.3e}, vs reference {err(got, gold):.3e}, "
          f"bit-equal to one-shot: {torch.equal(got, one)}")
    assert got.shape == one.shape and err(got, one) < GATE and err(got, gold) < GATE


def test_model_stream_carries_in_place(models, dev):
    """chunks at least as long as every history: the carry copies run in place (one launch)"""
    g = models["small"][0]
    c = rnd(2, 80, 18, seed=11).to(dev)
    pl_ops = [type(op).__name__ for op in vocoder.CausalHiFiGANPlan(g, 2, 9, carry=True).ops]
    assert pl_ops.count("MultiCopyOp") == 1
    got, one = _streamed(g, c, 9), g(c)[:, 0].cpu()
    print(f"CAUSAL model small 2 x 9 frames: vs one-shot {err(got, one):.3e}")
    assert err(got, one) < GATE


def test_model_lengths(models):
    g, c, gold, one = models["small"]
    cl = c.transpose(1, 2).contiguous()
    cl[1, 5:] = float("nan")  # behind item 1's end: anything
    y = g.inference_batch(cl, lengths=[9, 5])[:, 0].cpu()
    g5 = torch.from_numpy(dict(np.load(os.path.join(GOLDEN, "hifigan_causal_small.npz")))["y5"])[1, 0]
    assert err(y[0], gold[0]) < GATE and err(y[1, :40], g5) < GATE and bool((bits(y[1, 40:]) == 0).all())


@pytest.mark.parametrize("name,chunk_frames", [("small", 4), ("full", 2)])
def test_model_stream_under_graph_replay(models, name, chunk_frames):
    """chunk 1 runs eagerly, chunk 2 is captured, later chunks replay the capture: the eager stream's bits"""
    g, c, gold, one = models[name]
    c = torch.cat([c, c.flip(2), c], dim=2)[:, :, :4 * chunk_frames + 1]  # four chunks and a short one
    eager = _streamed(g, c, chunk_frames)
    g._plans.clear()  # a fresh stream plan, with a runner that has not run
    was = ops.GRAPHS
    ops.set_graphs(True)
    try:
        graphed = _streamed(g, c, chunk_frames)
        runner = next(v for k, v in g._plans.items() if k[0] == "stream")._runner
        assert runner._graph is not None, "the stream did not replay a captured graph"
    finally:
        ops.set_graphs(was)
        g._plans.clear()
    assert torch.equal(graphed, eager)
