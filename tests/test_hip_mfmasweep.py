"""The fused residual unit (every implementation of srn_hifigan_resunit) and srn_tn_gemm (both kernels, both tile
edges, time-sliced or not, the reduce kernel) on the MI355X: one launch per case of the sweep in tests/_mfma_cases.py,
against float64 references of the same operation.

Per case: (a) the route query answers the form the case is meant for; (b) every output within |g - r| <= tol (|r| + s)
of the reference, per element, and finite although every padding column, gap and row past len_b of the inputs holds NaN
(the tolerance table and how it is derived: the docstring of tests/_mfma_cases.py); (c) every sentinel intact -- 64 values
on either side of out, colsum and the workspace, ld padding columns, the gaps between items; (d) the columns of a shift
that meets no row of b exactly zero; (e) a second call on fresh clones is bit-identical (the time slices are added in
slice order); (f) a case that takes the lean form (resunit_f32.hip, tn_lean_kernel) runs once more on the other form
(SRN_RESUNIT_ROUTE_SHARED, SRN_TN_ROUTE_GENERAL) and must agree bit for bit.
A call the validation rejects must return its error and write nothing.  Every case is a shape the contract accepts or
one the validation refuses before a launch."""
import ctypes

import pytest
import torch

from serenade_amd import _lib
from tests import _mfma_cases as C

pytestmark = pytest.mark.gpu

RU = [(f, cid) for fam, f, cid in C.all_ids() if fam == "resunit"]
TN = C.tn_ids()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    C.library()
    return torch.device("cuda:0")


def _launch(op):
    try:
        op()
    finally:
        torch.cuda.synchronize()


def run_resunit(case, dev, route=None, want=None):
    args, bufs = C.materialize(case, dev)
    op = C.ru_op(args)
    if route is not None:
        op.p.route = route
    if want is not None:
        assert C.ru_form_key(op.p) == want, C.ru_form_key(op.p)
        assert bool(op.p.w1_hi) == (op.p.precision == C.X3)  # the planes ResUnitOp built on the device, not a stand-in
    _launch(op)
    return {k: v.cpu() for k, v in bufs.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(C._bits(a[k]), C._bits(b[k])) for k in a)


@pytest.mark.parametrize("form,cid", RU, ids=[f"{f}-{c}" for f, c in RU])
def test_resunit_against_fp64(dev, form, cid):
    case = C.make("resunit", form, cid)
    tol = C.tol_for("resunit", form, cid)
    first = run_resunit(case, dev, want=C.RU_FORMS[form][:3])
    err, _ = C.check_outputs(case, first)  # (c) inside
    print(f"MFMASWEEP resunit {form} {cid}: worst per-element error {err:.3e}, tol {tol:.1e}, ratio {err / tol:.3f}")
    assert err <= tol
    assert _same(run_resunit(case, dev), first), "a second call on fresh clones differs"
    if C.RU_FORMS[form][0] == _lib.RESUNIT_FORM_F32:
        shared = run_resunit(case, dev, route=_lib.RESUNIT_ROUTE_SHARED,
                             want=(_lib.RESUNIT_FORM_SHARED_F32, C.RU_FORMS[form][1], "route"))
        assert _same(shared, first), "resunit_f32.hip and resunit.hip's fp32 form differ"


@pytest.mark.parametrize("form", list(C.RU_FORMS))
@pytest.mark.parametrize("epi", ["res2", "inplace"])
def test_resunit_post_div_one_means_none(dev, form, epi):
    """post_div 0 and 1.0 both mean "no division": the same bits from the same inputs"""
    a = run_resunit(C.make("resunit", form, f"{epi}-pd0"), dev)
    b = run_resunit(C.make("resunit", form, f"{epi}-pd1"), dev)
    assert [torch.equal(C._bits(x), C._bits(y)) for x, y in zip(a.values(), b.values())] == [True] * len(a)


def run_tn(case, dev, route=None, want=None):
    args, bufs = C.materialize(case, dev)
    op = C.tn_op(args, route=route)
    got = C.tn_route(op.p)
    if want is not None:
        assert C.tn_form_name(got[0], got[2], got[1] > 1) == want, got
    _launch(op)
    return {k: v.cpu() for k, v in bufs.items()}, got


@pytest.mark.parametrize("cid", TN)
def test_tn_gemm_against_fp64(dev, cid):
    form = C.tn_form(cid)
    case = C.tn_make(cid)
    tol = C.tol_for("tn", form, cid)
    first, (tb, ks, lean) = run_tn(case, dev, want=form)
    err, _ = C.check_outputs(case, first)  # (c), (d) inside
    print(f"MFMASWEEP tn {form} {cid}: worst per-element error {err:.3e}, tol {tol:.1e}, ratio {err / tol:.3f}")
    assert err <= tol
    assert _same(run_tn(case, dev)[0], first), "a second call on fresh clones differs"
    if lean:
        general, got = run_tn(case, dev, route=_lib.TN_ROUTE_GENERAL)
        assert got == (tb, ks, False)
        # the workspace holds the slices' raw partial tiles: the same bits there too
        assert _same(general, first), "tn_lean_kernel and tn_gemm_kernel differ"


@pytest.mark.parametrize("rid", [r[0] for r in C.ru_rejects()])
def test_rejected_resunit_returns_an_error_and_writes_nothing(dev, rid):
    case, edit = C.ru_reject_case(rid)
    args, bufs = C.materialize(case, dev)
    op = C.ru_op(args)
    if edit is not None:
        edit(op.p)
    with pytest.raises(RuntimeError, match=case.error):
        _launch(op)
    assert C.check_outputs(case, {k: v.cpu() for k, v in bufs.items()}) == (0.0, 0.0)


@pytest.mark.parametrize("rid", [r[0] for r in C.tn_rejects()])
def test_rejected_tn_gemm_returns_an_error_and_writes_nothing(dev, rid):
    case, edit = C.tn_reject_case(rid)
    args, bufs = C.materialize(case, dev)
    op = C.tn_op(args)
    if edit is not None:
        edit(op.p)
    with pytest.raises(RuntimeError, match=case.error):
        _launch(op)
    assert C.check_outputs(case, {k: v.cpu() for k, v in bufs.items()}) == (0.0, 0.0)
