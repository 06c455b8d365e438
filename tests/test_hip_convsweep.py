"""Every kernel form behind srn_conv_gemm on the MI355X, one launch per case of the sweep in tests/_conv_cases.py,
against float64 references of the same contraction.

Per case: (a) the params route to the form the case is meant for (split-K cases: more than one K slice); (b) every
output within |g - r| <= tol (|r| + s) of the reference, per element (the tolerance table and how it is derived: the
docstring of tests/_conv_cases.py); (c) every sentinel intact -- 64 values on either side of out, out_tr and
gn_partials, every ld padding column, the rows between strided output rows, out_tr columns at or past T_out, the columns
of `out` at or past out_tr_col0; (d) rows at or past len_out exactly zero where nothing is added to them; (e) a second
call on fresh clones is bit-identical (split-K included: the slices are added in slice order).
A shape the validation rejects must return its error and write nothing."""
import ctypes

import pytest
import torch

from serenade_amd import _lib, ops
from tests import _conv_cases as C
from tests.test_conv_route import FAMILY

pytestmark = pytest.mark.gpu

CASES = C.all_ids()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def run_hip(case, dev, edit=None, form=None):
    args, bufs = C.materialize(case, dev)
    op = ops.ConvOp(**C.kwargs(args))
    if edit is not None:
        edit(op.p)
    if form is not None:
        out = (ctypes.c_int32 * 3)()
        _lib.check(_lib.lib().srn_conv_gemm_route(ctypes.byref(op.p), out), "srn_conv_gemm_route")
        assert (FAMILY[out[0]], out[1], out[2] > 1) == (form.family, form.tile, form.splitk), (out[0], out[1], out[2])
        # the planes ConvOp built on the device, not a stand-in: without them the in-loop form would run and pass
        assert bool(op.p.w_hi) == form.planes and bool(op.p.w_lo) == (form.planes and form.prec == C.X6)
    try:
        op()
    finally:
        torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("form,vid", CASES, ids=[f"{f}-{v}" for f, v in CASES])
def test_kernel_against_fp64(dev, form, vid):
    case = C.make(form, vid)
    tol = C.tol_for(form, vid)
    bufs = run_hip(case, dev, form=C.forms()[form])
    first = {k: v.cpu() for k, v in bufs.items()}
    del bufs
    err, _ = C.check_outputs(case, first)  # (c), (d) inside
    print(f"CONVSWEEP {form} {vid}: worst per-element error {err:.3e}, tol {tol:.1e}, ratio {err / tol:.3f}")
    assert err <= tol
    bufs = run_hip(case, dev)
    for k, v in bufs.items():
        assert torch.equal(C._bits(v.cpu()), C._bits(first[k])), "a second call on fresh clones differs"


@pytest.mark.parametrize("rid", [r[0] for r in C.rejects()])
def test_rejected_shape_returns_an_error_and_writes_nothing(dev, rid):
    case, edit = C.reject_case(rid)
    args, bufs = C.materialize(case, dev)
    op = ops.ConvOp(**C.kwargs(args))
    if edit is not None:
        edit(op.p)
    with pytest.raises(RuntimeError, match=case.error):
        op()
    torch.cuda.synchronize()
    assert C.check_outputs(case, {k: v.cpu() for k, v in bufs.items()}) == (0.0, 0.0)
