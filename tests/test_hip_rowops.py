"""The row / norm / training kernels of norm_act.hip, train.hip and gst_train.hip on the MI355X, one launch per case of
the sweep in tests/_rowop_cases.py, against float64 references of the same operation.

Per case: (a) every output within |g - r| <= tol_op (|r| + s) of the reference, per element (the tolerance table and
how it is derived: the docstring of tests/_rowop_cases.py); (b) every sentinel intact -- 64 values on either side of
each output buffer, every ld padding column, every row the contract does not write; (c) rows the contract zeroes are
exactly zero; (d) a second call on fresh clones is bit-identical (none of these kernels accumulates with atomics).
A shape a launcher rejects must return its error and write nothing."""
import ctypes

import pytest
import torch

from serenade_amd import _lib, ops
from tests import _rowop_cases as R

pytestmark = pytest.mark.gpu

CASES = R.all_ids(error=False)
REJECTS = R.all_ids(error=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def run_hip(case, args):
    if case.kind == "call":
        ops.CallOp(case.op, args)()
    elif case.kind == "transpose_multi":
        ops.TransposeMultiOp(args)()
    elif case.kind == "multi_copy":  # the table by hand: ops.MultiCopyOp cannot express a zero-length entry
        srcs, offs, lens, dst = args
        lst = _lib.SrnCopyList()
        lst.n = len(srcs)
        for j, (src, off, n) in enumerate(zip(srcs, offs, lens)):
            lst.src[j], lst.off[j], lst.len[j] = ops._ptr(src), off, n
        _lib.check(_lib.lib().srn_multi_copy(ctypes.byref(lst), ops._ptr(dst), ops._stream()), "srn_multi_copy")
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,cid", CASES, ids=[f"{op}-{cid}" for op, cid in CASES])
def test_kernel_against_fp64(dev, op, cid):
    case = R.make(op, cid)
    tol = R.tol_for(op, cid)
    args, bufs = R.materialize(case, dev)
    run_hip(case, args)
    first = {k: v.cpu() for k, v in bufs.items()}
    del args, bufs
    err = R.check_outputs(case, first)  # (b), (c) inside
    print(f"{op} {cid}: worst per-element error {err}, tol {tol}")
    assert R.within(err, tol)
    args, bufs = R.materialize(case, dev)
    run_hip(case, args)
    for k, v in bufs.items():
        assert torch.equal(R._bits(v.cpu()), R._bits(first[k])), "a second call on fresh clones differs"


@pytest.mark.parametrize("op,cid", REJECTS, ids=[f"{op}-{cid}" for op, cid in REJECTS])
def test_rejected_shape_returns_an_error_and_writes_nothing(dev, op, cid):
    case = R.make(op, cid)
    args, bufs = R.materialize(case, dev)
    with pytest.raises(RuntimeError, match=case.error):
        run_hip(case, args)
    torch.cuda.synchronize()
    assert R.check_outputs(case, {k: v.cpu() for k, v in bufs.items()}) == (0.0, 0.0)


@pytest.mark.parametrize("shape", list(R.im2col_shapes()), ids=lambda s: "B{}-H{}-W{}-C{}-ld{}".format(*s))
def test_im2col_col2im_adjoint(dev, shape):
    """<im2col(x), c> == <x, col2im(c)> in fp64, at 1e-6 relative: col2im is the transpose of the gather"""
    lhs, rhs = R.adjoint_pair(shape, run_hip, dev)
    print(f"{shape}: <im2col(x), c> = {lhs!r}, <x, col2im(c)> = {rhs!r}")
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))
