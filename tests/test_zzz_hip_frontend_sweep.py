"""The feature front-end's own kernels (serenade_amd/csrc/features.hip) and the GST inference tail (gst.hip) on the
MI355X, one C-ABI call per case of the sweep in tests/_frontend_cases.py, against float64 references of the same
operation.

Per case: (a) every output within its bound (the criteria and the table: the docstring of tests/_frontend_cases.py);
(b) every sentinel intact -- 64 values on either side of each written buffer; (c) rows and tails the contract zeroes
are exactly zero; (d) a second call on fresh clones is bit-identical (the atomicMax of srn_loudness runs on
non-negative floats as integers, which is order-free, so loudness repeats too).  The ragged entries give each item what
the dense entry gives it on its own rows, bit for bit, and srn_gru_recur_last is the last state of srn_gru_train_fwd,
bit for bit.  A refused call returns its error, names the entry in srn_last_error and writes nothing.

tests/test_frontend_cases_host.py shows on the CPU that fp32 statements of the entries meet a quarter of each bound and
that each case reaches the branch it is named for, so that the bounds here judge the kernels.

The file's name sorts it behind the test files that were there before it."""
import pytest
import torch

from serenade_amd import _lib, ops
from tests import _frontend_cases as C
from tests import _rowop_cases as R

pytestmark = pytest.mark.gpu

CASES = C.all_ids(error=False)
REJECTS = C.all_ids(error=True)
_id = lambda pairs: [f"{op}-{cid}" for op, cid in pairs]  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def run_hip(op, args):
    ops.CallOp(op, args)()
    torch.cuda.synchronize()


def _on(dev, args):
    return [a.to(dev) if isinstance(a, torch.Tensor) else a for a in args]


@pytest.mark.parametrize("op,cid", CASES, ids=_id(CASES))
def test_kernel_against_fp64(dev, op, cid):
    case = C.make(op, cid)
    tol = C.tol_for(op)
    args, bufs = C.materialize(case, dev)
    run_hip(op, args)
    first = {k: v.cpu() for k, v in bufs.items()}
    err = C.check_outputs(case, first)[0]  # (b), (c) inside
    print(f"{op} {cid}: worst per-element error {err:.3e}, tol {tol:.1e}")
    assert err <= tol
    again, bufs2 = C.materialize(case, dev)
    run_hip(op, again)
    for k, v in bufs2.items():
        assert torch.equal(R._bits(v.cpu()), R._bits(first[k])), "a second call on fresh clones differs"
    if op == "srn_gru_recur_last":  # the training twin's last state, bit for bit
        m = case.meta
        hs = torch.zeros(m["B"], m["T"] + 1, m["H"], device=dev)
        gates = torch.zeros(m["B"], m["T"], 4 * m["H"], device=dev)
        run_hip("srn_gru_train_fwd", [args[0], args[1], args[2], hs, gates, m["B"], m["T"], m["H"]])
        assert torch.equal(R._bits(args[3].view(m["B"], m["H"])), R._bits(hs[:, m["T"]]))
    twin = {"srn_logmel_ragged": ("srn_logmel", C.logmel_dense_twin, 3),
            "srn_loudness_ragged": ("srn_loudness", C.loudness_dense_twin, 4)}.get(op)
    if twin is not None:  # each item: the dense call on its own rows, bit for bit
        dense, build, out_at = twin
        got = args[out_at].view(case.outs[-1].ref.shape).cpu()
        for b, L in enumerate(case.meta["live"]):
            if L:
                d_args, d_out = build(case, b)
                d_args = _on(dev, d_args)
                run_hip(dense, d_args)
                want = d_args[d_out].cpu()
                assert torch.equal(R._bits(got[b, :L].contiguous()), R._bits(want.view(got[b, :L].shape))), (b, L)


@pytest.mark.parametrize("op,cid", REJECTS, ids=_id(REJECTS))
def test_refused_call_returns_an_error_and_writes_nothing(dev, op, cid):
    case = C.make(op, cid)
    args, bufs = C.materialize(case, dev)
    h = _lib.lib()
    assert h.srn_pad_ragged(None, 8, None, None, 2, 8, 2, 16, None) != 0 and b"pad_ragged" in h.srn_last_error()
    with pytest.raises(RuntimeError, match=case.error) as e:
        run_hip(op, args)
    assert op[4:] + ":" in str(e.value)  # srn_last_error names the entry
    torch.cuda.synchronize()
    assert C.check_outputs(case, {k: v.cpu() for k, v in bufs.items()}) == (0.0, 0.0)
