"""CPU half of the srn_conv_gemm sweep (tests/_conv_cases.py): every case through the executable spec of the ABI
(tests/_emulator.emul_conv, fp32 torch) under the same check_outputs as the HIP kernels get in test_hip_convsweep.py --
references, masks and guards are proven without a GPU, and the restatement has to stay within tol / 4, so the
tolerance table cannot rot; every case's params, built as on a GPU (weight planes and split-K workspace attached), are
routed on the cross-compiled library and must reach the kernel form the case is meant for; and the forms reached are
the forms that exist."""
import ctypes
import json

import pytest
import torch

from serenade_amd import _lib, ops
from tests import _conv_cases as C
from tests.test_conv_route import FAMILY, FORMS_TABLE, device_params, lib  # noqa: F401  (lib is a fixture)

FORMS = list(C.forms())


def _op(case, edit=None):
    args, bufs = C.materialize(case)
    op = ops.ConvOp(**C.kwargs(args))
    if edit is not None:
        edit(op.p)
    return op, args, bufs


@pytest.mark.parametrize("form", FORMS)
def test_emulator_within_a_quarter_of_tol(form):
    f = C.forms()[form]
    ids = [vid for fn, vid in C.all_ids() if fn == form]
    assert ids
    for vid in ids:
        case = C.make(form, vid)
        args, bufs = C.materialize(case)
        C.run_emulated(case, args)
        err, _ = C.check_outputs(case, bufs)
        assert err <= C.TOL["fp32"][1] / 4, (form, vid, err)
        if f.prec == C.X3:  # the mode's own restatement: split operands, three products
            args, bufs = C.materialize(case)
            C.run_bf16x3(case, args)
            err, _ = C.check_outputs(case, bufs)
            assert err <= C.TOL["bf16x3"][1] / 4, (form, vid, err)


@pytest.fixture(scope="module")
def routed(lib):  # noqa: F811
    """{(form, case id): what the library's route answers for the case's params, as Form.key spells a form}"""
    out = (ctypes.c_int32 * 3)()
    got = {}
    for form, vid in C.all_ids():
        op, args, bufs = _op(C.make(form, vid))
        p = device_params(op)
        _lib.check(lib.srn_conv_gemm_route(ctypes.byref(p), out), "srn_conv_gemm_route")
        planes = bool(p.w_hi) and (p.precision != C.X6 or bool(p.w_lo))
        got[(form, vid)] = (FAMILY[out[0]], out[1], p.precision, planes, bool(p.w_nmajor), out[2] > 1), p.w_bs
    return got


@pytest.mark.parametrize("form", FORMS)
def test_every_case_reaches_its_form(routed, form):
    f = C.forms()[form]
    ids = [v for fn, v in C.all_ids() if fn == form]
    assert ids
    for vid in ids:
        key, w_bs = routed[(form, vid)]
        assert key == f.key, (form, vid, key)
        if not f.planes and f.family == "fast" and f.prec != C.FP32:
            assert w_bs != 0, (form, vid)  # operands split in the loop


def test_the_sweep_reaches_every_form_that_exists(routed):
    """what the route answered over the whole sweep, against the forms the library lists (srn_conv_gemm_forms)"""
    reached = {key for key, _ in routed.values()}
    assert reached == C.existing_forms(), reached ^ C.existing_forms()


def test_the_sweep_has_its_60_forms():
    """the forms the sweep makes of the library's list, by name and in order, against the committed snapshot"""
    want = json.load(open(FORMS_TABLE))["sweep"]
    assert len(FORMS) == 60 and FORMS == want, set(FORMS) ^ set(want)


def test_tolerance_table_follows_its_rule():
    for prec, (base, tol) in C.TOL.items():
        assert tol == C._round_up(max(4 * base, C.FLOOR)), prec
    assert C.TOL["bf16x6"] == C.TOL["fp32"]


@pytest.mark.parametrize("rid", [r[0] for r in C.rejects()])
def test_rejected_shape_is_refused_by_the_route(lib, rid):  # noqa: F811
    case, edit = C.reject_case(rid)
    op, args, bufs = _op(case, edit)
    rc = lib.srn_conv_gemm_route(ctypes.byref(op.p), (ctypes.c_int32 * 3)())
    assert rc == -1, rid
    assert case.error.encode() in lib.srn_last_error(), lib.srn_last_error()


def test_mirror_mode_2_reads_zero_past_one_reflection():
    """reflect = 2, len_in = 2, taps -3 .. 3: the mirror image of row t + 3 for t = 0 is 2 (len_in - 1) - 3 < 0 -> zero,
    in the reference and in the emulator alike (one mirror per end; the header bounds the taps by T_in only)"""
    kw = dict(n_batch=1, T_in=8, T_out=8, C_in=4, N=4, taps=C.TAPS["k7"], in0=torch.ones(8, 4), in0_bs=32, ld_in0=4,
              w=torch.ones(4, 28), ldw=28, out=torch.zeros(8, 4), out_bs=32, ld_out=4, reflect=2,
              len_in=torch.tensor([2], dtype=torch.int32))
    val = next(C.contract(kw))[3]
    # row 0: taps -3 .. 3 -> rows 3, 2, 1, 0, 1, 2, 3 -> mirrored at 1: -1, 0, 1, 0, 1, 0, -1: five live rows x 4 channels
    assert float(val[0, 0]) == 20.0
    from tests import _emulator
    _emulator.emul_conv(kw)
    assert torch.equal(kw["out"].double(), val)
