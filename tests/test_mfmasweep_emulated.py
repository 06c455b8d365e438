"""CPU half of the sweep over the fused residual unit and srn_tn_gemm (tests/_mfma_cases.py): every case through the
executable spec of the ABI (tests/_emulator.emul_resunit / emul_tn_gemm) and through the restatement in the arithmetic of
its mode, under the same check_outputs as the HIP kernels get in test_hip_mfmasweep.py -- references, masks and guards
are proven without a GPU, and the restatements have to stay within tol / 4, so the tolerance table cannot rot; every
case's params are routed on the cross-compiled library (srn_hifigan_resunit_route, srn_tn_gemm_route: the code the
launches run) and must reach the form the case names; the forms reached are the forms there are.  No kernel is launched
here."""
import ctypes

import pytest
import torch

from serenade_amd import _lib
from tests import _mfma_cases as C

IDS = C.all_ids()
RU_FORMS = list(C.RU_FORMS)


@pytest.fixture(scope="module")
def lib():
    return C.library()


@pytest.mark.parametrize("form", RU_FORMS)
def test_resunit_restatements_within_a_quarter_of_tol(form):
    x3 = C.RU_FORMS[form][3] == C.X3
    ids = [cid for fam, f, cid in IDS if f == form and fam == "resunit"]
    assert ids
    for cid in ids:
        case = C.make("resunit", form, cid)
        args, bufs = C.materialize(case)
        C.ru_run_emulated(args)
        err, _ = C.check_outputs(case, bufs)
        assert err <= C.TOL["resunit-fp32"][1] / 4, (form, cid, err)
        if x3:  # the mode's own restatement: split operands, three products
            args, bufs = C.materialize(case)
            C.ru_run_bf16x3(args)
            err, _ = C.check_outputs(case, bufs)
            assert err <= C.TOL["resunit-bf16x3"][1] / 4, (form, cid, err)


@pytest.mark.parametrize("form", C.TN_FORMS)
def test_tn_restatements_within_a_quarter_of_tol(lib, form):
    ids = [cid for fam, f, cid in IDS if f == form and fam == "tn"]
    assert ids
    for cid in ids:
        case = C.make("tn", form, cid)
        for run in (C.tn_run_emulated, C.tn_run_fp32):
            args, bufs = C.materialize(case)
            run(args)
            err, _ = C.check_outputs(case, bufs)
            assert err <= C.TOL["tn"][1] / 4, (form, cid, run.__name__, err)


def test_tolerance_table_follows_its_rule():
    for row, (base, tol) in C.TOL.items():
        # (the table holds the two-digit decimal; _round_up's own result can lie one ulp beside it)
        assert tol == pytest.approx(C._round_up(max(4 * base, C.FLOOR)), rel=1e-12, abs=0), row
    assert C.TOL["resunit-bf16x6"] == C.TOL["resunit-fp32"]
    assert not C.CASE_TOL


# ------------------------------------------------------------------------------------------------------- routes
@pytest.fixture(scope="module")
def ru_routed(lib):
    """{(form, case id): ((form code, C, why), tiles per item, grid, params)} as the library answers"""
    got = {}
    for fam, form, cid in IDS:
        if fam == "resunit":
            args, _ = C.materialize(C.make(fam, form, cid))
            op = C.ru_op(args, planes=True)
            _, tpz, grid = C.ru_route(op.p)
            got[(form, cid)] = (C.ru_form_key(op.p), tpz, grid, op.p)
    return got


@pytest.mark.parametrize("form", RU_FORMS)
def test_every_resunit_case_reaches_its_form(ru_routed, form):
    code, Cc, why = C.RU_FORMS[form][:3]
    for (f, cid), (key, tpz, grid, p) in ru_routed.items():
        if f == form:
            assert key == (code, Cc, why), (form, cid, key)
            bmo = C.bmi(Cc) - (p.k - 1)
            assert tpz == (p.T + bmo - 1) // bmo and grid == min(512, p.n_batch * tpz), (form, cid, tpz, grid)


def test_the_resunit_sweep_reaches_every_form_and_walks_the_tile_loop(ru_routed):
    assert {v[0] for v in ru_routed.values()} == {f[:3] for f in C.RU_FORMS.values()}
    for form in RU_FORMS:
        tiles = {cid: v[3].n_batch * v[1] for (f, cid), v in ru_routed.items() if f == form}
        assert tiles["tiles513"] == 513 and tiles["items601-T5"] == 601 and tiles["tiles1100"] == 1100, form
        assert {1, 2} <= {v[1] for (f, _), v in ru_routed.items() if f == form}


def test_resunit_lean_form_hands_on_an_item_of_2_gib(lib):
    """T * C * 4 >= 2^31 - 1: the lean form's 32-bit byte offsets end, the shared form runs (too large to launch in a
    test: asserted on the route alone)"""
    args, _ = C.materialize(C.make("resunit", "lean-C64", "aligned"))
    op = C.ru_op(args)
    for T, want in ((2 ** 23 - 1, _lib.RESUNIT_FORM_F32), (2 ** 23, _lib.RESUNIT_FORM_SHARED_F32)):
        op.p.T = T
        assert C.ru_route(op.p)[0] == want, T
        assert C.ru_form_key(op.p)[2] == ("auto" if want == _lib.RESUNIT_FORM_F32 else "size")


@pytest.fixture(scope="module")
def tn_routed(lib):
    got = {}
    for cid in C.tn_ids():
        case = C.tn_make(cid)
        args, _ = C.materialize(case)
        op = C.tn_op(args)
        tb, ks, lean = C.tn_route(op.p)
        op.p.route = _lib.TN_ROUTE_GENERAL
        forced = C.tn_route(op.p)
        got[cid] = (tb, ks, lean, forced, dict(args))
    return got


@pytest.mark.parametrize("form", C.TN_FORMS)
def test_every_tn_case_reaches_its_form(tn_routed, form):
    ids = [cid for cid in C.tn_ids() if C.tn_form(cid) == form]
    assert ids
    for cid in ids:
        tb, ks, lean, forced, _ = tn_routed[cid]
        assert C.tn_form_name(tb, lean, ks > 1) == form, (cid, tb, ks, lean)
        assert forced == (tb, ks, False), (cid, forced)  # SRN_TN_ROUTE_GENERAL changes the kernel, nothing else


def test_the_tn_sweep_reaches_every_form_and_both_reduces(tn_routed):
    reached = {C.tn_form_name(tb, lean, ks > 1) for tb, ks, lean, _, _ in tn_routed.values()}
    assert reached == set(C.TN_FORMS), reached ^ set(C.TN_FORMS)
    # tn_reduce_kernel with and without column sums, at both tile edges
    assert {(tb, kw["colsum"] is not None) for tb, ks, _, _, kw in tn_routed.values() if ks > 1} == \
        {(64, False), (64, True), (128, False), (128, True)}
    # a last slice shorter than the others, and one that ends in a partial slab
    tb, ks, _, _, kw = tn_routed["s128-Ta16"]
    assert (tb, ks) == (128, 4) and kw["n_items"] * kw["T_a"] == 528
    tb, ks, _, _, kw = tn_routed["s64-Ta5-K305"]
    assert (tb, ks) == (64, 2)


def test_tn_workspace_fallbacks_answer_one_slice(tn_routed, lib):
    n = 0
    for cid, (tb, ks, lean, _, kw) in tn_routed.items():
        if "ws-" in cid:
            n += 1
            assert ks == 1, cid
            # the same shape with the workspace it asks for is sliced
            p = C._tn_params(kw)
            assert lib.srn_tn_gemm_workspace_bytes(ctypes.byref(p)) > 0, cid
    assert n == 6


# ------------------------------------------------------------------------------------------------------ rejects
@pytest.mark.parametrize("rid", [r[0] for r in C.ru_rejects()])
def test_rejected_resunit_is_refused_by_the_route(lib, rid):
    case, edit = C.ru_reject_case(rid)
    args, _ = C.materialize(case)
    op = C.ru_op(args)
    if edit is not None:
        edit(op.p)
    assert lib.srn_hifigan_resunit_route(ctypes.byref(op.p), (ctypes.c_int32 * 3)()) == -1, rid
    assert case.error.encode() in lib.srn_last_error(), lib.srn_last_error()


@pytest.mark.parametrize("rid", [r[0] for r in C.tn_rejects()])
def test_rejected_tn_gemm_is_refused_by_the_route(lib, rid):
    case, edit = C.tn_reject_case(rid)
    args, _ = C.materialize(case)
    op = C.tn_op(args)
    if edit is not None:
        edit(op.p)
    assert lib.srn_tn_gemm_route(ctypes.byref(op.p), (ctypes.c_int32 * 3)()) == -1, rid
    assert case.error.encode() in lib.srn_last_error(), lib.srn_last_error()


def test_route_queries_refuse_null(lib):
    out = (ctypes.c_int32 * 3)()
    assert lib.srn_tn_gemm_route(None, out) == -1 and b"null params" in lib.srn_last_error()
    assert lib.srn_hifigan_resunit_route(None, out) == -1 and b"null params" in lib.srn_last_error()
    assert lib.srn_tn_gemm_route(ctypes.byref(_lib.SrnTnGemmParams()), None) == -1
    assert lib.srn_hifigan_resunit_route(ctypes.byref(_lib.SrnResUnitParams()), None) == -1


# ------------------------------------------------------------------------------------------- the references themselves
def test_resunit_reference_is_leaky_relu_at_every_slope():
    """the reference's own LeakyReLU against F.leaky_relu's definition, and the shared inputs of the pd0 / pd1 pairs"""
    v = torch.linspace(-3, 3, 25, dtype=torch.float64)
    for slope in (0.0, 0.1, 1.0, 1.5, -0.2):
        assert torch.equal(C._lrelu(v, slope), torch.nn.functional.leaky_relu(v, slope))
    a, b = C.make("resunit", "lean-C32", "res2-pd0"), C.make("resunit", "lean-C32", "res2-pd1")
    assert torch.equal(a.outs[0].ref, b.outs[0].ref)
