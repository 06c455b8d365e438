"""The row / norm / training kernels' sweep (tests/_rowop_cases.py) on the CPU: the emulator -- the executable spec
the rest of the CPU suite trusts -- and a plain fp32 restatement of every op against the float64 references, under the
per-element criterion |g - r| <= tol_op (|r| + s) and the guard-band convention the GPU module applies to the HIP
kernels (tests/test_hip_rowops.py).  This is what pins the tolerance table: the fp32 restatement must stay within
tol_op / 4 on every case."""
import pytest
import torch

from tests import _rowop_cases as R

CASES = R.all_ids(error=False)


@pytest.mark.parametrize("op,cid", CASES, ids=[f"{op}-{cid}" for op, cid in CASES])
def test_emulator_and_fp32_baseline_against_fp64(op, cid):
    case = R.make(op, cid)
    tol = R.tol_for(op, cid)
    args, bufs = R.materialize(case)
    R.run_emulated(case, args)
    e_emul = R.check_outputs(case, bufs)
    print(f"{op} {cid}: emulator {e_emul}, tol {tol}")
    assert R.within(e_emul, tol)
    if op in R.EXACT_OPS or op in R.FIXED_TOL:
        return
    if op in R.BASELINE:  # the emulator computes this op in fp64: the fp32 restatement is a function of its own
        args, bufs = R.materialize(case)
        R.run_baseline(case, args)
        e_base = R.check_outputs(case, bufs)
        print(f"{op} {cid}: fp32 restatement {e_base}")
    else:
        e_base = e_emul
    assert R.within(e_base, (tol[0] / 4, tol[1] / 4)), "the fp32 baseline moved: re-measure the table (python -m tests._rowop_cases)"


def test_table_is_four_times_the_measured_baseline():
    """tol_op = max(4 x baseline, 8 * 2^-24), rounded up to two digits -- never more"""
    for name, (base, tol) in list(R.TOL.items()) + [(k[0], v) for k, v in R.CASE_TOL.items()]:
        want = max(4 * base, R.FLOOR)
        assert want <= tol <= want * 1.1 + 1e-12, name
    swept = set(R.SWEEPS)
    assert swept == set(R.TOL) | set(R.FIXED_TOL) | set(R.EXACT_OPS)
    for op, cid in R.CASE_TOL:
        assert cid in R.case_ids(op) and R.ill_conditioned(op, cid)


def test_sweep_covers_what_it_claims():
    ids = {op: R.case_ids(op) for op in R.SWEEPS}
    # every softmax_rows_kernel<NV> instantiation: nv = ceil(ld / 256) against 2, 4, 8, 12, 20, 36
    nvs = set()
    for cid in ids["srn_softmax_rows"]:
        if not cid.startswith("reject-"):
            nv = (int(cid.split("-")[0][2:]) // 4 + 63) // 64
            nvs.add(min(t for t in (2, 4, 8, 12, 20, 36) if nv <= t))
    assert nvs == {2, 4, 8, 12, 20, 36}
    for op in ("srn_gn_mish_apply", "srn_resblock_tail", "srn_resblock_tail_ln"):
        got = {c.split("-")[0] for c in ids[op]}
        assert {"wg511", "wg512", "wg1000", "lowvar"} <= got          # both sides of SMALL_GRID, and well above
        assert any(c.startswith("wg512-C1024") for c in ids[op])     # C = 1024 with 8 rows per workgroup
    for op in ("srn_layernorm", "srn_rowln_fwd", "srn_rowln_bwd", "srn_gn_mish_bwd_partial", "srn_gn_mish_bwd_apply",
               "srn_gn_stats", "srn_chunk_colsum"):
        assert any("C1024" in c for c in ids[op]), op


def test_host_constants_match_the_library():
    """the sweep sizes its buffers by restating two pure host functions of the library and one constant of the header"""
    from serenade_amd import _lib
    h = _lib.lib()
    for n in (1, 8, 2048, 2049, (1 << 20) + 5, (1 << 21) + 7, 84_287_728):
        assert h.srn_sumsq_blocks(n) == R.sumsq_blocks(n)
    for rows in (1, 16, 17, 4096, 4097, 100_000):
        assert h.srn_bn_chunks(rows) == R.bn_chunks(rows)
    assert _lib.SRN_COPY_LIST_MAX == R.COPY_LIST_MAX


def test_gn_backward_restatement_is_the_gradient():
    """the two-step formula the GroupNorm backward references restate == torch.autograd through F.group_norm, in fp64"""
    formula, auto = R.gn_backward_by_autograd()
    assert float((formula - auto).abs().max()) <= 1e-12 * float(auto.abs().max())


@pytest.mark.parametrize("shape", list(R.im2col_shapes()), ids=lambda s: "B{}-H{}-W{}-C{}-ld{}".format(*s))
def test_im2col_col2im_adjoint(shape):
    """<im2col(x), c> == <x, col2im(c)> in fp64, at 1e-6 relative, through the emulator"""
    lhs, rhs = R.adjoint_pair(shape, R.run_emulated, None)
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))
