"""No GPU: the cases of tests/_speechnet_cases.py are fit to judge the transcriber's and ContentVec's kernels.  Every
case runs through the plain float32 CPU statements of the entry points (emul_transcriber of
tests/test_transcriber_emulated.py, emul_contentvec of tests/test_contentvec_emulated.py) and through the very checks the
GPU test applies, and
  * the float32 statement meets each bound with a factor 10 to spare (beyond one float32 spacing, see ULP below): the
    bounds are attainable, and the inputs are conditioned well enough that a summation order cannot read as error;
  * each case reaches the branch it is named for (worked out from the kernels' own launch rules);
  * for srn_mel_db the three regimes (above both clamps, at amin, at the top_db floor) each hold a tenth of the valid
    elements in some case, and only the all-zero item is clamped in every element."""
import pytest
import torch

from serenade_amd import _lib
from tests import _speechnet_cases as C
from tests.test_contentvec_emulated import emul_contentvec
from tests.test_transcriber_emulated import emul_transcriber

# What a float32 result cannot avoid whatever the order of its sums: the spacing of float32 at the scale the error is
# measured on, 2^-23 of max|ref| (2^-17 dB between 64 and 128 dB).  The factor 10 to spare is asked of what a
# statement errs BEYOND that: a 1e-6 bound is 8 spacings, so a bare factor 10 would ask for less than one.
ULP = 2.0 ** -23
ULP_DB = 2.0 ** -17


def run(name, args):
    (emul_contentvec if name in ("srn_cvec_conv0", "srn_channel_norm_gelu", "srn_posconv_gelu_res")
     else emul_transcriber)(name, args)


def _spare(case, res):
    for what, (err, bound) in res.items():
        print(f"{case} {what}: float32 statement {err:.2e}, bound {bound:.2e}"
              + (f", a factor {bound / err:.1f} to spare" if err > 0 else ""))
        assert err <= bound and 10.0 * max(err - (ULP_DB if what == "dB" else ULP), 0.0) <= bound, (case, what, err, bound)


# (check, case, entry, index of the output among the entry's arguments, element to spoil: a valid one)
NAN_INJECTIONS = [
    (C.check_mel, (65, 16, 50), "srn_mel_db", 6, 0),
    (C.check_conv0, (1, 97, 39, 12), "srn_trans_conv0", 6, (5 * 41 + 7) * 12 + 3),  # item 0, frame 5, column 6
    (C.check_lstm, (72, 1), "srn_bilstm_recur", 5, 0),
    (C.check_cvec, (10, 5, 12, 139, "rand"), "srn_cvec_conv0", 5, 17 * 12 + 2),     # item 0, frame 17: the conv output
    (C.check_cvec, (10, 5, 12, 139, "rand"), "srn_cvec_conv0", 6, 4),               # a partial sum
    (C.check_cvec, (10, 5, 12, 139, "rand"), "srn_channel_norm_gelu", 7, 17 * 12 + 2),  # y
    (C.check_cvec, (10, 5, 12, 139, "rand"), "srn_channel_norm_gelu", 6, 6),        # a mean
    (C.check_pos, (16, 7, 3, 129), "srn_posconv_gelu_res", 4, 40 * 64 + 5),
]


@pytest.mark.parametrize("check,case,entry,arg,at", NAN_INJECTIONS, ids=lambda v: v if isinstance(v, str) else None)
def test_a_nan_in_a_valid_element_fails_the_check(check, case, entry, arg, at):
    """what padding that reached a valid row, or an element left unwritten, looks like: it may not pass as error 0"""
    check(case, run)  # the check passes as it stands

    def spoiled(name, args):
        run(name, args)
        if name == entry:
            args[arg].view(-1)[at] = float("nan")

    with pytest.raises(AssertionError):
        check(case, spoiled)


def test_posconv_without_lengths_is_checked_for_nan():
    def spoiled(name, args):
        run(name, args)
        if args[1] is None:  # only the call with lens == nullptr
            args[4].view(-1)[40 * 64 + 5] = float("nan")

    with pytest.raises(AssertionError):
        C.check_pos((16, 7, 3, 129), spoiled)


@pytest.mark.parametrize("case", C.MEL_CASES, ids=repr)
def test_mel_db_cases(case):
    _spare(case, C.check_mel(case, run))


def test_mel_db_regimes_and_branches():
    shares = [C.mel_regimes(*case) for case in C.MEL_CASES]
    for k, what in enumerate(("above both clamps", "at amin", "at the top_db floor")):
        assert max(s[k] for s in shares) >= 0.1, (what, [round(s[k], 3) for s in shares])
    assert not any(s[3] for s in shares)  # no item but the all-zero one is clamped everywhere
    for nb, nm, T in C.MEL_CASES:
        refs = C.mel_ref(nb, nm, T, 0)
        assert refs[0][0].max().item() > 0 > refs[1][0].max().item()  # both halves of the order-preserving bits decide
        assert C.mel_bound(nb) <= C.MEL_OLD_BOUND
    assert min(nm for _, nm in C.MEL_SHAPES) < 64 and max(nm for _, nm in C.MEL_SHAPES) > 256


@pytest.mark.parametrize("case", C.CONV0_CASES, ids=repr)
def test_trans_conv0_cases(case):
    _spare(case, C.check_conv0(case, run))
    assert all(r is None or r.max().item() > 0 for r in C.conv0_ref(*case))  # ReLU left something to compare


def test_trans_conv0_and_pool_branches():
    assert any(T * (Fq + 2) * C_ > C.CONV0_GRID for _, T, Fq, C_ in C.CONV0_CASES)  # past the grid: the stride loop
    assert {d for d, *_ in C.CONV0_CASES} == {1, 2}
    big = [c for c in C.POOL_CASES if C.POOL_T * C.pool_width(*c) > C.POOL_GRID]
    assert big, "no pool case past the grid"
    for fl, Fin, C_, Cv, extra in C.POOL_CASES:
        assert bool((C.pool_ref(fl, Fin, C_, Cv, extra) < 0).any())  # a maximum seeded with 0 fails
    assert any(fl and Cv < C_ for fl, _, C_, Cv, _ in C.POOL_CASES) and any(F % 2 for _, F, *_ in C.POOL_CASES)
    assert any(fl and C.pool_width(fl, F, C_, Cv, e) > Cv * (F // 2) for fl, F, C_, Cv, e in C.POOL_CASES)  # zero tail


@pytest.mark.parametrize("case", C.POOL_CASES, ids=repr)
def test_trans_pool_cases(case):
    C.check_pool(case, run)


def test_pool_check_rejects_a_zero_seeded_maximum():
    case = (1, 39, 12, 12, 8)

    def seeded(name, args):
        run(name, args)
        args[2].clamp_(min=0.0)

    with pytest.raises(AssertionError):
        C.check_pool(case, seeded)


@pytest.mark.parametrize("case", C.LSTM_CASES, ids=repr)
def test_bilstm_cases(case):
    _spare(case, C.check_lstm(case, run))


def test_bilstm_branches():
    slices = _lib.lib().srn_bilstm_slices
    want = {48: (16, 768, 768, 0), 72: (14, 1008, 1024, 2), 200: (5, 1000, 1024, 0), 344: (2, 688, 704, 0)}
    for H in C.LSTM_H:
        KS = slices(H)
        assert (KS,) + C.lstm_slices(H, KS) == want[H], H
    for H in (32, 40, 384, 512):  # tests/test_hip_transcriber.py's: every launched thread owns a (slice, unit)
        live, launched, _ = C.lstm_slices(H, slices(H))
        assert live == launched, H
    gb = C.lstm_inputs(72, 8)[0]
    assert float(gb[4][torch.isfinite(gb[4])].abs().max()) == 200.0  # expf overflows in the sigmoid
    assert sorted(C.LSTM_LENS)[:2] == [0, 1]


@pytest.mark.parametrize("case", C.CVEC_CASES, ids=repr)
def test_cvec_layer0_cases(case):
    _spare(case, C.check_cvec(case, run))


def test_cvec_layer0_branches():
    shapes = {(k, s, C_) for k, s, C_, _, _ in C.CVEC_CASES}
    assert {(1, 64, 8), (16, 1, 260), (10, 5, 12), (10, 5, 512)} <= shapes
    assert any(C_ % 256 and C_ > 256 for _, _, C_ in shapes) and any(C_ < 256 for _, _, C_ in shapes)
    for T0, lens in C.CVEC_LENS.items():
        assert lens[-1] == 0 and lens[0] == T0
    assert any(T0 % C.C0_FRAMES and T0 > C.C0_FRAMES for *_, T0, _ in C.CVEC_CASES)  # a short last chunk
    assert any(-(-C.CVEC_LENS[T0][1] // C.C0_FRAMES) < -(-T0 // C.C0_FRAMES) for *_, T0, _ in C.CVEC_CASES)  # a chunk past an item
    assert any(T0 * C_ // 4 > C.NORM_GRID_QUADS for _, _, C_, T0, _ in C.CVEC_CASES)  # the norm's grid-stride loop
    k, s, C_, T0, kind = C.CVEC_SHORT_N
    assert C.cvec_inputs(k, s, C_, T0, kind)[1] < (T0 - 1) * s + k
    # the DC case: mean / std of the conv output up to about 60 (statistics in fp32 would lose the variance)
    dc = [c for c in C.CVEC_CASES if c[4] == "dc"][0]
    ratio = max(float((r.mean(0).abs() / r.std(0).clamp_min(1e-30))[[0] + list(range(2, dc[2]))].max())
                for r in C.cvec_conv_ref(*dc) if r is not None)
    assert 40.0 <= ratio <= 90.0, ratio


@pytest.mark.parametrize("case", C.POS_CASES, ids=repr)
def test_posconv_cases(case):
    _spare(case, C.check_pos(case, run))


def test_posconv_branches():
    lds = {(Cg, K): C.pos_lds_bytes(Cg, K) for Cg, K, _ in C.POS_SHAPES}
    assert lds[(64, 128)] == 66300 and sorted(v > 65536 for v in lds.values()) == [False] * 4 + [True]  # the raised limit
    assert {Cg for Cg, *_ in C.POS_SHAPES if Cg > 32 and Cg % 32} == {36, 60}
    assert any(K == 1 for _, K, _ in C.POS_SHAPES) and any(K % 2 and K > 1 for _, K, _ in C.POS_SHAPES)
    assert any(p == 0 and K > 1 for _, K, p in C.POS_SHAPES) and any(p == K - 1 and K > 1 for _, K, p in C.POS_SHAPES)
    assert set(C.POS_LENS) == {1, 128, 129, 300}
    assert [L for L in C.POS_LENS[300] if -(-max(L, 1) // C.PC_BM) < -(-300 // C.PC_BM)] == [150, 20, 0]  # tiles past an item
