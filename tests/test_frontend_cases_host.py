"""No GPU: the cases of tests/_frontend_cases.py are fit to judge the kernels of features.hip and gst.hip.
  * every case runs through the fp32 CPU statements of the entry points (tests/_emulator.py, emul_features of
    tests/test_features_ragged_emulated.py) under the very check the GPU test applies, and stays within tol_op / 4:
    the table of tests/_frontend_cases.py cannot rot;
  * each case reaches the branch it is named for, worked out from the launch rules of features.hip / gst.hip (loop
    trips, block clamps, which regime a loudness bin is in);
  * a NaN in one live output element, or one overwritten sentinel, fails the check;
  * the refused cases are refused by the launchers of the cross-compiled library itself: their argument checks come
    before anything touches a device, so they are called here with host pointers (and again on the GPU, where "writes
    nothing" is also the device's word)."""
import ctypes

import pytest
import torch

from serenade_amd import _lib
from tests import _frontend_cases as C
from tests import _rowop_cases as R

CASES = C.all_ids(error=False)
REJECTS = C.all_ids(error=True)
_id = lambda pairs: [f"{op}-{cid}" for op, cid in pairs]  # noqa: E731


@pytest.mark.parametrize("op,cid", CASES, ids=_id(CASES))
def test_emulator_within_a_quarter_of_tol(op, cid):
    case = C.make(op, cid)
    args, bufs = C.materialize(case)
    C.run_emulated(case, args)
    err = C.check_outputs(case, bufs)[0]
    print(f"{op} {cid}: fp32 statement {err:.3e}, tol {C.tol_for(op):.1e}")
    assert err <= C.tol_for(op) / 4, "the fp32 baseline moved: re-measure the table (python -m tests._frontend_cases)"


def test_table_is_four_times_the_measured_baseline():
    for op, (base, tol) in C.TOL.items():
        want = max(4 * base, C.FLOOR)
        assert want <= tol <= want * 1.1 + 1e-12, op
    assert set(C.SWEEPS) == set(C.TOL) | set(C.EXACT_OPS)
    for op in C.SWEEPS:
        worst = max((C.baseline_error(op, cid) for cid in C.case_ids(op) if not cid.startswith("reject-")), default=0.0)
        if op in C.EXACT_OPS:
            assert worst == 0.0
        else:  # the column is a measurement; the order of an fp32 sum on another CPU may move its last digits
            assert worst <= C.TOL[op][1] / 4, (op, worst)


# ------------------------------------------------------------------------------------------------ spoiled outputs
SPOIL = [  # (op, case id, index of the output among the arguments, element to spoil: a live one)
    ("srn_logmel", "nb257-nm300-ld517-fr3-log10-zerorow2-empty200", 2, 300 + 129),       # frame 1, second mel trip
    ("srn_logmel_ragged", "B3-T4-nb129-nm130-ld261-log10-frames3_4_9", 3, 2 * 130 + 5),  # item 0, its last live frame
    ("srn_loudness", "B3-fr600-nb256-ld513-spike_tiny_rand", 3, 599),                    # item 0, frame 599
    ("srn_loudness_ragged", "B4-T600-nb255-ld510-frames0_1_600_605-quiet1", 4, 600),     # item 1's only frame
    ("srn_pad_signal", "mode0-n257-pad256-tail37-B1", 1, 0),
    ("srn_pad_ragged_zero", "n255-pad1-tail0-gap0-B4-rot8", 3, 257 + 2),
    ("srn_gru_recur_last", "B3-T64-H341", 3, 2 * 341 + 340),
    ("srn_style_token_attention_kv", "B3-Dq300-tok257-F4-h4", 7, 11),
]


@pytest.mark.parametrize("op,cid,arg,at", SPOIL, ids=[s[0] for s in SPOIL])
def test_a_nan_or_an_overwritten_sentinel_fails_the_check(op, cid, arg, at):
    case = C.make(op, cid)
    args, bufs = C.materialize(case)
    C.run_emulated(case, args)
    C.check_outputs(case, bufs)  # passes as it stands
    keep = float(args[arg].view(-1)[at])
    args[arg].view(-1)[at] = float("nan")
    with pytest.raises(AssertionError):
        C.check_outputs(case, bufs)
    args[arg].view(-1)[at] = keep
    C.check_outputs(case, bufs)
    big = bufs[id(case.args[arg])]
    for guard in (R.G - 1, R.G + case.args[arg].n):  # the last element before the payload, the first after it
        big[guard] = 0.0
        with pytest.raises(AssertionError, match="guard band"):
            C.check_outputs(case, bufs)
        big[guard] = R.SENT
    C.check_outputs(case, bufs)


def test_a_dead_row_that_is_not_zero_fails_the_check():
    for op, cid, arg, at in (("srn_logmel_ragged", "B3-T4-nb129-nm130-ld261-log10-frames3_4_9", 3, 3 * 130),
                             ("srn_loudness_ragged", "B4-T600-nb255-ld510-frames0_1_600_605-quiet1", 4, 601),
                             ("srn_pad_signal", "mode0-n2-pad1-tail37-B1", 1, 16)):
        case = C.make(op, cid)
        args, bufs = C.materialize(case)
        C.run_emulated(case, args)
        C.check_outputs(case, bufs)
        assert float(args[arg].view(-1)[at]) == 0.0
        args[arg].view(-1)[at] = 1e-30
        with pytest.raises(AssertionError):
            C.check_outputs(case, bufs)


def test_unread_inputs_hold_nan():
    c = C.make("srn_logmel", "nb5-nm80-ld13-fr3-log2-empty40")
    assert bool(torch.isnan(c.args[0][:, 10:]).all()) and bool(torch.isfinite(c.args[0][:, :10]).all())
    c = C.make("srn_logmel_ragged", "B3-T4-nb129-nm130-ld261-log10-frames3_4_9")
    assert bool(torch.isnan(c.args[0][0, 3:]).all()) and bool(torch.isnan(c.args[0][:, :, 258:]).all())
    c = C.make("srn_loudness_ragged", "B3-T5-nb63-ld129-frames1_5_10-quiet0")
    spec = c.args[0]
    assert bool(torch.isfinite(spec[0, 1:, :126]).all()) and float(spec[0, 1:, :126].abs().max()) > 1e4  # loud, dead
    assert float(spec[0, :1, :126].abs().max()) <= 100.0 and bool(torch.isnan(spec[..., 126:]).all())
    c = C.make("srn_loudness_ragged", "B4-T600-nb255-ld510-frames0_1_600_605-quiet1")
    assert bool(torch.isnan(c.args[0][0]).all())  # frames[0] = 0: nothing of item 0 is read
    c = C.make("srn_pad_ragged_zero", "n256-pad0-tail37-gap9-B4-rot11")
    x, lens = c.args[0], c.meta["lens"]
    assert sorted(lens) == [0, 1, 256, 263]
    for b, ln in enumerate(lens):
        L = min(ln, 256)
        assert bool(torch.isnan(x[b, L:]).all()) and bool(torch.isfinite(x[b, :L]).all())
    for op in ("srn_loudness", "srn_loudness_ragged"):
        for cid in C.case_ids(op):  # a dirty workspace in every case
            ws = C.make(op, cid).args[2 if op == "srn_loudness" else 3]
            assert ws.big.dtype == torch.int32 and bool((ws.initial() == -1).all())


# ------------------------------------------------------------------------------------------------ branches
def _live(op):
    return [C.make(op, cid) for cid in C.case_ids(op) if not cid.startswith("reject-")]


def test_logmel_branches():
    metas = [c.meta for c in _live("srn_logmel")]
    for key, want in (("nb", {1, 5, 127, 128, 129, 257, 8192}), ("nm", {1, 2, 80, 127, 128, 129, 300}),
                      ("frames", {1, 3}), ("mode", {0, 2, 10})):
        assert {m[key] for m in metas} == want, key
    assert {m["ld"] - 2 * m["nb"] for m in metas} == {0, 3}
    assert {(129, 129), (1, 1), (8192, 2)} <= {(m["nb"], m["nm"]) for m in metas}
    wg = C.LOGMEL_WG
    trips = lambda n: -(-n // wg)  # noqa: E731
    assert {trips(m["nm"]) for m in metas} == {1, 2, 3} and {trips(m["nb"]) for m in metas} >= {1, 2, 3}
    assert any(m["nb"] < wg for m in metas) and 8192 * 4 == 32 * 1024
    for m in metas:
        if m["zero_row"] is not None:  # exactly log(eps), in float64
            want = C._LOG64[m["mode"]](torch.tensor(R.f32(C.EPS), dtype=torch.float64))
            assert bool((m["ref"][m["zero_row"]] == want).all())
        if m["empty"] is not None:
            assert bool((m["ref"][:, m["empty"]] == m["ref"][:, m["empty"]][0]).all())
    assert any(m["empty"] is not None and m["empty"] >= wg for m in metas)   # an empty filter in the second trip
    assert any(m["zero_row"] is not None and m["nm"] > wg for m in metas)
    rag = [c.meta for c in _live("srn_logmel_ragged")]
    assert {(m["B"], m["T"]) for m in rag} == {(1, 1), (3, 4), (5, 6)}
    seen = set()
    for c in _live("srn_logmel_ragged"):
        T = c.meta["T"]
        seen |= {("0", "1", "T-1", "T", "T+5")[(0, 1, T - 1, T, T + 5).index(int(f))] for f in c.args[2]
                 if int(f) in (0, 1, T - 1, T, T + 5)}
    assert seen == {"0", "1", "T-1", "T", "T+5"}
    assert any(m["nm"] > wg for m in rag)


def test_loudness_regimes_and_branches():
    cases = _live("srn_loudness")
    metas = [c.meta for c in cases]
    assert {m["B"] for m in metas} == {1, 3} and {m["frames"] for m in metas} == {1, 2, 513, 600}
    assert {m["nb"] for m in metas} == {1, 63, 255, 256, 257, 1025}
    assert {m["ld"] - 2 * m["nb"] > 0 for m in metas} == {True, False}
    assert sum(m["frames"] > C.POWER_MAX_GRID for m in metas) >= 2            # power_max_kernel's grid-stride loop
    assert any(m["nb"] < C.LOUD_WG for m in metas) and any(m["nb"] > 4 * C.LOUD_WG for m in metas)
    for k, what in enumerate(("above both clamps", "at amin", "at the top_db floor")):
        best = max(sum(sh[k] for sh in m["shares"]) / m["B"] for m in metas)  # share of the case's live bins
        assert best >= 0.1, (what, best)
    kinds = {k for m in metas for k in m["kinds"]}
    assert kinds == set(C.KINDS)
    for m in metas:
        for kind, sh in zip(m["kinds"], m["shares"]):
            if kind == "zero":
                assert sh == (0.0, 1.0, 0.0)
            if kind == "spike" and m["frames"] * m["nb"] > 1:  # every bin but the spike sits at the floor
                assert sh[2] == 1.0 - 1.0 / (m["frames"] * m["nb"])
            if kind == "lastmax" and m["frames"] * m["nb"] > 100:
                assert 0.3 < sh[2] < 0.55   # the floor of -40 dB cuts levels uniform in [-70, 0] dB
    for c in cases:  # the loudest bin of a lastmax item is its last frame's last bin
        for b, kind in enumerate(c.meta["kinds"]):
            if kind == "lastmax":
                nb = c.meta["nb"]
                p = c.args[0][b, :, :nb].double() ** 2 + c.args[0][b, :, nb:2 * nb].double() ** 2
                assert int(p.argmax()) == p.numel() - 1
    assert float(C.a_weight(257)[0]) == -80.0 and float(C.a_weight(257)[1:].min()) > -80.0  # the table's clamp
    rag = [c.meta for c in _live("srn_loudness_ragged")]
    assert {(m["B"], m["T"]) for m in rag} == {(1, 1), (3, 5), (4, 600)}
    assert {m["nb"] for m in rag} == {1, 63, 255, 256, 257, 1025}
    assert any(m["quiet"] is not None and 0 < m["live"][m["quiet"]] < m["T"] for m in rag)
    for c in _live("srn_loudness_ragged"):
        T = c.meta["T"]
        assert all(int(f) in (0, 1, T, T + 5) for f in c.args[2])
    assert {int(f) - c.meta["T"] for c in _live("srn_loudness_ragged") for f in c.args[2]} >= {0, 5}


def test_pad_branches():
    for op in ("srn_pad_signal", "srn_pad_ragged_zero"):
        lds = [c.args[5 if op == "srn_pad_signal" else 7] for c in _live(op)]
        assert sum(ld > C.PAD_WG * C.PAD_GRID for ld in lds) == 1 and max(lds) == C.BIG_LD   # the block clamp
        assert any(ld < C.PAD_WG for ld in lds)
    sig = [tuple(c.args[2:7]) for c in _live("srn_pad_signal")]  # (B, n, pad, ld, mode)
    assert {s[1] for s in sig} >= set(C.PAD_N) and {s[0] for s in sig} == {1, 3} and {s[4] for s in sig} == {0, 1}
    for n in C.PAD_N:
        assert {(0, 0), (1, 0), (n - 1, 0), (n - 1, 1), (n + 5, 1)} & {(s[2], s[4]) for s in sig if s[1] == n} \
            >= {(n - 1, 0), (n - 1, 1), (n + 5, 1)}
        assert {s[2] for s in sig if s[1] == n} >= {0, 1, n - 1, n + 5}
    assert {s[3] - s[1] - 2 * s[2] for s in sig if s[1] <= 1000} == {0, 37}
    rag = _live("srn_pad_ragged_zero")
    assert {c.args[1] - c.args[5] for c in rag} == {0, 9}
    for n in C.PAD_N:
        assert {ln for c in rag if c.args[5] == n for ln in c.meta["lens"]} == {0, 1, n, n + 7}


def test_gst_branches():
    gru = [c.meta for c in _live("srn_gru_recur_last")]
    assert {m["H"] for m in gru} == set(C.GRU_H) and {m["T"] for m in gru} == {1, 2, 64} and {m["B"] for m in gru} == {1, 3}
    threads = lambda H: -(-3 * H // 64) * 64  # noqa: E731  the launcher's rule
    assert (threads(21), threads(22), threads(341)) == (64, 128, 1024)
    assert (3, 64, 341) in {(m["B"], m["T"], m["H"]) for m in gru}
    att = [c.meta for c in _live("srn_style_token_attention_kv")]
    assert {m["Dq"] for m in att} >= {1, 128, 257, 300} and {m["n_tok"] for m in att} >= {1, 10, 50, 257}
    assert {m["F"] for m in att} == {4, 256, 260} and {m["B"] for m in att} >= {1, 3}
    assert {"1" if m["nh"] == 1 else "F" if m["nh"] == m["F"] else str(m["nh"]) for m in att} == {"1", "4", "F"}
    assert any(m["nh"] * m["n_tok"] > C.ATTN_WG for m in att)      # the score loop's second trip
    assert max(m["nh"] for m in att) == C.ATTN_WG                 # the most heads the softmax has threads for
    assert any(m["F"] > C.ATTN_WG for m in att) and any(m["Dq"] > C.ATTN_WG for m in att)  # second trips of the projections
    B, Dq, tok, Fd, nh = C.ATTN_LDS_LIMIT
    assert C.attn_lds_bytes(Dq, tok, Fd, nh) == C.ATTN_LDS and C.attn_lds_bytes(Dq + 1, tok, Fd, nh) > C.ATTN_LDS
    assert C.attn_lds_bytes(8, 2, 516, 258) < C.ATTN_LDS  # only the head count refuses that case


# ------------------------------------------------------------------------------------------------ refusals
def _c_args(args):
    out = []
    for a in args:
        if isinstance(a, C.Buf):
            a = a.big[R.G:]
        if isinstance(a, torch.Tensor):
            out.append(ctypes.c_void_p(a.data_ptr()))
        else:
            out.append(a)
    return out


@pytest.mark.parametrize("op,cid", REJECTS, ids=_id(REJECTS))
def test_refused_by_the_library(op, cid):
    """the launcher's own SRN_CHECK_ARG: non-zero return and the entry's name with the reason in srn_last_error.
    Nothing is dereferenced before the checks, so host pointers do; a call that passed them would reach
    hipLaunchKernel without a device and fail there with another message."""
    h = _lib.lib()
    case = C.make(op, cid)
    assert h.srn_pad_ragged(None, 8, None, None, 2, 8, 2, 16, None) != 0 and b"pad_ragged" in h.srn_last_error()
    rc = getattr(h, op)(*_c_args(case.args), None)
    msg = h.srn_last_error().decode()
    assert rc == -1 and case.error in msg and op[4:] + ":" in msg, (rc, msg)


def test_the_refused_cases_are_the_issue_s():
    want = {"srn_logmel": {"reject-nb8193", "reject-ld-short", "reject-log3", "reject-frames0"},
            "srn_logmel_ragged": {"reject-B65536"},
            "srn_loudness": {"reject-ld-short", "reject-frames0", "reject-B65536"},
            "srn_loudness_ragged": {"reject-B65536", "reject-ld-short"},
            "srn_pad_signal": {"reject-reflect-pad-n", "reject-n1", "reject-ld-short", "reject-B65536"},
            "srn_pad_ragged_zero": {"reject-x_bs-short", "reject-ld-short", "reject-B65536"},
            "srn_gru_recur_last": {"reject-H342"},
            "srn_style_token_attention_kv": {"reject-lds", "reject-h258-F516", "reject-F6-h4"}}
    got = {}
    for op, cid in REJECTS:
        got.setdefault(op, set()).add(cid)
    assert got == want
