"""Case generators and float64 references for the two hand-written MFMA launch families outside the conv sweep: the
fused HiFi-GAN residual unit (srn_hifigan_resunit: resunit.hip, resunit_f32.hip) and the contractions over time of the
training step (srn_tn_gemm: tn_gemm.hip).

Shared by tests/test_mfmasweep_emulated.py (CPU: the emulator and the restatements against these references, and the
route of every case on the cross-compiled library) and tests/test_hip_mfmasweep.py (MI355X: the kernels against the same
references).  No GPU is touched here.  Buf / Out / Case / materialize / check_outputs are those of tests/_rowop_cases.py.

A case is the keyword dict of one ``ops.ResUnitOp`` / ``ops.TnGemmOp`` (``Case.args`` holds its items) and names the
form it is meant for; the library's route queries (srn_hifigan_resunit_route, srn_tn_gemm_route) decide whether it gets
there.  Forms:
  residual unit   {lean fp32 (resunit_f32.hip), shared fp32 by SRN_RESUNIT_ROUTE_SHARED, shared fp32 by a slope outside
                  [0, 1], bf16x3} x C in {32, 64}
  srn_tn_gemm     tile edge {64, 128} x {lean, general} x {K sliced, not}; tn_reduce_kernel with and without colsum
Every buffer a call writes is a Buf between guard bands: out (or the in-place res2) of the residual unit; out, colsum and
the workspace of srn_tn_gemm (exactly the bytes srn_tn_gemm_workspace_bytes asks for).  ld padding columns and the gaps
between items start as sentinels (in place: as their input values) and must come back bit for bit.  The inputs' padding
columns (a in [M, lda), b in [N, ldb)), the rows of b at or past len_b and every gap between items of a, b and x hold
NaN; every output must still be finite.  Output columns of a shift that pairs no row of a with a row of b inside
[0, min(T_b, len_b)) must be exactly zero.

References are float64 torch from the same fp32 inputs, written independently of tests/_emulator.py:
  residual unit   gather of the tap rows (zero outside [0, T)) and a matmul, twice; the intermediate exists for rows
                  [0, T) only, so conv2 sees zeros outside them; LeakyReLU is where(x > 0, x, slope x) at every slope
  srn_tn_gemm     the header's formula, item by item: rows of b outside [0, min(T_b, len_b)) count as zero whatever they
                  hold, columns of a at or past M and of b at or past N are never read

Pass criterion, per element:   |got - ref| <= tol (|ref| + s)
with s the size of the terms summed: |alpha| sum |a| |b| for srn_tn_gemm's output, |alpha| sum |a| for colsum;
(|lrelu(xt)| (*) |w2|) + |b2| + |x| + |res2| for the residual unit, divided by post_div where it divides.

tol is not chosen: 4 x the worst error over this same sweep, under this same formula, of a CPU restatement in the
arithmetic of the mode, rounded up to two digits, floor 8 * 2^-24 (`python -m tests._mfma_cases` prints the column
again; test_mfmasweep_emulated.py holds the restatements to tol / 4):

  row              baseline    tol        restatement
  tn               1.937e-07   7.8e-07    tests/_emulator.emul_tn_gemm's loop with fp32 products and sums (the emulator
                                         itself accumulates in fp64)
  resunit-fp32     3.387e-07   1.4e-06    tests/_emulator.emul_resunit (fp32 torch)
  resunit-bf16x6   the fp32 row: bf16x6 on the residual unit runs the fp32 form and is held to it
  resunit-bf16x3   3.945e-06   1.6e-05    both convolutions with operands split as the kernel splits them (the image
                                         after LeakyReLU, the intermediate after bias + LeakyReLU, hi = bf16(v),
                                         lo = bf16(v - hi); weights: the planes of ops.weight_planes), three products
                                         A_lo W_hi + A_hi W_lo + A_hi W_hi accumulated in fp32
No case needs a tolerance of its own (CASE_TOL is empty).

The residual unit's fall-back from the lean form for T * C * 4 >= 2^31 is asserted through the route query only
(test_mfmasweep_emulated.py): one such item is 2 GiB, too large to run in a test.
Where a variant cannot reach a form it is left out of that form's list, nothing else: the lean form takes slopes in
[0, 1] only (others ARE the slope-fallback form, whose base slope is 1.5), bf16x6 runs on the fp32 forms.
"""
import ctypes

import torch

from serenade_amd import _lib, ops
from tests._rowop_cases import (FLOOR, Buf, Case, Out, _bits, _Rng, _round_up, check_outputs,  # noqa: F401
                                materialize)

FP32, X3, X6 = _lib.PREC_FP32, _lib.PREC_BF16X3, _lib.PREC_BF16X6
NAN = float("nan")

# row -> (measured baseline of the restatement, tol); filled from `python -m tests._mfma_cases`
TOL = {
    "tn": (1.937e-07, 7.8e-07),
    "resunit-fp32": (3.387e-07, 1.4e-06),
    "resunit-bf16x6": (3.387e-07, 1.4e-06),
    "resunit-bf16x3": (3.945e-06, 1.6e-05),
}
CASE_TOL = {}  # (form, case id) -> (baseline, tolerance): none needed


def library():
    """the cross-compiled library (a no-op when it is up to date)"""
    from serenade_amd import build
    build.build(verbose=False)
    return _lib.lib()


def _r4(n):
    return (n + 3) // 4 * 4


# =========================================================================================== the residual unit
KD = ((1, 1), (3, 1), (3, 25), (5, 2), (7, 3), (11, 1), (11, 5), (13, 4), (51, 1))
RU_FORMS = {}  # name -> (what the route answers, C, why, precision, route field, base slope)
for _C in (32, 64):
    RU_FORMS[f"lean-C{_C}"] = (_lib.RESUNIT_FORM_F32, _C, "auto", FP32, 0, 0.1)
    RU_FORMS[f"shared-C{_C}"] = (_lib.RESUNIT_FORM_SHARED_F32, _C, "route", FP32, _lib.RESUNIT_ROUTE_SHARED, 0.1)
    RU_FORMS[f"slopefb-C{_C}"] = (_lib.RESUNIT_FORM_SHARED_F32, _C, "slope", FP32, 0, 1.5)
    RU_FORMS[f"bf16x3-C{_C}"] = (_lib.RESUNIT_FORM_BF16X3, _C, "auto", X3, 0, 0.1)


def bmi(C):
    return 256 if C == 32 else 128


def ru_variants(form):
    """[(case id, spec)] of one form of the residual unit"""
    _, C, why, prec, _, _ = RU_FORMS[form]
    V = []

    def add(vid, **kw):
        V.append((vid, kw))

    # every (k, d) with a tile seam inside the item: BMo + 1 rows -> a second tile of one row, whose receptive field
    # reaches back over the seam
    for k, d in KD:
        add(f"k{k}d{d}-seam", k=k, d=d, T=bmi(C) - (k - 1) + 1)
    # T below the halo (k 11, d 5: (k - 1) / 2 = 5, (k - 1) d = 50), T = 1 at k = 1
    for T in (1, 2, 5, 50):
        add(f"k11d5-T{T}", k=11, d=5, T=T)
    add("k1d1-T1", k=1, d=1, T=1)
    add("k51d1-T25", k=51, d=1, T=25)
    # around the tile at k = 3; last tiles of 31 / 32 / 33 rows: the two epilogue branches of resunit_f32.hip
    bmo = bmi(C) - 2
    for name, T in (("BMo-1", bmo - 1), ("BMo", bmo), ("2BMo+1", 2 * bmo + 1), ("last31", bmo + 31), ("last32", bmo + 32),
                    ("last33", bmo + 33)):
        add(f"k3d1-{name}", T=T)
    add("k7d3-last33", k=7, d=3, T=bmi(C) - 6 + 33)
    # the persistent loop: 513 tiles of full length (one workgroup walks two), 601 items of one short tile each, 1100
    # tiles over 550 items (two and three tiles per workgroup, uneven)
    add("tiles513", B=9, T=57 * bmo)
    add("items601-T5", B=601, T=5)
    add("tiles1100", B=550, T=bmo + 1)
    add("tiles1100-k11d5", B=550, T=bmi(C) - 10 + 1, k=11, d=5)
    # epilogue: res2 of its own / in place, post_div 0 / 1 / 3 (pd0 and pd1 share inputs: the same bits)
    for epi in ("res2", "inplace"):
        for pd in (0.0, 1.0, 3.0):
            add(f"{epi}-pd{int(pd)}", epi=epi, post_div=pd, T=bmo + 33, key=f"{epi}-pd")
    add("none-pd3", post_div=3.0)
    add("none-pd1", post_div=1.0)
    add("aligned", T=40, align=True)  # out / res2 at 16-byte aligned addresses, contiguous items (every other case: neither)
    for slope in (0.0, 1.0) if why != "slope" else ():
        add(f"slope{slope}", slope=slope, T=bmo + 33, epi="res2")
    if why != "auto" or prec == X3:  # slopes the lean form hands on
        for slope in (1.5, -0.2):
            add(f"slope{slope}", slope=slope, T=bmo + 33, epi="res2")
            add(f"slope{slope}-k11d5-T50", slope=slope, k=11, d=5, T=50)
    if why == "auto" and prec == FP32:
        add("x6", precision=X6, T=bmo + 33, epi="inplace", post_div=3.0)
    return V


def ru_case(form, vid, spec):
    code, C, why, prec, route, slope0 = RU_FORMS[form]
    g = spec.get
    k, d, B, T = g("k", 3), g("d", 1), g("B", 2), g("T", 33)
    slope = g("slope", slope0)
    rng = _Rng(f"resunit-{form}-{g('key', vid)}")
    item = T * C
    al = bool(g("align", False))
    x_bs, out_bs, res2_bs = (item, item, item) if al else (item + 8, item + 4, item + 12)
    x_off, out_off, res2_off = (4, 0, 4) if al else (4, 1, 3)
    x = torch.full((x_off + B * x_bs,), NAN)
    torch.as_strided(x, (B, item), (x_bs, 1), x_off).copy_(rng.n(B, item))
    scale = 1.0 / (k * C) ** 0.5
    w1, w2 = rng.n(C, k * C) * scale, rng.n(C, k * C) * scale
    b1 = 1.5 + 0.5 * rng.n(C)  # order 1 with a mean: an intermediate not zeroed outside [0, T) shows
    b2 = rng.n(C)
    epi = g("epi", "none")
    n_out = out_off + B * out_bs
    out = Buf(n_out, init=rng.n(n_out) if epi == "inplace" else None)
    kw = dict(x=(x, x_off), w1=w1, b1=b1, w2=w2, b2=b2, out=(out, out_off), n_batch=B, T=T, C=C, k=k, dilation=d,
              slope=slope, post_div=g("post_div", 0.0), precision=g("precision", prec), route=route, x_bs=x_bs,
              out_bs=out_bs, res2_bs=res2_bs)
    if epi == "res2":
        q = torch.full((res2_off + B * res2_bs,), NAN)
        torch.as_strided(q, (B, item), (res2_bs, 1), res2_off).copy_(rng.n(B, item))
        kw.update(res2=(q, res2_off))
    elif epi == "inplace":
        kw.update(res2=(out, out_off), res2_bs=out_bs)
    ref = torch.zeros(n_out, dtype=torch.float64)
    s = torch.zeros(n_out, dtype=torch.float64)
    written = torch.zeros(n_out, dtype=torch.bool)
    for b0, val, sv in ru_contract(kw):
        idx = out_off + (b0 + torch.arange(val.shape[0]))[:, None] * out_bs + torch.arange(item)[None]
        ref[idx], s[idx], written[idx] = val.reshape(-1, item), sv.reshape(-1, item), True
    return Case(f"{form} {vid}", tuple(kw.items()), [Out("out", out, ref, s=s, written=written)], kind="resunit")


def _flat0(x):
    """(flat fp32 tensor as the call finds it, element offset) of a tensor, Buf or (tensor | Buf, offset) pair"""
    off = 0
    if isinstance(x, tuple):
        x, off = x
    return (x.initial() if isinstance(x, Buf) else x.reshape(-1)), int(off)


def _lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def _gather(a, k, step):
    """(B, T, C) -> (B, T, k * C): rows t + (j - (k - 1) / 2) * step, zero outside [0, T)"""
    B, T, C = a.shape
    ti = torch.arange(T)[:, None] + (torch.arange(k)[None] - (k - 1) // 2) * step
    live = (ti >= 0) & (ti < T)
    A = a[:, ti.clamp(0, T - 1)]  # (B, T, k, C)
    return torch.where(live[None, :, :, None], A, torch.zeros((), dtype=a.dtype)).reshape(B, T, k * C)


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def ru_contract(kw, dt=torch.float64, mm=None, w_planes=None):
    """the unit in dtype dt (float64: the reference), a few items at a time: yields (first item, val, s) with val / s of
    shape (items, T, C).  mm(A, W_hi_lo) -> A W^T replaces both products (the split-bf16 restatement)."""
    g = kw.get
    B, T, C, k, d = g("n_batch"), g("T"), g("C"), g("k"), g("dilation")
    slope, pdiv = _f32(g("slope")), _f32(g("post_div", 0.0))
    xf, xo = _flat0(g("x"))
    w1, w2 = (g("w1").to(dt), g("w2").to(dt)) if w_planes is None else w_planes
    b1, b2 = g("b1").to(dt), g("b2").to(dt)
    qf, qo = _flat0(g("res2")) if g("res2") is not None else (None, 0)
    want_s = dt == torch.float64
    step = max(1, (1 << 22) // (T * k * C))
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        x = torch.as_strided(xf, (nb, T, C), (g("x_bs"), C, 1), xf.storage_offset() + xo + b0 * g("x_bs")).to(dt)
        A1 = _gather(_lrelu(x, slope), k, d)
        h = (A1 @ w1.t() if mm is None else mm(A1, w1)) + b1
        A2 = _gather(_lrelu(h, slope), k, 1)
        y = (A2 @ w2.t() if mm is None else mm(A2, w2)) + b2
        val = y + x
        s = A2.abs() @ w2.abs().t() + b2.abs() + x.abs() if want_s else None
        if qf is not None:
            q = torch.as_strided(qf, (nb, T, C), (g("res2_bs"), C, 1), qf.storage_offset() + qo + b0 * g("res2_bs")).to(dt)
            val = val + q
            s = s + q.abs() if want_s else None
        if pdiv not in (0.0, 1.0):
            val = val / pdiv
            s = s / abs(pdiv) if want_s else None
        yield b0, val, s


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def ru_run_bf16x3(args):
    """the bf16x3 baseline: both convolutions restated in fp32 with split operands, stored like the kernel stores it"""
    kw = dict(args)
    C, k = kw["C"], kw["k"]

    def planes(w):  # [C][k][C / 32][hi 32 | lo 32] -> (hi, lo) as [C][k * C] fp32
        pl = ops.weight_planes(w, C, k, C, k * C)[0].to(torch.float32)
        return pl[:, :, :, 0].reshape(C, k * C), pl[:, :, :, 1].reshape(C, k * C)

    def mm(A, W):
        wh, wl = W
        ah = _bf(A)
        al = _bf(A - ah)
        return (al @ wh.t() + ah @ wl.t()) + ah @ wh.t()

    todo = list(ru_contract(kw, torch.float32, mm, (planes(kw["w1"]), planes(kw["w2"]))))  # in place: read before storing
    of, oo = kw["out"][0].view(-1), kw["out"][1]
    for b0, val, _ in todo:
        torch.as_strided(of, val.shape, (kw["out_bs"], C, 1), of.storage_offset() + oo + b0 * kw["out_bs"]).copy_(val)


def ru_run_emulated(args):
    from tests import _emulator
    _emulator.emul_resunit(dict(args))


def ru_rejects():
    """[(id, keyword changes, params edit, message)] over one valid base call"""
    def no_planes(p):  # on a GPU ResUnitOp attaches the planes itself
        p.w1_hi = p.w2_hi = None
    return [
        ("C48", dict(C=48), None, "takes 32 or 64 channels"),
        ("k-even", dict(k=4), None, "outside the staged halo"),
        ("halo52", dict(k=5, dilation=13), None, "outside the staged halo"),
        ("out-is-x", dict(alias=True), None, "out must not alias x"),
        ("null-b1", dict(null="b1"), None, "null pointer"),
        ("x-misaligned", dict(x_off=5), None, "must be 16-byte aligned"),
        ("x_bs%4", dict(x_bs_extra=2), None, "must be 16-byte aligned"),
        ("x3-no-planes", dict(precision=X3), no_planes, "needs the weight planes"),
    ]


def ru_reject_case(rid):
    _, ch, edit, msg = next(r for r in ru_rejects() if r[0] == rid)
    rng = _Rng("resunit-reject-" + rid)
    B, T, C, k = 2, 33, ch.get("C", 32), ch.get("k", 3)
    item = T * C
    x_bs = item + 8 + ch.get("x_bs_extra", 0)
    x = rng.n(8 + B * x_bs)
    out = Buf(B * item)
    kw = dict(x=(x, ch.get("x_off", 4)), w1=rng.n(64, k * 64), b1=rng.n(64), w2=rng.n(64, k * 64), b2=rng.n(64),
              out=(out, 0), n_batch=B, T=T, C=C, k=k, dilation=ch.get("dilation", 1), slope=0.1,
              precision=ch.get("precision", FP32), x_bs=x_bs)
    if ch.get("null"):
        kw[ch["null"]] = None
    if ch.get("alias"):  # out = x: the Buf stands in for both
        kw.update(x=(out, 0), x_bs=item)
    outs = [Out("out", out, torch.zeros(out.n, dtype=torch.float64), written=torch.zeros(out.n, dtype=torch.bool))]
    return Case("reject " + rid, tuple(kw.items()), outs, kind="resunit", error=msg), edit


def ru_op(args, planes=False):
    """ops.ResUnitOp of materialized args; planes: stand-in weight planes for the route on the CPU (the route only asks
    whether there are any; on a GPU ResUnitOp builds the real ones)"""
    op = ops.ResUnitOp(**dict(args))
    if planes and op.p.precision == X3 and not op.p.w1_hi:
        op.p.w1_hi, op.p.w2_hi = op.p.w1, op.p.w2
    return op


def ru_route(p):
    out = (ctypes.c_int32 * 3)()
    _lib.check(library().srn_hifigan_resunit_route(ctypes.byref(p), out), "srn_hifigan_resunit_route")
    return out[0], out[1], out[2]


def ru_form_key(p):
    """(form the route answers, C, why) of filled params, as RU_FORMS spells a form"""
    code = ru_route(p)[0]
    why = "auto"
    if code == _lib.RESUNIT_FORM_SHARED_F32:
        why = "route" if p.route == _lib.RESUNIT_ROUTE_SHARED else "slope" if not 0.0 <= p.slope <= 1.0 else "size"
    return code, p.C, why


# ================================================================================================== srn_tn_gemm
def tn_form_name(tb, lean, sliced):
    return f"t{tb}-{'lean' if lean else 'general'}-{'sliced' if sliced else 'one'}"


TN_FORMS = [tn_form_name(tb, lean, sl) for tb in (64, 128) for lean in (True, False) for sl in (True, False)]
MS = (1, 3, 63, 64, 65, 127, 128, 129, 203)
NS = (4, 60, 64, 68, 132)
KS = (1, 3, 15, 16, 17)
SHIFTS16 = (3, -1, 0, 0, -20, 25, 1, -2, 7, 7, -19, 19, 18, -18, 2, 5)  # unsorted, duplicated; T_b = 19: four shifts miss b


def tn_specs():
    """{case id: (form, spec)}: the form is what the case is meant for; the route query decides"""
    S = {}

    def add(cid, tb, lean, sliced, **kw):
        assert cid not in S
        S[cid] = (tn_form_name(tb, lean, sliced), kw)

    # ---- tile 64, one slice: the shape edges.  K = n_items * T_a in {1, 3, 15, 16, 17}; ld padding everywhere
    for i, M in enumerate(MS):
        K = KS[i % 5]
        add(f"M{M}-N{NS[i % 5]}-K{K}", 64, K % 16 == 0, False, M=M, N=NS[i % 5], n_items=1, T_a=K, shifts=(-1, 0, 1),
            alpha=(1.0, 0.5, -2.0)[i % 3])
    for N in NS:
        add(f"N{N}-M65-K17", 64, False, False, M=65, N=N, n_items=1, T_a=17, shifts=(0, 3))
    for K in KS:
        add(f"M129-N68-K{K}x3", 64, K % 16 == 0, False, M=129, N=68, n_items=3, T_a=K, shifts=(0, 2))
    # a 16-row slab spans several items: the general kernel's reseat loop
    for T_a in (1, 3, 5, 7):
        add(f"Ta{T_a}-items30", 64, False, False, n_items=30, T_a=T_a, shifts=(-1, 0, 1))
    add("inner2", 64, False, False, n_items=6, T_a=7, n_inner=2, shifts=(-1, 0, 1))
    add("inner3-Ta16", 64, False, False, n_items=6, T_a=16, n_inner=3, shifts=(0, 1))
    add("Ta16-items5", 64, True, False, n_items=5, T_a=16, shifts=(-1, 0, 1))
    add("Ta48-items3", 64, True, False, n_items=3, T_a=48, shifts=(-2, 0, 2), alpha=0.5)
    # taps
    add("shifts16", 64, False, False, n_items=3, T_a=19, shifts=SHIFTS16)
    add("shifts16-Ta16", 64, True, False, n_items=3, T_a=16, T_b=19, shifts=SHIFTS16)
    for st in (2, 3):
        add(f"stride{st}", 64, False, False, n_items=3, T_a=13, stride=st, T_b=13 * st - 2, shifts=(-1, 0, 1))
        add(f"stride{st}-Ta16", 64, True, False, n_items=3, T_a=16, stride=st, T_b=16 * st - 2, shifts=(-1, 0, 1))
    # len_b: 0, 1, T_b, T_b + 5 within one call; n_batch = 3 indexes it zb * n_items + item
    for nb in (1, 3):
        add(f"lenb-nb{nb}", 64, False, False, n_batch=nb, n_items=4, T_a=13, shifts=(-1, 0, 1), len_b=True)
        add(f"lenb-nb{nb}-Ta16", 64, True, False, n_batch=nb, n_items=4, T_a=16, shifts=(-1, 0, 1), len_b=True)
    # problems: batch x head with head slices of b and out, an out column offset (attention's dK / dV)
    add("heads", 64, False, False, n_batch=2, n_head=3, M=43, N=32, n_items=1, T_a=43, heads=True, coloff=8, alpha=0.5)
    add("heads-Ta48", 64, True, False, n_batch=2, n_head=3, M=48, N=32, n_items=1, T_a=48, heads=True, coloff=8, alpha=-2.0)
    add("heads-own", 64, False, False, n_batch=2, n_head=2, M=33, N=36, n_items=2, T_a=9, shifts=(0, 1))
    # column sums, one slice: more than one m-tile, NaN in a's padding columns
    for M in (4, 68, 132):
        add(f"colsum-M{M}", 64, False, False, M=M, N=36, n_items=3, T_a=11, colsum=True, alpha=0.5)
    add("colsum-M132-Ta16", 64, True, False, M=132, N=36, n_items=3, T_a=16, colsum=True)
    # ---- tile 64, sliced (tiles128 <= 8, K >= 256)
    add("s64-Ta16-K272", 64, True, True, n_items=17, T_a=16)  # 2 slices: 144 + 128
    add("s64-Ta48-K336", 64, True, True, n_items=7, T_a=48, shifts=(-1, 0, 1))  # k_per 176: the boundary inside item 3
    add("s64-Ta5-K305", 64, False, True, n_items=61, T_a=5, shifts=(-1, 0, 1))  # k_per 160, last slice 145: a partial slab
    add("s64-inner2", 64, False, True, n_items=40, T_a=7, n_inner=2)
    add("s64-lenb-nb3", 64, True, True, n_batch=3, n_items=17, T_a=16, len_b=True, shifts=(-1, 0))
    add("s64-lenb-nb3-Ta5", 64, False, True, n_batch=3, n_items=61, T_a=5, len_b=True, shifts=(-1, 0))
    add("s64-heads", 64, True, True, n_batch=2, n_head=2, M=272, N=32, n_items=1, T_a=272, heads=True, coloff=4, alpha=0.5)
    for M in (68, 132):
        add(f"s64-colsum-M{M}", 64, True, True, M=M, N=68, n_items=17, T_a=16, colsum=True, alpha=-2.0)
    add("s64-colsum-M132-Ta5", 64, False, True, M=132, N=4, n_items=61, T_a=5, colsum=True)
    # the workspace fall-backs: the same sliced shapes end in one slice
    for ws in ("null", "small", "misaligned"):
        add(f"ws-{ws}", 64, True, False, n_items=17, T_a=16, ws=ws)
    add("ws-null-colsum-Ta5", 64, False, False, M=132, N=4, n_items=61, T_a=5, colsum=True, ws="null")
    # ---- tile 128, sliced: M = N = 384, K = 528 -> four slices of 144 rows, the last with 96
    add("s128-Ta16", 128, True, True, M=384, N=384, n_items=33, T_a=16)
    add("s128-Ta48-colsum", 128, True, True, M=384, N=384, n_items=11, T_a=48, colsum=True, alpha=0.5)
    add("s128-Ta3", 128, False, True, M=384, N=384, n_items=176, T_a=3)
    add("s128-inner3-colsum", 128, False, True, M=384, N=384, n_items=48, T_a=11, n_inner=3, colsum=True)
    add("s128-M259-lenb", 128, True, True, M=259, N=260, n_items=33, T_a=16, len_b=True)  # tiles128 = 9, ragged both ways
    # ---- tile 128, one slice: tiles128 >= 384, or the sliced shape without a workspace
    add("u128-Ta16", 128, True, False, M=132, N=132, n_batch=2, n_head=3, n_items=2, T_a=16, T_b=20, shifts=SHIFTS16)
    add("u128-Ta7", 128, False, False, M=129, N=132, n_batch=3, n_head=2, n_items=3, T_a=7, T_b=19, shifts=SHIFTS16,
        len_b=True)
    add("u128-ws-null", 128, True, False, M=384, N=384, n_items=33, T_a=16, ws="null")
    add("u128-ws-small-Ta3", 128, False, False, M=384, N=384, n_items=176, T_a=3, ws="small")
    return S


_TN = None


def tn_ids():
    global _TN
    if _TN is None:
        _TN = tn_specs()
    return list(_TN)


def tn_form(cid):
    tn_ids()
    return _TN[cid][0]


def tn_make(cid):
    tn_ids()
    return tn_case(cid, *_TN[cid])


def _tn_params(kw):
    """the sizes of a case as the workspace query reads them (no pointers but colsum's presence)"""
    p = _lib.SrnTnGemmParams()
    p.n_batch, p.n_head, p.n_items, p.T_a, p.T_b = kw["n_batch"], kw["n_head"], kw["n_items"], kw["T_a"], kw["T_b"]
    p.n_shifts, p.M, p.N, p.stride = len(kw["shifts"]), kw["M"], kw["N"], kw["stride"]
    p.colsum = 16 if kw.get("colsum") is not None else None
    return p


def tn_case(cid, form, spec):
    g = spec.get
    M, N, n_items, T_a = g("M", 65), g("N", 68), g("n_items", 3), g("T_a", 16)
    stride, shifts = g("stride", 1), tuple(g("shifts", (0,)))
    T_b = g("T_b", T_a * stride)
    nb, nh, n_inner = g("n_batch", 1), g("n_head", 1), g("n_inner", 1)
    heads = bool(g("heads", False))
    rng = _Rng("tn-" + cid)
    # a: one block of T_a x lda per (zb, zh, item), NaN in its padding columns and between the blocks
    lda = _r4(M) + 4
    a_is2 = T_a * lda + 8
    a_is = (n_inner * a_is2 + 4) if n_inner > 1 else T_a * lda + 4
    n_i1 = n_items // n_inner
    a_hs = n_i1 * a_is + 4
    a_bs = nh * a_hs + 8
    a = torch.full((4 + nb * a_bs,), NAN)
    # b: T_b x ldb per item; with head slices the heads lie side by side in its rows (b_hs = N)
    ldb = (nh * N if heads else N) + 4
    b_is2 = T_b * ldb + 4
    b_is = (n_inner * b_is2 + 8) if n_inner > 1 else T_b * ldb + 8
    b_hs = N if heads else n_i1 * b_is + 4
    b_bs = (n_i1 * b_is + 4) if heads else nh * b_hs + 4
    b = torch.full((8 + nb * b_bs,), NAN)
    len_b = None
    if g("len_b"):
        pool = (0, 1, T_b, T_b + 5, T_b // 2, T_b - 1)
        len_b = torch.tensor([pool[(3 * zb + it) % len(pool)] for zb in range(nb) for it in range(n_items)], dtype=torch.int32)
    for zb in range(nb):
        for zh in range(nh):
            for it in range(n_items):
                i1, i2 = divmod(it, n_inner)
                torch.as_strided(a, (T_a, M), (lda, 1), 4 + zb * a_bs + zh * a_hs + i1 * a_is + i2 * a_is2).copy_(rng.n(T_a, M))
                live = T_b if len_b is None else min(T_b, int(len_b[zb * n_items + it]))  # rows past it stay NaN
                torch.as_strided(b, (live, N), (ldb, 1), 8 + zb * b_bs + zh * b_hs + i1 * b_is + i2 * b_is2).copy_(rng.n(live, N))
    # out: M x ldc per problem at a column offset; with head slices the heads lie side by side (out_hs = n_shifts N)
    coloff = g("coloff", 0)
    wide = len(shifts) * N
    ldc = coloff + (nh * wide if heads else wide) + 4
    out_hs = wide if heads else M * ldc + 4
    out_bs = (M * ldc + 8) if heads else nh * out_hs + 8
    out = Buf(coloff + nb * out_bs)
    kw = dict(a=(a, 4), b=(b, 8), out=(out, coloff), n_items=n_items, T_a=T_a, T_b=T_b, M=M, N=N, lda=lda, ldb=ldb, ldc=ldc,
              shifts=shifts, stride=stride, n_batch=nb, n_head=nh, a_bs=a_bs, a_hs=a_hs, a_is=a_is, b_bs=b_bs, b_hs=b_hs,
              b_is=b_is, out_bs=out_bs, out_hs=out_hs, alpha=g("alpha", 1.0), n_inner=n_inner,
              a_is2=a_is2 if n_inner > 1 else 0, b_is2=b_is2 if n_inner > 1 else 0, len_b=len_b, colsum=None,
              route=g("route", 0))
    bufs = {"out": out}
    if g("colsum"):
        bufs["colsum"] = Buf(M)
        kw["colsum"] = bufs["colsum"]
    # the workspace: exactly what the library asks for, between guards; or one of the three the launch must refuse
    need = int(library().srn_tn_gemm_workspace_bytes(ctypes.byref(_tn_params(kw))))
    mode = g("ws", "exact")
    ws = None
    if need and mode != "null":
        assert need % 16 == 0
        ws = Buf(need // 4 - (1 if mode == "small" else 0) + (1 if mode == "misaligned" else 0))
        kw["ws"] = (ws, 1) if mode == "misaligned" else ws
    outs = tn_reference(kw, bufs)
    if ws is not None:
        outs.append(Out("ws", ws, scratch=True))
    return Case(f"{form} {cid}", tuple(kw.items()), outs, kind="tn")


def tn_contract(kw):
    """float64, the header's formula: yields (zb, zh, j, val, s, dead) per problem and shift; dead: no row of a meets a
    row of b inside [0, min(T_b, len_b)) -- the columns must be exactly zero"""
    g = kw.get
    af, ao = _flat0(g("a"))
    bf, bo = _flat0(g("b"))
    M, N, T_a, T_b, st, n_inner = g("M"), g("N"), g("T_a"), g("T_b"), g("stride"), max(1, g("n_inner", 1))
    alpha = _f32(g("alpha"))
    t = torch.arange(T_a)
    for zb in range(g("n_batch")):
        for zh in range(g("n_head")):
            for j, sh in enumerate(g("shifts")):
                val = torch.zeros(M, N, dtype=torch.float64)
                s = torch.zeros(M, N, dtype=torch.float64)
                met = 0
                for it in range(g("n_items")):
                    i1, i2 = divmod(it, n_inner)
                    end = T_b if g("len_b") is None else min(T_b, int(g("len_b")[zb * g("n_items") + it]))
                    tb = t * st + sh
                    live = (tb >= 0) & (tb < end)
                    if not bool(live.any()):
                        continue
                    met += int(live.sum())
                    a0 = ao + zb * g("a_bs") + zh * g("a_hs") + i1 * g("a_is") + i2 * g("a_is2")
                    b0 = bo + zb * g("b_bs") + zh * g("b_hs") + i1 * g("b_is") + i2 * g("b_is2")
                    A = af[a0 + t[live][:, None] * g("lda") + torch.arange(M)[None]].double()
                    Bm = bf[b0 + tb[live][:, None] * g("ldb") + torch.arange(N)[None]].double()
                    val += A.t() @ Bm
                    s += A.abs().t() @ Bm.abs()
                yield zb, zh, j, val * alpha, s * abs(alpha), met == 0


def tn_reference(kw, bufs):
    g = kw.get
    out = bufs["out"]
    _, oo = _flat0(g("out"))
    M, N = g("M"), g("N")
    ref, s = torch.zeros(out.n, dtype=torch.float64), torch.zeros(out.n, dtype=torch.float64)
    written, zero = torch.zeros(out.n, dtype=torch.bool), torch.zeros(out.n, dtype=torch.bool)
    for zb, zh, j, val, sv, dead in tn_contract(kw):
        idx = (oo + zb * g("out_bs") + zh * g("out_hs") + j * N + torch.arange(M)[:, None] * g("ldc") + torch.arange(N)[None]).reshape(-1)
        assert not bool(written[idx].any()), "two elements of the reference land on one address"
        ref[idx], s[idx], written[idx], zero[idx] = val.reshape(-1), sv.reshape(-1), True, dead
    outs = [Out("out", out, ref, s=s, written=written, zero=zero)]
    if "colsum" in bufs:
        af, ao = _flat0(g("a"))
        n_inner = max(1, g("n_inner", 1))
        cs, css = torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64)
        for it in range(g("n_items")):
            i1, i2 = divmod(it, n_inner)
            A = af[ao + i1 * g("a_is") + i2 * g("a_is2") + torch.arange(g("T_a"))[:, None] * g("lda") + torch.arange(M)[None]].double()
            cs += A.sum(0)
            css += A.abs().sum(0)
        alpha = _f32(g("alpha"))
        outs.append(Out("colsum", bufs["colsum"], cs * alpha, s=css * abs(alpha)))
    return outs


def tn_kwargs(args):
    """materialized Case.args -> (TnGemmOp / emul_tn_gemm keywords, workspace or None)"""
    kw = dict(args)
    return kw, kw.pop("ws", None)


def tn_op(args, route=None):
    """ops.TnGemmOp of materialized args with the case's own workspace attached (or none: the launch falls back)"""
    kw, ws = tn_kwargs(args)
    if route is not None:
        kw["route"] = route
    op = ops.TnGemmOp(**kw)
    op._ws = ws
    if ws is None:
        op.p.ws, op.p.ws_bytes = None, 0
    else:
        t, off = ws if isinstance(ws, tuple) else (ws, 0)
        op.p.ws, op.p.ws_bytes = t.data_ptr() + 4 * off, 4 * (t.numel() - off)
    return op


def tn_route(p):
    out = (ctypes.c_int32 * 3)()
    _lib.check(library().srn_tn_gemm_route(ctypes.byref(p), out), "srn_tn_gemm_route")
    return out[0], out[1], bool(out[2])


def tn_run_emulated(args):
    from tests import _emulator
    _emulator.emul_tn_gemm(tn_kwargs(args)[0])


def tn_run_fp32(args):
    """the fp32 baseline: tests/_emulator.emul_tn_gemm's loop with fp32 products and sums"""
    kw = tn_kwargs(args)[0]
    g = kw.get
    (a, oa), (b, ob), (out, oo) = ((x[0].view(-1), x[1]) for x in (g("a"), g("b"), g("out")))
    oa, ob, oo = oa + a.storage_offset(), ob + b.storage_offset(), oo + out.storage_offset()
    M, N, T_a, T_b, stride, ninner = g("M"), g("N"), g("T_a"), g("T_b"), g("stride"), max(1, g("n_inner", 1))
    alpha = torch.tensor(g("alpha"), dtype=torch.float32)
    if g("colsum") is not None:
        cs = torch.zeros(M)
        for it in range(g("n_items")):
            i1, i2 = divmod(it, ninner)
            cs += torch.as_strided(a, (T_a, M), (g("lda"), 1), oa + i1 * g("a_is") + i2 * g("a_is2")).sum(0)
        g("colsum").view(-1)[:M] = cs * alpha
    for zb in range(g("n_batch")):
        for zh in range(g("n_head")):
            for j, sh in enumerate(g("shifts")):
                acc = torch.zeros(M, N)
                for it in range(g("n_items")):
                    i1, i2 = divmod(it, ninner)
                    a0 = oa + zb * g("a_bs") + zh * g("a_hs") + i1 * g("a_is") + i2 * g("a_is2")
                    b0 = ob + zb * g("b_bs") + zh * g("b_hs") + i1 * g("b_is") + i2 * g("b_is2")
                    am = torch.as_strided(a, (T_a, M), (g("lda"), 1), a0)
                    tb = torch.arange(T_a) * stride + sh
                    end = T_b if g("len_b") is None else min(T_b, int(g("len_b").view(-1)[zb * g("n_items") + it]))
                    ok = (tb >= 0) & (tb < end)
                    rows = torch.as_strided(b, (T_b, N), (g("ldb"), 1), b0)[tb.clamp(0, T_b - 1)]
                    acc += am.t() @ torch.where(ok[:, None], rows, torch.zeros(()))
                torch.as_strided(out, (M, N), (g("ldc"), 1), oo + zb * g("out_bs") + zh * g("out_hs") + j * N).copy_(acc * alpha)


def tn_rejects():
    """[(id, spec changes, params edit, message)] over one valid base call"""
    sa = lambda k, v: (lambda p: setattr(p, k, v))
    return [
        ("N%4", {}, sa("N", 66), "multiples of 4 floats"),
        ("lda-short", {}, sa("lda", 64), "multiples of 4 floats"),
        ("ldc-short", {}, sa("ldc", 64), "ldc 64 < n_shifts"),
        ("n_shifts-0", {}, sa("n_shifts", 0), "n_shifts 0"),
        ("n_shifts-17", {}, sa("n_shifts", 17), "n_shifts 17"),
        ("stride-0", {}, sa("stride", 0), "stride 0"),
        ("a_is%4", {}, lambda p: setattr(p, "a_is", p.a_is + 2), "multiples of 4 floats"),
        ("b-misaligned", {}, lambda p: setattr(p, "b", p.b + 4), "16-byte aligned"),
        ("colsum-two-problems", dict(colsum=True, M=68), sa("n_head", 2), "colsum needs one problem"),
        ("colsum-M%4", dict(colsum=True), None, "colsum needs one problem"),
        ("lenb-inner", dict(len_b=True, n_inner=1, n_items=4), sa("n_inner", 2), "len_b is per item"),
    ]


def tn_reject_case(rid):
    _, ch, edit, msg = next(r for r in tn_rejects() if r[0] == rid)
    case = tn_case("reject-" + rid, "reject", dict(dict(n_items=3, T_a=16, shifts=(-1, 0)), **ch))
    for o in case.outs:  # nothing may be written
        if not o.scratch:
            o.written = torch.zeros(o.buf.n, dtype=torch.bool)
            o.zero = None
    case.error = msg
    return case, edit


# ====================================================================================================== the list
def all_ids():
    """[(family, form, case id)]"""
    ids = [("resunit", f, vid) for f in RU_FORMS for vid, _ in ru_variants(f)]
    return ids + [("tn", tn_form(cid), cid) for cid in tn_ids()]


def make(family, form, cid):
    if family == "tn":
        return tn_make(cid)
    return ru_case(form, cid, dict(ru_variants(form))[cid])


def tol_row(family, form, cid):
    if family == "tn":
        return "tn"
    spec = dict(ru_variants(form))[cid]
    prec = spec.get("precision", RU_FORMS[form][3])
    return {FP32: "resunit-fp32", X3: "resunit-bf16x3", X6: "resunit-bf16x6"}[prec]


def tol_for(family, form, cid):
    return CASE_TOL.get((form, cid), TOL[tol_row(family, form, cid)])[1]


def baseline_error(family, form, cid, which):
    """the error of a restatement on one case: which in {"emul", "fp32", "bf16x3"}"""
    case = make(family, form, cid)
    args, bufs = materialize(case)
    if family == "tn":
        (tn_run_emulated if which == "emul" else tn_run_fp32)(args)
    else:
        (ru_run_bf16x3 if which == "bf16x3" else ru_run_emulated)(args)
    return check_outputs(case, bufs)[0]


def _main():
    worst, where = {"tn": 0.0, "resunit-fp32": 0.0, "resunit-bf16x3": 0.0}, {}
    for family, form, cid in all_ids():
        rows = ["tn"] if family == "tn" else ["resunit-fp32"] + (["resunit-bf16x3"] if RU_FORMS[form][3] == X3 else [])
        for row in rows:
            e = baseline_error(family, form, cid, {"tn": "fp32", "resunit-fp32": "emul", "resunit-bf16x3": "bf16x3"}[row])
            if e > worst[row]:
                worst[row], where[row] = e, (form, cid)
    for row, e in worst.items():
        print(f"TOL    {row!r}: ({e:.3e}, {_round_up(max(4 * e, FLOOR)):.1e}),   # worst at {where.get(row)}", flush=True)
    n_ru = sum(1 for f, _, _ in all_ids() if f == "resunit")
    print(f"cases: {len(all_ids())} ({n_ru} residual unit over {len(RU_FORMS)} forms, {len(tn_ids())} srn_tn_gemm over "
          f"{len(TN_FORMS)} forms)")


if __name__ == "__main__":
    _main()
