"""Case generators and float64 references for every kernel form behind srn_conv_gemm (conv_gemm.hip, conv_fast.hip,
conv_f32.hip, conv_halo.hip, conv_strip.hip, conv_splitk.hip).

Shared by tests/test_convsweep_emulated.py (CPU: the emulator against these references, and the route of every case on
the cross-compiled library) and tests/test_hip_convsweep.py (MI355X: the kernels against the same references).  No GPU
is touched here.  Buf / Out / Case / materialize / check_outputs are those of tests/_rowop_cases.py.

A case is the keyword dict of one ``ops.ConvOp`` (``Case.args`` holds its items; ``kwargs`` turns materialized args
back into the dict).  It forces ``tile``, ``route`` and ``precision`` so that it reaches ONE kernel form (forms() below:
the rows of the library's own list, srn_conv_gemm_forms, told apart further by weight planes / operands split in the
loop and by ROUTE_FAST_FP32; the split-K slices of both families are forms of their own).  Every tensor the call writes
(out, out_tr, gn_partials, in-place res / res2) is a Buf between guard bands; ld padding columns, rows not congruent to
out_t_off mod out_t_stride, out_tr columns at or past T_out and the columns of `out` at or past out_tr_col0 start as
sentinels (or, in place, as their input values) and must come back bit for bit.  Rows at or past len_out must be exactly
zero where no residual is added to them.

The reference is float64 torch from the same fp32 inputs, written independently of tests/_emulator.emul_conv: gather of
the tap rows, length mask, reflection (mode 1: at the tensor's ends; mode 2: at 0 and at the item's own end), prologue,
A64 @ W64, then the epilogue in the header's order (alpha, bias, GEGLU, len_out mask, residual, second residual, post
op); GroupNorm partials are fp64 sums of the reference's stored values over 32 x 32 tiles.
Reflection is ONE mirror per end, as the header's formula and the emulator both have it: with reflect = 2 and len_in = 2
under a span-6 table (taps -3 .. 3), tap offsets whose mirror image still lies outside [0, len_in) read as zero; the
validation only bounds the taps by T_in.  The reference states that rule and the sweep asserts it.

Pass criterion, per element:   |got - ref| <= tol (|ref| + s)
with s the size of the terms that were summed: |alpha| (|A| @ |W|) + |bias| + |res| (RES_AXPY: |res| + |beta| times the
former) + |res2|; divided by post_div under POST_DIV (POST_GELU: times 1.13, the bound of |gelu'|; the other post ops are
1-Lipschitz); through GEGLU's v gelu(g): (|v| + s_v) |gelu(g)| + 1.13 |v| (|g| + s_g); a GroupNorm partial takes the sum
of s over its tile (times 2 |v| for the square sum).

tol is not chosen: 4 x the worst error over this same sweep, under this same formula, of a CPU restatement in the
arithmetic of the mode, rounded up to two digits, floor 8 * 2^-24 (`python -m tests._conv_cases` prints the column again;
test_convsweep_emulated.py holds the restatement to tol / 4):

  precision   baseline    tol        restatement
  fp32        2.775e-07   1.2e-06    tests/_emulator.emul_conv (fp32 torch)
  bf16x6      2.775e-07   1.2e-06    the fp32 row: DESIGN.md holds bf16x6 "to the fp32 tolerances", the claim under test
  bf16x3      1.014e-05   4.1e-05    both operands split as split4 does (hi = bf16(x), lo = bf16(x - hi)), the kernels'
                                     three products A_lo W_hi + A_hi W_lo + A_hi W_hi (conv_fast.hip, SRN_MFMA_GROUP)
                                     accumulated in fp32
No case needs a tolerance of its own (CASE_TOL is empty).

What a family does not take is left out of its list, nothing else: the halo kernel has no k1 / stride 2 / reflection /
GEGLU; the strip kernel takes C_in and N in {32, 64} only, one column tile, no heads, no concat; n-major B is k1 with
N % 4 == 0 (GEGLU included: N = 64, 192); the split-K forms need N % 4 == 0 and no GEGLU / transposed tail; SiLU / Mish run on the generic 64 x 64
form and on conv_fast.hip's run-time-activation instantiation; GEGLU needs a 64-column wave tile (ids 1, 2, 3, 9).
T_out = 64 (with and without strided rows) puts the tensor's last row into an interior sub-tile: conv_f32.hip stores those
without predicates, so that is where its store descriptor's byte count is on its own -- one row short there fails these
cases on every f32 tile (one row long changes nothing: the kernel never issues a store past the last row).
"""
import math

import torch
import torch.nn.functional as F

from serenade_amd import _lib
from tests._rowop_cases import (FLOOR, Buf, Case, Out, _bits, _Rng, _round_up, check_outputs,  # noqa: F401
                                materialize)

FP32, X3, X6 = _lib.PREC_FP32, _lib.PREC_BF16X3, _lib.PREC_BF16X6
PREC_NAME = {FP32: "fp32", X3: "bf16x3", X6: "bf16x6"}

# precision -> (measured baseline of the restatement, tol); filled from `python -m tests._conv_cases`
TOL = {
    "fp32": (2.775e-07, 1.2e-06),
    "bf16x6": (2.775e-07, 1.2e-06),
    "bf16x3": (1.014e-05, 4.1e-05),
}
CASE_TOL = {}  # (form, case id) -> (baseline, tolerance): none needed


class Form:
    """one kernel form: what the route must answer (family, tile, K slices > 1), how a case forces it, and the tile
    geometry of its row in the library's list"""

    def __init__(self, row, family, tile, prec, planes, nmajor, splitk):
        self.family, self.tile, self.prec, self.planes, self.nmajor, self.splitk = family, tile, prec, planes, nmajor, splitk
        self.bm, self.bn, self.wn = row.bm, row.bn, row.wn
        p = PREC_NAME[prec]
        self.route = {"generic": _lib.ROUTE_GENERIC, "f32": _lib.ROUTE_AUTO, "halo": _lib.ROUTE_HALO, "strip": _lib.ROUTE_STRIP,
                      "fast": _lib.ROUTE_FAST_FP32 if prec == FP32 else _lib.ROUTE_TILED}[family]
        self.name = {"generic": f"generic{tile}-{'nmaj-' if nmajor else ''}{p}", "f32": f"f32-{tile}", "halo": f"halo{tile}",
                     "fast": f"fast{tile}-{p}" + ("" if prec == FP32 else "-planes" if planes else "-loop"),
                     "strip": "strip"}[family]
        if splitk:
            self.name = "splitk-f32" if family == "f32" else f"splitk-fast-{p}"

    @property
    def key(self):
        """what the completeness check counts: (family, tile, precision, weight planes, n-major, split-K)"""
        return (self.family, self.tile, self.prec, self.planes, self.nmajor, self.splitk)


def _keys(row):
    """the Form.key s the sweep makes of one row of the library's list: conv_fast.hip's split-bf16 forms with weight
    planes and with operands split in the loop are forms of their own (the strip kernel has planes only), and so are
    the K slices of a row that takes them (with planes, where the arithmetic has them)"""
    from tests.test_conv_route import FAMILY
    fam = FAMILY[row.family]
    split = fam == "fast" and row.precision != FP32
    for planes in ((True, False) if split else (fam == "strip",)):
        yield (fam, row.tile, row.precision, planes, bool(row.nmajor), False)
    if row.kslices:
        yield (fam, row.tile, row.precision, split, bool(row.nmajor), True)


def _forms():
    from tests.test_conv_route import library_forms
    # generic: by tile, the n-major form after the k-major one; conv_fast.hip: by arithmetic; the K slices last
    rows = sorted(library_forms(), key=lambda r: (r.family, r.precision if r.family == _lib.FAMILY_FAST else 0, r.tile,
                                                  r.precision, r.nmajor))
    keyed = [(r, k) for r in rows for k in _keys(r)]
    return [Form(r, *k) for splitk in (False, True) for r, k in keyed if k[5] == splitk]


_FORMS = None


def forms():
    global _FORMS
    if _FORMS is None:
        _FORMS = {f.name: f for f in _forms()}
    return _FORMS


def existing_forms():
    """the set of Form.key a kernel exists for, from the library's list and the distinctions of _keys: what the sweep
    must reach, no more and no less"""
    from tests.test_conv_route import library_forms
    return {k for r in library_forms() for k in _keys(r)}


# ------------------------------------------------------------------------------------------------------- the matrix
TAPS = {
    "k1": (0,), "k3": (-1, 0, 1), "k5": (-2, -1, 0, 1, 2), "k7": (-3, -2, -1, 0, 1, 2, 3),
    "k11d5": tuple(5 * (i - 5) for i in range(11)),  # span 50, just under SRN_HALO_MAX
    "onesided": (0, 2, 4, 6),
    "k11": tuple(i - 5 for i in range(11)),
}
EPILOGUES = ("res-add", "res2", "res-res2", "axpy", "mean", "relu", "leaky", "tanh", "gelu", "ots3-0", "ots3-2", "gn")


def variants(f):
    """[(case id, spec)] of one form: every spec changes the base shape along one axis of the matrix"""
    V = []

    def add(vid, **kw):
        V.append((vid, kw))

    bm, bn = f.bm, f.bn
    strip, halo, gen = f.family == "strip", f.family == "halo", f.family == "generic"
    if f.splitk:
        # steps = n_taps * C_in / 32 in {24, 25, 33}: even and uneven slices, slices that start mid-tap (k3 x 256: 4
        # steps per slice, 8 per tap) and inside the in1 segment of a concat (k11 x (32 | 64): 5 steps per slice)
        depth = {24: dict(taps="k3", C_in=256), 25: dict(taps="k5", C_in=160), 33: dict(taps="k11", C_in=96, C_in0=32)}
        for steps, d in depth.items():
            for T in (1, 70):
                for N in (4, 160):
                    add(f"steps{steps}-T{T}-N{N}", T_out=T, N=N, **d)
        for ep in EPILOGUES + ("lout",):
            kw = dict(T_out=70, N=160, epi=ep, **depth[24])
            if ep == "lout":
                kw.update(epi=None, len_out=(1, 70))
            add(f"steps24-T70-N160-{ep}", **kw)
        return V
    n_free = not f.nmajor  # n-major B and the split-K forms need N % 4 == 0
    Ns = ([32, 64] if strip else sorted({4, 36, bn - 4, bn + 4} | ({1, 5} if n_free else set())))
    Cs = [32, 64] if strip else ([4, 20, 36] if gen else [32, 96])
    taps_ok = ["k1"] if f.nmajor else (["k3", "k11d5", "onesided"] if halo else ["k1", "k3", "k11d5", "onesided"])
    # rows: 1, 31 / 33 around the 32-row sub-tile, bm -+ 1 around the tile; 64: the last row of the tensor lies in an
    # interior sub-tile, the only place where conv_f32.hip's store descriptor (no predicates) decides what is written
    for T in sorted({1, 31, 33, 64, bm - 1, bm + 1}):
        add(f"T{T}", T_out=T)
    add("T64-ots3-2", T_out=64, epi="ots3-2")
    # band walk (conv_common.h's tile_coords, conv_f32.hip's switch (gm)): m_tiles % 8 in {1, 3, 5, 6, 7}, two n tiles,
    # z >= 2 and a block count that is no multiple of 8 (the XCD map's remainder path)
    for mt in (9, 11, 5, 6, 7):
        nt = 1 if strip else 2
        B = 2 if (2 * mt * nt) % 8 else 3
        add(f"band{mt}", T_out=(mt - 1) * bm + 1, N=(Ns[0] if strip else bn + 4), B=B)
    for N in Ns:
        add(f"N{N}", N=N)
    for C in Cs:
        add(f"C{C}", C_in=C)
    for tp in taps_ok:
        add(tp, taps=tp)
    if not f.nmajor and not halo and not strip:
        add("stride2", taps="k3", stride=2)
        add("reflect1", taps="k7", reflect=1)
        # reflect = 2: the mirror sits at each item's own end; len_in = 2 under the span-6 table: see the docstring
        add("reflect2", taps="k7", reflect=2, B=3, T_out=40, len_in=(40, 33, 2))
    # lengths
    add("lin", B=4, T_out=40, len_in=(1, 31, 33, 40))
    add("lout", B=4, T_out=40, len_out=(1, 31, 33, 40))
    add("lin-lout-gn", B=4, T_out=40, N=64, len_in=(31, 1, 40, 33), len_out=(1, 31, 33, 40), epi="gn")
    # operands
    if not strip:
        add("concat32", C_in=96, C_in0=32)
        add("concat64", C_in=96, C_in0=64)
        add("heads", nh=2, epi="res-add")
        if not f.planes:
            add("wbatch", wbatch=True)
    if gen and f.nmajor:
        add("cw", C_in=36, C_w=20)  # the P.V shape: fewer live k on the weight side
    add("alpha", alpha=0.37)
    # prologue
    add("leaky0.1", pro_act=_lib.ACT_LEAKY, pro_slope=0.1)
    add("leaky1.0", pro_act=_lib.ACT_LEAKY, pro_slope=1.0)
    if (gen and f.tile == 4) or f.family == "fast":  # run-time activation: the generic 64 x 64 form, conv_fast.hip's ACT = -1
        add("silu", pro_act=_lib.ACT_SILU)
        add("mish", pro_act=_lib.ACT_MISH)
    # epilogue
    for ep in EPILOGUES:
        kw = dict(epi=ep)
        if ep == "gn":
            kw.update(T_out=40, N=64)
        add(ep, **kw)
    if f.wn >= 64 and not halo and not strip:
        add("geglu64", N=64, geglu=True)
        add("geglu192", N=192, geglu=True)
    add("tr1-col0", T_out=33, N=(64 if strip else 36), tr_col0=0)
    add("tr3-col32", T_out=35, N=(64 if strip else 68), tr_col0=32)
    return V


_LIST = None


def _list():
    global _LIST
    if _LIST is None:
        _LIST = {}
        for f in forms().values():
            for vid, spec in variants(f):
                assert (f.name, vid) not in _LIST
                _LIST[(f.name, vid)] = spec
    return _LIST


def all_ids():
    return list(_list())


def make(form, vid):
    return build_case(forms()[form], vid, _list()[(form, vid)])


def tol_for(form, vid):
    return CASE_TOL.get((form, vid), TOL[PREC_NAME[forms()[form].prec]])[1]


def _r4(n):
    return (n + 3) // 4 * 4


def build_case(f, vid, spec):
    """the ConvOp keywords of one case, its Bufs and their float64 references"""
    g = spec.get
    strip, gen = f.family == "strip", f.family == "generic"
    B, nh = g("B", 2), g("nh", 1)
    taps = TAPS[g("taps", "k1" if f.nmajor else "k3")]
    stride = g("stride", 1)
    T_out = g("T_out", 33)
    N = g("N", 32 if strip else 36)
    C_in = g("C_in", 20 if gen else 32)
    C_in0 = g("C_in0", C_in)
    geglu = bool(g("geglu", False))
    N_out = N // 2 if geglu else N
    if stride == 2:
        T_in = 2 * T_out - 1  # odd: the last output row's right tap is padding
    elif min(taps) >= 0:
        T_in = T_out + max(taps)
    else:
        T_in = T_out
    rng = _Rng(f"conv-{f.name}-{vid}")
    kw = dict(n_batch=B, n_head=nh, T_in=T_in, T_out=T_out, C_in=C_in, N=N, taps=taps, in_stride=stride,
              tile=0 if f.splitk else f.tile, route=f.route, precision=f.prec)
    # inputs: in0 / in1 with ld = width + 4 behind an offset of 4 elements; heads side by side in the channel dim
    ld0 = nh * C_in0 + 4
    in0 = rng.n(4 + B * T_in * ld0)
    kw.update(in0=(in0, 4), in0_bs=T_in * ld0, in0_hs=C_in0 if nh > 1 else 0, ld_in0=ld0)
    if C_in0 < C_in:
        c1 = C_in - C_in0
        kw.update(C_in0=C_in0, in1=(rng.n(8 + B * T_in * (c1 + 4)), 8), in1_bs=T_in * (c1 + 4), ld_in1=c1 + 4)
    # weights: planes forms take a plain tensor (ConvOp splits it once); every other form an (tensor, offset) pair;
    # operands split in the loop: one B per batch item (w_bs != 0)
    K = len(taps) * C_in
    scale = 1.0 / math.sqrt(K)
    wbatch = g("wbatch", False) or (f.family == "fast" and f.prec != FP32 and not f.planes)
    C_w = g("C_w", 0)
    if f.nmajor:
        rows_w, ldw = (C_w or C_in), N + 4
        kw.update(w_nmajor=True)
    else:
        rows_w, ldw = N, K + 4
    per = rows_w * ldw
    whead = nh > 1 and not f.planes  # weight planes are shared by every (batch, head)
    nw = (B if wbatch else 1) * (nh if whead else 1)
    wt = rng.n(nw * per) * scale
    if f.planes:
        kw.update(w=wt)
    else:
        wt = torch.cat([torch.zeros(4), wt])
        kw.update(w=(wt, 4))
    kw.update(ldw=ldw, w_hs=per if whead else 0, w_bs=per * (nh if whead else 1) if wbatch else 0)
    if C_w:
        kw.update(C_w=C_w)
    kw.update(bias=rng.n(N))
    if g("alpha") is not None:
        kw.update(alpha=g("alpha"))
    if g("pro_act"):
        kw.update(pro_act=g("pro_act"), pro_slope=g("pro_slope", 0.0))
    if g("reflect"):
        kw.update(reflect=g("reflect"))
    if g("len_in"):
        kw.update(len_in=torch.tensor(g("len_in"), dtype=torch.int32))
    if g("len_out"):
        kw.update(len_out=torch.tensor(g("len_out"), dtype=torch.int32))
    if geglu:
        kw.update(geglu=True)
    # outputs: ld_out = width + 3 at an odd offset; residuals with ld + 5 / + 1
    epi = g("epi")
    ots, oto = (3, int(epi[-1])) if epi in ("ots3-0", "ots3-2") else (1, 0)
    rows = (T_out - 1) * ots + oto + 1 + (1 if ots > 1 else 0)  # one more row behind the last strided one
    W_out = nh * N_out
    ld_out, ld_res, ld_res2 = W_out + 3, W_out + 5, W_out + 1
    o_off = 1
    inplace = epi in ("axpy", "mean")  # res (axpy) / res2 (mean) ARE out: same pointer, same strides
    n_out = o_off + B * rows * ld_out
    out = Buf(n_out, init=rng.n(n_out) if inplace else None)
    kw.update(out=(out, o_off), out_bs=rows * ld_out, out_hs=N_out if nh > 1 else 0, ld_out=ld_out)
    if ots > 1:
        kw.update(out_t_stride=ots, out_t_off=oto)
    bufs = {"out": out}
    if epi in ("res-add", "res-res2", "mean"):
        kw.update(res=(rng.n(3 + B * rows * ld_res), 3), res_mode=_lib.RES_ADD, res_bs=rows * ld_res,
                  res_hs=N_out if nh > 1 else 0, ld_res=ld_res)
    if epi == "axpy":
        kw.update(res=(out, o_off), res_mode=_lib.RES_AXPY, beta=0.25, res_bs=rows * ld_out, ld_res=ld_out)
    if epi == "mean":
        kw.update(res2=(out, o_off), res2_bs=rows * ld_out, ld_res2=ld_out, post=_lib.POST_DIV, post_div=3.0)
    if epi in ("res2", "res-res2"):  # a second residual of its own: pointer offset, ld and batch stride unlike out's
        bs2 = rows * ld_res2 + 2
        kw.update(res2=(rng.n(7 + B * bs2), 7), res2_bs=bs2, ld_res2=ld_res2)
    post = {"relu": _lib.POST_RELU, "leaky": _lib.POST_LEAKY, "tanh": _lib.POST_TANH, "gelu": _lib.POST_GELU}.get(epi)
    if post:
        kw.update(post=post, post_div=0.2)
    if epi == "gn":
        gn = Buf(4 + B * ((T_out + 31) // 32) * (N // 32) * 2)
        kw.update(gn_partials=(gn, 4))
        bufs["gn_partials"] = gn
    if g("tr_col0") is not None:
        ld_tr = _r4(T_out) + 4
        tr_bs = (N - g("tr_col0")) * ld_tr + 8
        tr = Buf(4 + B * tr_bs)
        kw.update(out_tr=(tr, 4), out_tr_bs=tr_bs, ld_out_tr=ld_tr, out_tr_col0=g("tr_col0"))
        bufs["out_tr"] = tr
    outs = reference(kw, bufs)
    return Case(f"{f.name} {vid}", tuple(kw.items()), outs, kind="conv")


def kwargs(args):
    """materialized Case.args -> the keyword dict of ops.ConvOp / emul_conv"""
    return dict(args)


# ---------------------------------------------------------------------------------------------------- the reference
def _flat0(x):
    """(flat fp32 tensor as the call finds it, element offset) of a tensor, Buf or (tensor | Buf, offset) pair"""
    off = 0
    if isinstance(x, tuple):
        x, off = x
    return (x.initial() if isinstance(x, Buf) else x.reshape(-1)), int(off)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _act(a, act, slope):
    if act == _lib.ACT_LEAKY:
        return torch.where(a > 0, a, a * slope)
    if act == _lib.ACT_SILU:
        return a * torch.sigmoid(a)
    if act == _lib.ACT_MISH:
        return a * torch.tanh(F.softplus(a))
    return a


def contract(kw, dt=torch.float64, mm=None):
    """the contraction and its epilogue in dtype dt (float64: the reference), one entry per (zb, zh):
    (zb, zh, val, s) with val / s the T_out x N_out stored values and the size of their summed terms.  mm(A, W) -> A W^T
    replaces the product (the split-bf16 restatement); s is only formed in float64."""
    g = kw.get
    nb, nh = g("n_batch"), g("n_head", 1)
    T_in, T_out, C_in, N = g("T_in"), g("T_out"), g("C_in"), g("N")
    C_in0 = g("C_in0", 0) or C_in
    C_w = g("C_w", 0) or C_in
    taps = list(g("taps", (0,)))
    st = g("in_stride", 1)
    geglu = bool(g("geglu", False))
    refl = int(g("reflect", 0))
    in0, o0 = _flat0(g("in0"))
    in1, o1 = _flat0(g("in1")) if g("in1") is not None else (None, 0)
    w, ow = _flat0(g("w"))
    bias = g("bias").to(dt) if g("bias") is not None else torch.zeros(N, dtype=dt)
    alpha, beta = float(torch.tensor(g("alpha", 1.0), dtype=torch.float32)), float(torch.tensor(g("beta", 0.0), dtype=torch.float32))
    post, pdiv = g("post", 0), float(torch.tensor(g("post_div", 1.0), dtype=torch.float32))
    slope = float(torch.tensor(g("pro_slope", 0.0), dtype=torch.float32))
    ots, oto = g("out_t_stride", 1), g("out_t_off", 0)
    t = torch.arange(T_out)
    want_s = dt == torch.float64
    for zb in range(nb):
        li = T_in if g("len_in") is None else min(int(g("len_in")[zb]), T_in)
        lo = T_out if g("len_out") is None else min(int(g("len_out")[zb]), T_out)
        for zh in range(nh):
            A = torch.zeros(T_out, len(taps), C_in, dtype=dt)
            for j, off in enumerate(taps):
                ti = t * st + off
                if refl:  # one mirror at 0 and one at the end: the tensor's (1) or the item's own (2)
                    end = li if refl == 2 else T_in
                    ti = torch.where(ti < 0, -ti, ti)
                    ti = torch.where(ti >= end, 2 * (end - 1) - ti, ti)
                live = (ti >= 0) & (ti < li)
                rows_ = ti[live]
                base = o0 + zb * g("in0_bs", 0) + zh * g("in0_hs", 0)
                A[live, j, :C_in0] = in0[base + rows_[:, None] * g("ld_in0") + torch.arange(C_in0)[None]].to(dt)
                if C_in0 < C_in:
                    base = o1 + zb * g("in1_bs", 0)
                    A[live, j, C_in0:] = in1[base + rows_[:, None] * g("ld_in1") + torch.arange(C_in - C_in0)[None]].to(dt)
            A = _act(A, g("pro_act", 0), slope).reshape(T_out, -1)
            wb = ow + zb * g("w_bs", 0) + zh * g("w_hs", 0)
            if g("w_nmajor", False):
                Wm = torch.zeros(N, C_in, dtype=dt)
                Wm[:, :C_w] = w[wb + torch.arange(C_w)[None] * g("ldw") + torch.arange(N)[:, None]].to(dt)
            else:
                Wm = w[wb + torch.arange(N)[:, None] * g("ldw") + torch.arange(len(taps) * C_in)[None]].to(dt)
                Wm = Wm.reshape(N, len(taps), C_in).clone()
                Wm[:, :, C_w:] = 0
                Wm = Wm.reshape(N, -1)
            acc = A @ Wm.t() if mm is None else mm(A, Wm)
            val = acc * alpha + bias
            s = abs(alpha) * (A.abs() @ Wm.abs().t()) + bias.abs() if want_s else None
            if geglu:
                v4 = val.reshape(T_out, N // 64, 2, 32)
                v, gt = v4[:, :, 0].reshape(T_out, -1), v4[:, :, 1].reshape(T_out, -1)
                val = v * _gelu(gt)
                if want_s:
                    s4 = s.reshape(T_out, N // 64, 2, 32)
                    sv, sg = s4[:, :, 0].reshape(T_out, -1), s4[:, :, 1].reshape(T_out, -1)
                    s = (v.abs() + sv) * _gelu(gt).abs() + 1.13 * v.abs() * (gt.abs() + sg)
            val = val.clone()
            val[lo:] = 0
            if want_s:
                s[lo:] = 0
            n_out = val.shape[1]
            orow = (t * ots + oto)[:, None]
            cols = torch.arange(n_out)[None]
            if g("res_mode", 0):
                res, o_r = _flat0(g("res"))
                r = res[o_r + zb * g("res_bs", 0) + zh * g("res_hs", 0) + orow * g("ld_res") + cols].to(dt)
                if g("res_mode") == _lib.RES_ADD:
                    val = val + r
                    s = s + r.abs() if want_s else None
                else:
                    val = r + beta * val
                    s = r.abs() + abs(beta) * s if want_s else None
            if g("res2") is not None:
                res2, o_q = _flat0(g("res2"))
                q = res2[o_q + zb * g("res2_bs", 0) + orow * g("ld_res2") + cols].to(dt)
                val = val + q
                s = s + q.abs() if want_s else None
            if post == _lib.POST_DIV:
                val = val / pdiv
                s = s / abs(pdiv) if want_s else None
            elif post == _lib.POST_TANH:
                val = torch.tanh(val)
            elif post == _lib.POST_RELU:
                val = torch.relu(val)
            elif post == _lib.POST_LEAKY:
                val = torch.where(val > 0, val, val * pdiv)
            elif post == _lib.POST_GELU:
                val = _gelu(val)
                s = 1.13 * s if want_s else None
            yield zb, zh, lo, val, s


def _targets(kw, zb, zh, n_out):
    """flat element indices of one (zb, zh) tile of stored values: (into out or None, into out_tr or None), with the
    column split at out_tr_col0"""
    g = kw.get
    T_out = g("T_out")
    t = torch.arange(T_out)
    cols = torch.arange(n_out)[None]
    _, oo = _flat0(g("out"))
    oidx = oo + zb * g("out_bs", 0) + zh * g("out_hs", 0) + (t * g("out_t_stride", 1) + g("out_t_off", 0))[:, None] * g("ld_out") + cols
    if g("out_tr") is None:
        return oidx, None, n_out
    c0 = g("out_tr_col0", 0)
    _, ot = _flat0(g("out_tr"))
    tidx = ot + zb * g("out_tr_bs", 0) + (cols[:, c0:] - c0) * g("ld_out_tr") + t[:, None]
    return oidx[:, :c0], tidx, c0


def reference(kw, bufs):
    """[Out] of the Bufs of one case"""
    acc = {}
    for name, b in bufs.items():
        acc[name] = dict(ref=torch.zeros(b.n, dtype=torch.float64), s=torch.zeros(b.n, dtype=torch.float64),
                         written=torch.zeros(b.n, dtype=torch.bool), zero=torch.zeros(b.n, dtype=torch.bool))

    def put(name, idx, val, s, zero=None):
        a = acc[name]
        idx = idx.reshape(-1)
        assert not bool(a["written"][idx].any()), "two elements of the reference land on one address"
        a["ref"][idx], a["s"][idx], a["written"][idx] = val.reshape(-1), s.reshape(-1), True
        if zero is not None:
            a["zero"][idx] = zero.reshape(-1)

    g = kw.get
    T_out, N = g("T_out"), g("N")
    plain_rows = not g("res_mode", 0) and g("res2") is None  # masked rows are exactly 0 where nothing is added to them
    mt, nt = (T_out + 31) // 32, N // 32
    for zb, zh, lo, val, s in contract(kw):
        oidx, tidx, c0 = _targets(kw, zb, zh, val.shape[1])
        zero = (torch.arange(T_out)[:, None] >= lo).expand_as(val) if plain_rows else None
        if oidx.numel():
            put("out", oidx, val[:, :c0], s[:, :c0], None if zero is None else zero[:, :c0])
        if tidx is not None:
            put("out_tr", tidx, val[:, c0:], s[:, c0:], None if zero is None else zero[:, c0:])
        if "gn_partials" in bufs:
            pad = torch.zeros(2, mt * 32, nt * 32, dtype=torch.float64)
            pad_s = torch.zeros_like(pad)
            pad[0, :T_out, :N], pad[1, :T_out, :N] = val, val * val
            pad_s[0, :T_out, :N], pad_s[1, :T_out, :N] = s, 2 * val.abs() * s
            part = pad.reshape(2, mt, 32, nt, 32).sum(dim=(2, 4)).permute(1, 2, 0)
            part_s = pad_s.reshape(2, mt, 32, nt, 32).sum(dim=(2, 4)).permute(1, 2, 0)
            _, og = _flat0(g("gn_partials"))
            put("gn_partials", og + zb * mt * nt * 2 + torch.arange(mt * nt * 2), part, part_s)
    return [Out(name, bufs[name], a["ref"], s=a["s"], written=a["written"], zero=a["zero"]) for name, a in acc.items()]


# ----------------------------------------------------------------------------------------------------- restatements
def run_emulated(case, args):
    """the call through the CPU executable spec (fp32 torch): the fp32 baseline"""
    from tests import _emulator
    _emulator.emul_conv(kwargs(args))


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def mm_bf16x3(A, W):
    """split4 on both operands (hi = bf16(x), lo = bf16(x - hi)) and the kernels' three products, fp32 accumulate"""
    ah, wh = _bf(A), _bf(W)
    al, wl = _bf(A - ah), _bf(W - wh)
    return (al @ wh.t() + ah @ wl.t()) + ah @ wh.t()


def run_bf16x3(case, args):
    """the bf16x3 baseline: the contraction restated in fp32 with mm_bf16x3, stored like the kernels store it"""
    kw = kwargs(args)
    # in-place residuals are read from the buffers as the call finds them: evaluate everything before storing
    todo = [(zb, zh, val) for zb, zh, _, val, _ in contract(kw, torch.float32, mm_bf16x3)]
    T_out, N = kw["T_out"], kw["N"]
    mt, nt = (T_out + 31) // 32, N // 32
    for zb, zh, val in todo:
        oidx, tidx, c0 = _targets(kw, zb, zh, val.shape[1])
        if oidx.numel():
            kw["out"][0].view(-1)[oidx] = val[:, :c0]
        if tidx is not None:
            kw["out_tr"][0].view(-1)[tidx] = val[:, c0:]
        if kw.get("gn_partials") is not None:
            pad = torch.zeros(mt * 32, nt * 32)
            pad[:T_out, :N] = val
            tiles = pad.reshape(mt, 32, nt, 32)
            part = torch.stack([tiles.sum(dim=(1, 3)), (tiles ** 2).sum(dim=(1, 3))], dim=-1).reshape(-1)
            gp, og = kw["gn_partials"]
            gp.view(-1)[og + zb * part.numel():og + (zb + 1) * part.numel()] = part


def baseline_error(form, vid, which):
    case = make(form, vid)
    args, bufs = materialize(case)
    (run_emulated if which == "fp32" else run_bf16x3)(case, args)
    return check_outputs(case, bufs)[0]


# -------------------------------------------------------------------------------------------------------- rejects
def rejects():
    """[(id, keyword changes or a params edit, message)] over one valid base call: each must return the error and write
    nothing.  `edit` runs on the filled SrnConvParams (what ops.ConvOp cannot express)."""
    return [
        ("C_in%4", dict(C_in=30), None, "C_in"),
        ("in0-misaligned", dict(in0_off=5), None, "in0 must be 16-byte aligned"),
        ("n_taps-17", {}, lambda p: setattr(p, "n_taps", _lib.SRN_MAX_TAPS + 1), "n_taps"),
        ("geglu-N%64", dict(N=96, geglu=True), None, "GEGLU needs N % 64"),
        ("gn-N%32", dict(N=36, gn=True), None, "gn_partials needs N % 32"),
        ("reflect-wider", dict(T=8, taps=TAPS["k11d5"], reflect=1), None, "reflect pad wider"),
        ("tr-col0%32", dict(N=64, tr_col0=16), None, "out_tr needs"),
        ("nmajor-taps", dict(w_nmajor=True, taps=TAPS["k3"]), None, "n-major weights need n_taps == 1"),
        ("tile12", dict(tile=12), None, "unknown tile id"),
        ("N_out", dict(N_out=20), None, "N_out"),
    ]


def reject_case(rid):
    """(keywords with Bufs for everything writable, Case for check_outputs, params edit, message)"""
    _, ch, edit, msg = next(r for r in rejects() if r[0] == rid)
    rng = _Rng("conv-reject-" + rid)
    B, T, C, N = 2, ch.get("T", 33), ch.get("C_in", 32), ch.get("N", 32)
    taps = ch.get("taps", (-1, 0, 1))
    ldw = (N + 4) if ch.get("w_nmajor") else _r4(len(taps) * C) + 4
    out = Buf(B * T * N)
    kw = dict(n_batch=B, T_in=T, T_out=T, C_in=C, N=N, taps=taps, in0=(rng.n(8 + B * T * 32), ch.get("in0_off", 4)),
              in0_bs=T * 32, ld_in0=32, w=(rng.n(4 + 128 * ldw), 4), ldw=ldw, out=(out, 0), out_bs=T * N, ld_out=N,
              tile=ch.get("tile", 0), precision=FP32)
    outs = [Out("out", out, torch.zeros(out.n, dtype=torch.float64), written=torch.zeros(out.n, dtype=torch.bool))]
    for k in ("geglu", "reflect", "w_nmajor", "N_out"):
        if k in ch:
            kw[k] = ch[k]
    if ch.get("gn"):
        gn = Buf(B * 2 * 2 * 2)
        kw["gn_partials"] = (gn, 0)
        outs.append(Out("gn_partials", gn, torch.zeros(gn.n, dtype=torch.float64), written=torch.zeros(gn.n, dtype=torch.bool)))
    if "tr_col0" in ch:
        tr = Buf(B * N * 40)
        kw.update(out_tr=(tr, 0), out_tr_bs=N * 40, ld_out_tr=40, out_tr_col0=ch["tr_col0"])
        outs.append(Out("out_tr", tr, torch.zeros(tr.n, dtype=torch.float64), written=torch.zeros(tr.n, dtype=torch.bool)))
    return Case("reject " + rid, tuple(kw.items()), outs, kind="conv", error=msg), edit


def _main():
    worst = {"fp32": 0.0, "bf16x3": 0.0}
    where = {}
    for form, vid in all_ids():
        for which in worst:
            e = baseline_error(form, vid, which)
            if e > worst[which]:
                worst[which], where[which] = e, (form, vid)
    for which, e in worst.items():
        print(f"TOL    {which!r}: ({e:.3e}, {_round_up(max(4 * e, FLOOR)):.1e}),   # worst at {where.get(which)}", flush=True)
    print(f"cases: {len(all_ids())} over {len(forms())} forms")


if __name__ == "__main__":
    _main()
