"""Case generators and float64 references for the row / norm / training kernels (norm_act.hip, train.hip, gst_train.hip).

Shared by tests/test_rowops_emulated.py (CPU: the emulator and a plain fp32 restatement against these references) and
tests/test_hip_rowops.py (MI355X: the HIP kernels against the same references).  No GPU is touched here.

A case holds the arguments of one C-ABI call in the order of ``tests/_emulator.emul_call`` / ``ops.CallOp``.  Every
buffer the call writes is a ``Buf``: the payload sits between two guard bands of ``G`` sentinel values, and every element
the contract says is not written (``ld`` padding columns, rows past a length) starts as the sentinel too (or, for a
buffer updated in place, as its input value) and must come back bit for bit.  Each ``Out`` carries the float64 reference
of one buffer, computed from the same fp32 inputs with straightforward torch expressions.

Pass criterion, per element:   |got - ref| <= tol_op * (|ref| + s)
with s the RMS of the reference over the reduction unit the element belongs to: the row for LayerNorm / softmax, the
(item, group) for GroupNorm, the column for BatchNorm, the whole tensor for element-wise maps.  An output that IS a
reduction (column sums, partial sums, gsum) takes the vector of its neighbouring sums of the same item as its unit.

tol_op is not chosen: it is 4 x the worst error, under the same formula and over the same sweep, of the same operation
restated in fp32 on the CPU (the emulator where it computes in fp32, a plain torch restatement otherwise), rounded up to
two digits, with a floor of 8 * 2^-24.  `python -m tests._rowop_cases` prints the measured column again;
test_rowops_emulated.py asserts that the restatement stays within tol_op / 4, so the table cannot rot.

  op                        fp32 baseline   tol_op     remark
  srn_gn_mish_apply         3.790e-07       1.6e-06    statistics from fp32 32 x 32 tile sums (the contract), reference from x itself
  srn_resblock_tail         7.283e-07       3.0e-06    the same
  srn_resblock_tail_ln      8.852e-07       3.6e-06    the same
  srn_gn_stats              6.697e-08       4.8e-07    floor; the emulator adds the fp32 tile sums in fp64, as the kernel does
  srn_layernorm             2.026e-07       8.2e-07
  srn_rowln_fwd             3.237e-07       1.3e-06
  srn_rowln_bwd             2.061e-06       8.3e-06
  srn_gn_mish_bwd_partial   5.507e-07       2.3e-06
  srn_gn_mish_bwd_apply     2.004e-06       8.1e-06
  srn_chunk_colsum          2.311e-07       9.3e-07
  srn_softmax_rows          2.450e-06       9.9e-06    fp32 sum of up to 9216 exponentials
  srn_softmax_bwd           1.845e-06       7.4e-06
  srn_geglu_fwd             3.599e-07       1.5e-06
  srn_geglu_bwd             4.372e-07       1.8e-06
  srn_adamw                 2.838e-07       1.2e-06    scalars as the C ABI rounds them: 1 - float(0.999), not 0.001
  srn_adamw_dyn             2.838e-07       1.2e-06    the same
  srn_colsum                2.722e-07       1.1e-06
  srn_sinusoidal_emb        6.269e-05       2.6e-04    one ulp of an fp32 argument of 1e3 is 6e-5: the argument rounding
  srn_renorm                1.459e-07       5.9e-07
  srn_out_conv_tanh         1.346e-06       5.4e-06
  srn_pd_gather             3.107e-08       4.8e-07    floor
  srn_weight_norm_fwd       1.416e-07       5.7e-07
  srn_weight_norm_bwd       4.092e-07       1.7e-06
  srn_bn_relu_fwd           3.657e-06       1.5e-05    baseline with the kernel's formula: fp32 column sums of x - x[0] and its square
  srn_bn_relu_bwd           8.276e-07       3.4e-06
  srn_col2im_s2             1.377e-07       5.6e-07
  srn_gru_train_fwd         1.187e-06       4.8e-06
  srn_gru_train_bwd         1.291e-05       5.2e-05    64 steps of back-propagation through time
  srn_token_attn_fwd        1.345e-06       5.4e-06
  srn_token_attn_bwd        6.478e-06       2.6e-05
  srn_sumsq                 -               1e-12      sum of the fp64 partials against the fp64 sum of the fp32 inputs (relative)
  srn_dot                   -               1e-12      sum of the fp64 partials against the fp64 sum of the fp32 inputs (relative)
  srn_copy_channels, srn_scatter_rows, srn_transpose_ct, srn_transpose_multi, srn_multi_copy, srn_im2col_s2: bit for bit
Elements with a tolerance of their own (CASE_TOL): in the GroupNorm cases where one (item, group) has a variance of 1e-6
of its squared mean, the E[x^2] - mean^2 formula on fp32 32 x 32 tile sums (the kernels' contract: the statistics come
from the producing conv's partial sums) loses the variance itself; kernel and restatement get the same fp32 partials.
Only the elements that variance reaches are held to 4 x what the restatement reaches on them: that group's channels of
that item in gn_mish_apply, its rstd in gn_stats, and that item's rows in the two tail kernels (their LayerNorm runs
over all channels of a row, so the group's error enters the row's mean and variance).  Everything else in those cases
stays under tol_op.
BatchNorm backward over two rows: dx cancels analytically to O(eps / var), so the column RMS of the reference is no
scale for it; for rows <= 2 the unit of dx is gamma rstd RMS(dy), the size of the terms that cancel (the rounding an
fp32 evaluation cannot avoid is relative to those); at rows = 2, dx alone is held to 4 x the restatement's error in
that unit (xhat of two nearly equal values carries the rounding of x - mean), `sums` stays under tol_op.
Where no fp32 restatement of its own is listed (BASELINE), the baseline is the emulator; for srn_gn_stats and the
statistics inside the GroupNorm forward ops the emulator adds the fp32 tile sums in fp64 as the kernels do, so the figure
there is the rounding of the tile sums and of the output, not of an fp32 reduction.
"""
import math
import types
import zlib

import torch
import torch.nn.functional as F

G = 64                 # guard band, elements on either side of an output buffer
SENT = -12345.0        # finite sentinel: guards, ld padding, rows the contract leaves alone
FLOOR = 8 * 2.0 ** -24

# op -> (measured fp32 baseline, tol_op); filled from `python -m tests._rowop_cases`
TOL = {
    'srn_gn_mish_apply': (3.790e-07, 1.6e-06),
    'srn_resblock_tail': (7.283e-07, 3.0e-06),
    'srn_resblock_tail_ln': (8.852e-07, 3.6e-06),
    'srn_gn_stats': (6.697e-08, 4.8e-07),
    'srn_layernorm': (2.026e-07, 8.2e-07),
    'srn_rowln_fwd': (3.237e-07, 1.3e-06),
    'srn_rowln_bwd': (2.061e-06, 8.3e-06),
    'srn_gn_mish_bwd_partial': (5.507e-07, 2.3e-06),
    'srn_gn_mish_bwd_apply': (2.004e-06, 8.1e-06),
    'srn_chunk_colsum': (2.311e-07, 9.3e-07),
    'srn_softmax_rows': (2.450e-06, 9.9e-06),
    'srn_softmax_bwd': (1.845e-06, 7.4e-06),
    'srn_geglu_fwd': (3.599e-07, 1.5e-06),
    'srn_geglu_bwd': (4.372e-07, 1.8e-06),
    'srn_adamw': (2.838e-07, 1.2e-06),
    'srn_adamw_dyn': (2.838e-07, 1.2e-06),
    'srn_colsum': (2.722e-07, 1.1e-06),
    'srn_sinusoidal_emb': (6.269e-05, 2.6e-04),
    'srn_renorm': (1.459e-07, 5.9e-07),
    'srn_out_conv_tanh': (1.346e-06, 5.4e-06),
    'srn_pd_gather': (3.107e-08, 4.8e-07),
    'srn_weight_norm_fwd': (1.416e-07, 5.7e-07),
    'srn_weight_norm_bwd': (4.092e-07, 1.7e-06),
    'srn_bn_relu_fwd': (3.657e-06, 1.5e-05),
    'srn_bn_relu_bwd': (8.276e-07, 3.4e-06),
    'srn_col2im_s2': (1.377e-07, 5.6e-07),
    'srn_gru_train_fwd': (1.187e-06, 4.8e-06),
    'srn_gru_train_bwd': (1.291e-05, 5.2e-05),
    'srn_token_attn_fwd': (1.345e-06, 5.4e-06),
    'srn_token_attn_bwd': (6.478e-06, 2.6e-05),
}
# (op, case id) -> (measured fp32 baseline of that case, tolerance): see the module docstring
CASE_TOL = {
    ('srn_gn_mish_apply', 'lowvar-C256g8-T33-B2-valid0-tb0-lensNULL'): (1.480e-01, 6.0e-01),
    ('srn_resblock_tail', 'lowvar-C256g8-T33-B2-valid0-tb0-lensNULL'): (8.814e-02, 3.6e-01),
    ('srn_resblock_tail_ln', 'lowvar-C256g8-T33-B2-valid0-tb0-lensNULL'): (2.408e-01, 9.7e-01),
    ('srn_gn_stats', 'lowvar-C256g8-T33-B2'): (5.818e-03, 2.4e-02),
    ('srn_bn_relu_bwd', 'rows2-C4'): (6.387e-08, 4.8e-07),
    ('srn_bn_relu_bwd', 'rows2-C32'): (3.855e-07, 1.6e-06),
    ('srn_bn_relu_bwd', 'rows2-C128'): (1.841e-06, 7.4e-06),
}
FIXED_TOL = {"srn_sumsq": 1e-12, "srn_dot": 1e-12}  # fp64 partial sums against the fp64 sum of the fp32 inputs
EXACT_OPS = ("srn_copy_channels", "srn_scatter_rows", "srn_transpose_ct", "srn_transpose_multi", "srn_multi_copy",
             "srn_im2col_s2")  # pure data movement: bit for bit


# The low-variance GroupNorm cases mark the elements the lost variance reaches (Out.ill) and hold those alone to CASE_TOL,
# 4 x the restatement's own error on them; every other element of the same case stays under TOL[op].
# The same for dx of the BatchNorm backward over two rows (see the module docstring for its unit).
ILL = (("", "lowvar"), ("srn_bn_relu_bwd", "rows2-"))


def ill_conditioned(op, cid):
    return any(op.startswith(o) and cid.startswith(c) for o, c in ILL)


def tol_for(op, cid):
    """(tol_op, the tolerance of the elements the case marks ill-conditioned: tol_op where it marks none)"""
    if op in FIXED_TOL:
        return FIXED_TOL[op], FIXED_TOL[op]
    if op in EXACT_OPS:
        return 0.0, 0.0
    return TOL[op][1], CASE_TOL.get((op, cid), TOL[op])[1]


def within(errs, tols):
    return errs[0] <= tols[0] and errs[1] <= tols[1]


def f32(v):
    """a Python float as the kernel receives it (c_float)"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _seed(s):
    return zlib.crc32(s.encode()) & 0x7FFFFFFF


class _Rng:
    def __init__(self, key):
        self.g = torch.Generator().manual_seed(_seed(key))

    def n(self, *shape):
        return torch.randn(*shape, generator=self.g)

    def u(self, *shape):
        return torch.rand(*shape, generator=self.g)


class Buf:
    """an output (or in-place) buffer of n elements between two guard bands"""

    def __init__(self, n, init=None, dtype=torch.float32):
        self.n = int(n)
        self.big = torch.full((self.n + 2 * G,), SENT, dtype=dtype)
        if init is not None:
            self.big[G:G + self.n] = init.reshape(-1).to(dtype)

    def initial(self):
        return self.big[G:G + self.n]


class Out:
    """what one Buf must hold after the call.  ref: float64, its shape is the logical layout; s / written / zero
    broadcast to it.  written None: every element; scratch: only the guards are checked."""

    def __init__(self, name, buf, ref=None, s=None, written=None, zero=None, exact=False, scratch=False, extra=None,
                 free=False, ill=None):
        self.name, self.buf, self.ref, self.s = name, buf, ref, s
        self.written, self.zero, self.exact, self.scratch, self.extra = written, zero, exact, scratch, extra
        self.ill = ill    # mask of the elements an ill-conditioned case holds to CASE_TOL; all others stay under TOL[op]
        self.free = free  # written elements are only required to be finite (`extra` judges them together)
        if not scratch:
            assert ref.dim() >= 1 and ref.numel() == buf.n, (name, ref.shape, buf.n)


class Case:
    def __init__(self, op, args, outs, kind="call", error=None):
        self.op, self.args, self.outs, self.kind, self.error = op, args, outs, kind, error


def materialize(case, dev=None):
    """fresh copies of every Buf (and, with dev, of every input on that device): (args, {id(Buf): whole buffer})"""
    bufs, ins = {}, {}

    def m(a):
        if isinstance(a, Buf):
            if id(a) not in bufs:
                bufs[id(a)] = a.big.clone() if dev is None else a.big.to(dev)
            return bufs[id(a)][G:G + a.n]
        if isinstance(a, torch.Tensor):
            if dev is None:
                return a
            if id(a) not in ins:  # one device copy per input, however many arguments point into it
                ins[id(a)] = a.to(dev)
            return ins[id(a)]
        if isinstance(a, (tuple, list)):
            return type(a)(m(x) for x in a)
        return a

    return m(case.args), bufs


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def check_outputs(case, bufs):
    """guards, untouched elements, exact zeros, bit-exact outputs: asserted here.  Returns the worst per-element error
    |g - r| / (|r| + s) over the compared outputs (0.0 for an exact op) as (over the ordinary elements, over the
    elements marked ill-conditioned)."""
    worst, worst_ill = 0.0, 0.0
    for o in case.outs:
        big = bufs[id(o.buf)].cpu()
        n = o.buf.n
        assert bool((big[:G] == SENT).all()) and bool((big[G + n:] == SENT).all()), \
            f"{case.op}: {o.name}: a guard band was written"
        if o.scratch:
            continue
        shape = o.ref.shape
        g_all = big[G:G + n].view(shape)
        init_all = o.buf.initial().view(shape)
        bc = lambda t: None if t is None else torch.broadcast_to(t, shape)
        s_all, w_all, z_all, ill_all = bc(o.s), bc(o.written), bc(o.zero), bc(o.ill)
        step = max(1, (4 << 20) // max(1, o.ref[0].numel()))  # a few million elements at a time
        for i0 in range(0, shape[0], step):
            sl = slice(i0, i0 + step)
            g, r = g_all[sl], o.ref[sl]
            w = None if w_all is None else w_all[sl]
            if w is not None:
                assert torch.equal(_bits(g[~w]), _bits(init_all[sl][~w])), \
                    f"{case.op}: {o.name}: an element the contract leaves alone was written"
                g, r = g[w], r[w]
            if z_all is not None:
                z = z_all[sl] if w is None else z_all[sl][w]
                assert bool((g[z] == 0).all()), f"{case.op}: {o.name}: an element that must be exactly 0 is not"
            if o.exact:
                assert torch.equal(g, r.to(g.dtype)), f"{case.op}: {o.name}: not bit for bit"
                continue
            assert bool(torch.isfinite(g).all()), f"{case.op}: {o.name}: non-finite output"
            if o.free or g.numel() == 0:
                continue
            s = s_all[sl] if w is None else s_all[sl][w]
            e = (g.double() - r).abs_() / (r.abs() + s).clamp_min(1e-300)
            if ill_all is not None:
                ill = ill_all[sl] if w is None else ill_all[sl][w]
                if bool(ill.any()):
                    worst_ill = max(worst_ill, float(e[ill].max()))
                e = e[~ill]
            if e.numel():
                worst = max(worst, float(e.max()))
        if o.extra is not None:
            worst = max(worst, float(o.extra(g_all)))
    return worst, worst_ill


def run_emulated(case, args):
    """the call through the CPU executable spec"""
    from tests import _emulator
    if case.kind == "call":
        _emulator.emul_call(case.op, list(args))
    elif case.kind == "multi_copy":
        srcs, offs, lens, dst = args
        for (pool, so), o, n in zip(srcs, offs, lens):
            dst[o:o + n] = pool.view(-1)[so:so + n]
    elif case.kind == "transpose_multi":
        _emulator.emul_transpose_multi(types.SimpleNamespace(entries=args))


# ------------------------------------------------------------------------------------------------ sweep registry
SWEEPS = {}
_LISTS = {}
BASELINE = {}  # op -> fp32 restatement with emul_call's signature, where the emulator itself computes in fp64


def sweep(op):
    def deco(fn):
        SWEEPS[op] = fn
        return fn
    return deco


def _list(op):
    if op not in _LISTS:
        lst = list(SWEEPS[op]())
        assert len({c for c, _ in lst}) == len(lst), f"{op}: duplicate case ids"
        _LISTS[op] = dict(lst)
    return _LISTS[op]


def case_ids(op):
    return list(_list(op))


def make(op, cid):
    return _list(op)[cid]()


def cases(op):
    """(case_id, args) in emul_call / CallOp order, as (case_id, Case) with Case.args"""
    for cid, build in _list(op).items():
        yield cid, build()


def all_ids(error=None):
    """[(op, case id)] over every sweep; error True / False: only the cases that must / must not be rejected"""
    out = []
    for op in SWEEPS:
        for cid in case_ids(op):
            is_err = cid.startswith("reject-")
            if error is None or error == is_err:
                out.append((op, cid))
    return out


def run_baseline(case, args):
    fn = BASELINE.get(case.op)
    if fn is None:
        run_emulated(case, args)
    else:
        fn(list(args))


def rms(t, dims, keepdim=True):
    return t.pow(2).mean(dim=dims, keepdim=keepdim).sqrt()


# ------------------------------------------------------------------------------------------------ GroupNorm family
CG = ((256, 8), (512, 8), (1024, 8), (64, 2), (1024, 1))
TS = (1, 3, 4, 5, 8, 9, 33, 75)


def _lens_for(T, B, i):
    """full, 1, T - 1 and lengths with len % 8 in {1, 4, 7}, rotated over the items"""
    def mod(m):
        v = T - ((T - m) % 8)
        return v if 1 <= v <= T else min(T, max(1, m))
    cand = [T, 1, max(1, T - 1), mod(1), mod(4), mod(7)]
    return [cand[(i + j) % 6] for j in range(B)]


def _partials(x):
    """the producing conv's per-(32 rows x 32 channels) tile sums (sum, sum of squares), in fp32 as its epilogue forms them"""
    B, Tn, C = x.shape
    mt, nt = (Tn + 31) // 32, C // 32
    pad = torch.zeros(B, mt * 32, C)
    pad[:, :Tn] = x
    t = pad.reshape(B, mt, 32, nt, 32)
    return torch.stack([t.sum(dim=(2, 4)), (t ** 2).sum(dim=(2, 4))], dim=-1).contiguous()


def _gn_xhat(x64, lens, groups, eps, valid):
    B, T, C = x64.shape
    cpg = C // groups
    xh = torch.empty_like(x64)
    for b in range(B):
        n = lens[b] if valid else T
        xg = x64[b, :n].reshape(n, groups, cpg)
        mean, var = xg.mean((0, 2)), xg.var((0, 2), unbiased=False)
        xh[b] = ((x64[b].reshape(T, groups, cpg) - mean[None, :, None]) / torch.sqrt(var[None, :, None] + eps)).reshape(T, C)
    return xh


def _group_rms(y, lens, groups):
    B, T, C = y.shape
    cpg = C // groups
    s = torch.ones_like(y)
    for b in range(B):
        n = lens[b]
        r = y[b, :n].reshape(n, groups, cpg).pow(2).mean((0, 2)).sqrt()
        s[b] = r.repeat_interleave(cpg)[None, :].expand(T, C)
    return s


def _gn_shapes(wide):
    out, i = [], 0
    for (C, g) in CG + (((2048, 64),) if wide else ()):
        for T in TS:
            out.append(dict(B=3, T=T, C=C, groups=g, i=i))
            i += 1
    # both sides of the rows-per-workgroup switch (B * ceil(T / 8) = 511 | 512), well above it, and C = 1024 in the
    # 8-row branch (the loop behind gn_mish_apply's prefetch)
    out += [dict(B=7, T=583, C=64, groups=2, i=1, tag="wg511"), dict(B=8, T=509, C=64, groups=2, i=2, tag="wg512"),
            dict(B=8, T=1000, C=64, groups=2, i=3, tag="wg1000"), dict(B=8, T=509, C=1024, groups=8, i=4, tag="wg512"),
            dict(B=2, T=33, C=256, groups=8, i=0, tag="lowvar")]
    return out


def _gn_case_id(p, valid, tb, lens, use_lens):
    return (f"{p.get('tag', 'grid')}-C{p['C']}g{p['groups']}-T{p['T']}-B{p['B']}-valid{valid}-tb{tb}-lens"
            + ("NULL" if not use_lens else "_".join(str(v) for v in lens)))


def _gn_inputs(op, p):
    B, T, C, groups, i = p["B"], p["T"], p["C"], p["groups"], p["i"]
    lowvar = p.get("tag") == "lowvar"
    valid = 0 if lowvar else i % 2
    tb = (i // 2) % 2
    lens = _lens_for(T, B, i)
    use_lens = bool(valid) or i % 5 != 0
    if not use_lens:
        lens = [T] * B
    cid = _gn_case_id(p, valid, tb, lens, use_lens)
    return cid, dict(B=B, T=T, C=C, groups=groups, valid=valid, tb=tb, lens=lens, use_lens=use_lens, lowvar=lowvar,
                     key=op + cid)


def _gn_tensors(q):
    r = _Rng(q["key"])
    B, T, C, groups = q["B"], q["T"], q["C"], q["groups"]
    x = r.n(B, T, C) * 2 + 0.3
    if q["lowvar"]:
        x[0, :, :C // groups] = 1000.0 + r.n(T, C // groups)  # variance 1e-6 of the squared mean
    lens = q["lens"]
    if q["valid"]:
        x = x * (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float().unsqueeze(-1)  # the producing conv's len_out
    gamma, beta = 1 + 0.1 * r.n(C), 0.1 * r.n(C)
    lens_t = torch.tensor(lens, dtype=torch.int32) if q["use_lens"] else None
    return r, x, gamma, beta, lens_t


@sweep("srn_gn_mish_apply")
def _sw_gn_mish_apply():
    for p in _gn_shapes(wide=True):
        cid, q = _gn_inputs("srn_gn_mish_apply", p)
        yield cid, (lambda q=q: _mk_gn_mish_apply(q))


def _mk_gn_mish_apply(q):
    r, x, gamma, beta, lens_t = _gn_tensors(q)
    B, T, C, groups, lens = q["B"], q["T"], q["C"], q["groups"], q["lens"]
    eps = 1e-5
    tb, tb_bs, tb_arg = None, 0, None
    if q["tb"]:  # a non-zero offset and batch stride
        tb_bs = 2 * C
        tb = r.n(C + B * tb_bs)
        tb_arg = (tb, C)
    y64 = F.mish(_gn_xhat(x.double(), lens, groups, f32(eps), q["valid"]) * gamma.double() + beta.double())
    if tb is not None:
        y64 = y64 + tb.double()[C:].reshape(B, tb_bs)[:, None, :C]
    rows = torch.arange(T)[None, :, None] >= torch.tensor(lens)[:, None, None]
    y64 = y64.masked_fill(rows, 0.0)
    y = Buf(B * T * C)
    args = [x, _partials(x), gamma, beta, tb_arg, tb_bs, lens_t, y, B, T, C, groups, eps, q["valid"]]
    ill = None
    if q["lowvar"]:  # item 0, group 0
        ill = torch.zeros(B, 1, C, dtype=torch.bool)
        ill[0, 0, :C // groups] = True
    return Case("srn_gn_mish_apply", args, [Out("y", y, y64, _group_rms(y64, lens, groups), zero=rows, ill=ill)])


def _tail_common(op, q):
    r, x, gamma, beta, lens_t = _gn_tensors(q)
    B, T, C, groups, lens = q["B"], q["T"], q["C"], q["groups"], q["lens"]
    eps = f32(1e-5)
    res = r.n(B, T, C)
    ss = r.n(B * 4 * C)
    o = F.mish(_gn_xhat(x.double(), lens, groups, eps, q["valid"]) * gamma.double() + beta.double())
    o = o.masked_fill(torch.arange(T)[None, :, None] >= torch.tensor(lens)[:, None, None], 0.0)
    v = o + res.double()
    ssd = ss.double().reshape(B, 4 * C)
    y64 = F.layer_norm(v, (C,), None, None, eps) * ssd[:, None, C:2 * C] + ssd[:, None, 2 * C:3 * C]
    y = Buf(B * T * C)
    args = [x, _partials(x), gamma, beta, lens_t, res, (ss, C), (ss, 2 * C), 4 * C, y, B, T, C, groups, 1e-5, 1e-5,
            q["valid"]]
    ill = None
    if q["lowvar"]:  # every row of item 0: the LayerNorm behind the GroupNorm runs over all channels of a row
        ill = torch.zeros(B, 1, 1, dtype=torch.bool)
        ill[0] = True
    outs = [Out("y", y, y64, rms(y64, -1), ill=ill)]
    if op == "srn_resblock_tail_ln":
        g2, b2 = 1 + 0.1 * r.n(C), 0.1 * r.n(C)
        y2_64 = F.layer_norm(y64, (C,), g2.double(), b2.double(), eps)
        y2 = Buf(B * T * C)
        args += [g2, b2, y2, 1e-5]
        outs.append(Out("y2", y2, y2_64, rms(y2_64, -1), ill=ill))
    return Case(op, args, outs)


def _sw_tail(op):
    def gen():
        for p in _gn_shapes(wide=False):
            cid, q = _gn_inputs(op, p)
            yield cid, (lambda q=q: _tail_common(op, q))
        # C above the MAXV limit: rejected, nothing written
        yield "reject-C1056", lambda: _mk_tail_reject(op)
    return gen


def _mk_tail_reject(op):
    _, q = _gn_inputs(op, dict(B=1, T=3, C=1056, groups=1, i=1))
    c = _tail_common(op, q)
    for o in c.outs:
        o.written = torch.zeros((), dtype=torch.bool)
    c.error = "unsupported"
    return c


SWEEPS["srn_resblock_tail"] = _sw_tail("srn_resblock_tail")
SWEEPS["srn_resblock_tail_ln"] = _sw_tail("srn_resblock_tail_ln")


@sweep("srn_gn_stats")
def _sw_gn_stats():
    for p in _gn_shapes(wide=True):
        q = dict(B=p["B"], T=p["T"], C=p["C"], groups=p["groups"], valid=0, lens=[p["T"]] * p["B"], use_lens=False,
                 lowvar=p.get("tag") == "lowvar")
        cid = f"{p.get('tag', 'grid')}-C{p['C']}g{p['groups']}-T{p['T']}-B{p['B']}"
        q["key"] = "srn_gn_stats" + cid
        yield cid, (lambda q=q: _mk_gn_stats(q))


def _mk_gn_stats(q):
    _, x, _, _, _ = _gn_tensors(q)
    B, T, C, groups = q["B"], q["T"], q["C"], q["groups"]
    xg = x.double().reshape(B, T, groups, C // groups)
    mean64 = xg.mean((1, 3))
    rstd64 = 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + f32(1e-5))
    mean, rstd = Buf(B * groups), Buf(B * groups)
    args = [_partials(x), mean, rstd, B, T, C, groups, 1e-5]
    # mean: held to the scale of the data it averages (the group's RMS), so a mean near zero is not asked for digits
    # the fp32 tile sums never had
    ill = None
    if q["lowvar"]:  # rstd of item 0, group 0
        ill = torch.zeros(B, groups, dtype=torch.bool)
        ill[0, 0] = True
    return Case("srn_gn_stats", args, [Out("mean", mean, mean64, rms(xg, (1, 3), keepdim=False)),
                                      Out("rstd", rstd, rstd64, rstd64.abs(), ill=ill)])


# ------------------------------------------------------------------------------------------------ LayerNorm family
LN_C = (256, 512, 1024, 64, 4, 80, 1020)


@sweep("srn_layernorm")
def _sw_layernorm():
    for C in LN_C:
        for T in TS:
            yield f"C{C}-rows{2 * T}", (lambda C=C, T=T: _mk_layernorm(2 * T, C))
    yield "gridstride-C64-rows262151", lambda: _mk_layernorm(4 * 65536 + 7, 64)  # past the 65536-workgroup cap
    yield "reject-C1028", lambda: _mk_layernorm(3, 1028, error="unsupported")


def _mk_layernorm(rows, C, error=None):
    r = _Rng(f"ln{rows}x{C}")
    x = r.n(rows, C) * 2 + 0.3
    gamma, beta = 1 + 0.1 * r.n(C), 0.1 * r.n(C)
    y64 = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), f32(1e-5))
    y = Buf(rows * C)
    out = Out("y", y, y64, rms(y64, -1), written=torch.zeros((), dtype=torch.bool) if error else None)
    return Case("srn_layernorm", [x, gamma, beta, y, rows, C, 1e-5], [out], error=error)


def _rowln_inputs(key, B, T, C, per_b):
    r = _Rng(key)
    x = r.n(B, T, C) * 2 + 0.3
    nb = B if per_b else 1
    m, a = 1 + 0.3 * r.n(nb, C), 0.5 * r.n(nb, C)
    return r, x, m, a, (C if per_b else 0)


def _rowln_shapes():
    i = 0
    for C in LN_C:
        for T in TS:
            yield dict(B=3, T=T, C=C, per_b=i % 2)
            i += 1
    yield dict(B=1, T=4 * 16384 + 5, C=64, per_b=0)  # past rowln_fwd's 16384-workgroup cap


@sweep("srn_rowln_fwd")
def _sw_rowln_fwd():
    for p in _rowln_shapes():
        yield "C{C}-T{T}-B{B}-perb{per_b}".format(**p), (lambda p=p: _mk_rowln_fwd(**p))


def _mk_rowln_fwd(B, T, C, per_b):
    _, x, m, a, bs = _rowln_inputs(f"rowlnf{B}-{T}-{C}", B, T, C, per_b)
    y64 = F.layer_norm(x.double(), (C,), None, None, f32(1e-5)) * m.double()[:, None] + a.double()[:, None]
    y = Buf(B * T * C)
    return Case("srn_rowln_fwd", [x, m, bs, a, bs, y, B, T, C, 1e-5], [Out("y", y, y64, rms(y64, -1))])


from serenade_amd.training import NORM_BWD_ROWS  # noqa: E402  rows per chunk of srn_rowln_chunks / srn_gn_chunks


def _chunk_sums(v, T):
    """(B, T, C) -> (B, ceil(T / 8), C): sums over each chunk of 8 rows"""
    B, _, C = v.shape
    nch = (T + NORM_BWD_ROWS - 1) // NORM_BWD_ROWS
    pad = torch.zeros(B, nch * NORM_BWD_ROWS, C, dtype=v.dtype)
    pad[:, :T] = v
    return pad.reshape(B, nch, NORM_BWD_ROWS, C).sum(2)


@sweep("srn_rowln_bwd")
def _sw_rowln_bwd():
    for p in _rowln_shapes():
        if p["T"] > 100:
            p = dict(p, T=1003)  # many chunks; the backward has one workgroup per chunk and no cap
        yield "C{C}-T{T}-B{B}-perb{per_b}".format(**p), (lambda p=p: _mk_rowln_bwd(**p))


def _mk_rowln_bwd(B, T, C, per_b):
    r, x, m, _, bs = _rowln_inputs(f"rowlnb{B}-{T}-{C}", B, T, C, per_b)
    dy = r.n(B, T, C)
    x64 = x.double().requires_grad_(True)
    xh = F.layer_norm(x64, (C,), None, None, f32(1e-5))
    (xh * m.double()[:, None]).backward(dy.double())
    xh = xh.detach()
    part64 = torch.stack([_chunk_sums(dy.double() * xh, T), _chunk_sums(dy.double(), T)], dim=2)  # (B, nch, 2, C)
    dx, part = Buf(B * T * C), Buf(part64.numel())
    return Case("srn_rowln_bwd", [x, dy, m, bs, dx, part, B, T, C, 1e-5],
                [Out("dx", dx, x64.grad, rms(x64.grad, -1)), Out("partial", part, part64, rms(part64, -1))])


# ------------------------------------------------------------------------------------------------ GroupNorm backward
CG_BWD = CG + ((64, 16), (256, 64))  # the last two: C / groups = 4


def _mish_grad64(g):
    g = g.detach().clone().requires_grad_(True)
    F.mish(g).backward(torch.ones_like(g))
    return g.grad


def _gn_bwd_common(key, B, T, C, groups, i):
    r = _Rng(key)
    cpg = C // groups
    lens = _lens_for(T, B, i)
    use_lens = i % 5 != 0
    if not use_lens:
        lens = [T] * B
    h = r.n(B, T, C) * 2 + 0.3
    dy = r.n(B, T, C)
    gamma, beta = 0.5 + r.u(C), r.n(C)
    hg = h.double().reshape(B, T, groups, cpg)
    mean = hg.mean((1, 3)).float()                                            # what srn_gn_stats hands over, in fp32
    rstd = (1.0 / torch.sqrt(hg.var((1, 3), unbiased=False) + f32(1e-5))).float()
    mu = mean.double().repeat_interleave(cpg, 1)[:, None]
    rs = rstd.double().repeat_interleave(cpg, 1)[:, None]
    xh = (h.double() - mu) * rs
    valid = (torch.arange(T)[None, :, None] < torch.tensor(lens)[:, None, None]).double()
    dg = dy.double() * _mish_grad64(xh * gamma.double() + beta.double()) * valid
    lens_t = torch.tensor(lens, dtype=torch.int32) if use_lens else None
    return dict(h=h, dy=dy, gamma=gamma, beta=beta, mean=mean, rstd=rstd, xh=xh, rs=rs, dg=dg, lens_t=lens_t)


def _gn_bwd_shapes():
    i = 0
    for (C, g) in CG_BWD:
        for T in TS:
            yield dict(B=3, T=T, C=C, groups=g, i=i)
            i += 1
    yield dict(B=2, T=1003, C=64, groups=2, i=1)


def _gn_bwd_id(p):
    lens = _lens_for(p["T"], p["B"], p["i"]) if p["i"] % 5 else None
    return "C{C}g{groups}-T{T}-B{B}-lens".format(**p) + ("NULL" if lens is None else "_".join(str(v) for v in lens))


@sweep("srn_gn_mish_bwd_partial")
def _sw_gn_bwd_partial():
    for p in _gn_bwd_shapes():
        yield _gn_bwd_id(p), (lambda p=p: _mk_gn_bwd_partial(**p))
    yield "reject-C2048g8", lambda: _mk_gn_bwd_partial(B=1, T=3, C=2048, groups=8, i=1, error="unsupported")


def _mk_gn_bwd_partial(B, T, C, groups, i, error=None):
    d = _gn_bwd_common(f"gnbp{B}-{T}-{C}-{groups}", B, T, C, groups, i)
    part64 = torch.stack([_chunk_sums(d["dg"], T), _chunk_sums(d["dg"] * d["xh"], T)], dim=2)
    part = Buf(part64.numel())
    args = [d["h"], d["dy"], d["mean"], d["rstd"], d["gamma"], d["beta"], d["lens_t"], part, B, T, C, groups]
    out = Out("partial", part, part64, rms(part64, -1), written=torch.zeros((), dtype=torch.bool) if error else None)
    return Case("srn_gn_mish_bwd_partial", args, [out], error=error)


@sweep("srn_gn_mish_bwd_apply")
def _sw_gn_bwd_apply():
    for p in _gn_bwd_shapes():
        yield _gn_bwd_id(p), (lambda p=p: _mk_gn_bwd_apply(**p))


def _mk_gn_bwd_apply(B, T, C, groups, i):
    d = _gn_bwd_common(f"gnba{B}-{T}-{C}-{groups}", B, T, C, groups, i)
    cpg = C // groups
    gam = d["gamma"].double()
    gsum = torch.stack([(d["dg"] * gam).sum(1).reshape(B, groups, cpg).sum(-1),
                        (d["dg"] * gam * d["xh"]).sum(1).reshape(B, groups, cpg).sum(-1)], dim=-1).float()  # (B, G, 2)
    n = float(T * cpg)
    A = (gsum[:, :, 0].double() / n).repeat_interleave(cpg, 1)[:, None]
    Bq = (gsum[:, :, 1].double() / n).repeat_interleave(cpg, 1)[:, None]
    dh64 = d["rs"] * (d["dg"] * gam - A - d["xh"] * Bq)
    dh = Buf(B * T * C)
    args = [d["h"], d["dy"], d["mean"], d["rstd"], d["gamma"], d["beta"], gsum, d["lens_t"], dh, B, T, C, groups]
    return Case("srn_gn_mish_bwd_apply", args, [Out("dh", dh, dh64, _group_rms(dh64, [T] * B, groups))])


def gn_backward_by_autograd(B=2, T=13, C=64, groups=2, lens=(13, 6)):
    """(formula, autograd): dh of mish(GroupNorm(h)) * mask by the two-step formula of the kernels' contract and by
    torch.autograd in fp64 -- the restatement above is the gradient it claims to be"""
    r = _Rng("gnauto")
    cpg = C // groups
    h = r.n(B, T, C).double() * 2 + 0.3
    dy, gamma, beta = r.n(B, T, C).double(), (0.5 + r.u(C)).double(), r.n(C).double()
    mask = (torch.arange(T)[None, :, None] < torch.tensor(lens)[:, None, None]).double()
    hr = h.clone().requires_grad_(True)
    y = F.mish(F.group_norm(hr.transpose(1, 2), groups, gamma, beta, 1e-5)).transpose(1, 2) * mask
    y.backward(dy)
    hg = h.reshape(B, T, groups, cpg)
    mu = hg.mean((1, 3)).repeat_interleave(cpg, 1)[:, None]
    rs = (1.0 / torch.sqrt(hg.var((1, 3), unbiased=False) + 1e-5)).repeat_interleave(cpg, 1)[:, None]
    xh = (h - mu) * rs
    dg = dy * _mish_grad64(xh * gamma + beta) * mask
    n = float(T * cpg)
    A = ((dg * gamma).sum(1).reshape(B, groups, cpg).sum(-1) / n).repeat_interleave(cpg, 1)[:, None]
    Bq = ((dg * gamma * xh).sum(1).reshape(B, groups, cpg).sum(-1) / n).repeat_interleave(cpg, 1)[:, None]
    return rs * (dg * gamma - A - xh * Bq), hr.grad


@sweep("srn_chunk_colsum")
def _sw_chunk_colsum():
    for (C, g) in ((256, 8), (512, 8), (1024, 8), (256, 64)):  # with gsum: C % 256 == 0 and 256 % (C / groups) == 0
        for nch in (1, 3, 4, 5, 10, 126):
            yield f"gsum-C{C}g{g}-nch{nch}", (lambda C=C, g=g, nch=nch: _mk_chunk_colsum(3, nch, C, g, True))
    for C in (4, 64, 80, 1020, 1024):
        for nch in (1, 4, 7, 125):
            yield f"plain-C{C}-nch{nch}", (lambda C=C, nch=nch: _mk_chunk_colsum(2, nch, C, 1, False))
    for (C, g) in ((64, 2), (1024, 1)):  # whole groups do not tile a 256-thread block: rejected with gsum
        yield f"reject-gsum-C{C}g{g}", (lambda C=C, g=g: _mk_chunk_colsum(2, 3, C, g, True, error="unsupported"))


def _mk_chunk_colsum(B, nch, C, groups, with_gsum, error=None):
    r = _Rng(f"ccs{B}-{nch}-{C}-{groups}")
    part = r.n(B, nch, 2, C) + 0.1
    gamma = 0.5 + r.u(C)
    col64 = part.double().sum(1)
    none = torch.zeros((), dtype=torch.bool) if error else None
    col = Buf(B * 2 * C)
    outs = [Out("col", col, col64, rms(col64, -1), written=none)]
    gs = None
    if with_gsum:
        g64 = (col64 * gamma.double()).reshape(B, 2, groups, C // groups).sum(-1).transpose(1, 2).contiguous()
        gs = Buf(B * groups * 2)
        outs.append(Out("gsum", gs, g64, rms(g64, 1), written=none))
    return Case("srn_chunk_colsum", [part, gamma if with_gsum else None, col, gs, B, nch, C, groups], outs, error=error)


# ------------------------------------------------------------------------------------------------ softmax
SM_LD = (4, 8, 512, 516, 1024, 1028, 2048, 2052, 3072, 3076, 4096, 5120, 5124, 9216)
SM_VALS = ("normal", "const", "pm80")


@sweep("srn_softmax_rows")
def _sw_softmax_rows():
    k = 0
    for ld in SM_LD:
        if ld <= 516:      # every (L, values) pair; Z = 4 over 2 heads, lens behind a pointer offset
            combos = [(dl, vals) for dl in (0, 1, 3) for vals in SM_VALS]
        elif ld <= 1028:
            combos = [(dl, SM_VALS[(k + j) % 3]) for j, dl in enumerate((0, 1, 3))]
        else:
            combos = [((0, 1, 3)[k % 3], SM_VALS[(k // 2) % 3])]
        for dl, vals in combos:
            L = ld - dl
            if L < 1:
                continue
            Z, nh = (4, 2) if ld <= 1028 else (1, 1)
            short = max(1, L - 9)
            lens = ([L, short], [1, L], [short, 1])[k % 3][:Z // nh]
            if ld == 9216:
                lens = [short]
            yield (f"ld{ld}-L{L}-Z{Z}h{nh}-{vals}-lens{'_'.join(map(str, lens))}",
                   (lambda Z=Z, nh=nh, L=L, ld=ld, lens=lens, vals=vals: _mk_softmax_rows(Z, nh, L, ld, lens, vals)))
            k += 1
    yield "reject-ld9220", lambda: _mk_softmax_rows(1, 1, 5, 9220, [5], "normal", error="9216")


def _mk_softmax_rows(Z, nh, L, ld, lens, vals, error=None):
    r = _Rng(f"sm{Z}-{L}-{ld}-{vals}")
    s = torch.full((Z, L, ld), float("nan"))  # columns [L, ld): the score buffer is never zeroed
    if vals == "const":
        s[:, :, :L] = 1.5
    else:
        s[:, :, :L] = r.n(Z, L, L) * 3
        if vals == "pm80":  # the max subtraction
            s[:, :, 0:L:7] = 80.0
            s[:, :, 3:L:11] = -80.0
            s[:, 0::2, :L] -= 40.0
    lens_t = torch.tensor([-7, -7] + list(lens), dtype=torch.int32)  # read through a pointer offset, as plan.py passes it
    buf = Buf(Z * L * ld, s)
    if error:
        out = Out("s", buf, torch.zeros(Z * L, ld, dtype=torch.float64), written=torch.zeros((), dtype=torch.bool))
        return Case("srn_softmax_rows", [buf, (lens_t, 2), Z, nh, L, ld], [out], error=error)
    ln = torch.tensor(lens).repeat_interleave(nh)[:, None, None]                 # per z
    dead = (torch.arange(ld)[None, None, :] >= ln).expand(Z, L, ld).reshape(Z * L, ld)
    ref = torch.softmax(s.double().reshape(Z * L, ld).masked_fill(dead, float("-inf")), dim=-1)
    n_live = ln.expand(Z, L, 1).reshape(Z * L, 1).double()
    srow = (ref.pow(2).sum(-1, keepdim=True) / n_live).sqrt()

    def row_sums(g):  # every row sums to 1: the sum is one more element with reference 1 and scale 1
        return ((g.double().sum(-1) - 1.0).abs() / 2.0).max()

    return Case("srn_softmax_rows", [buf, (lens_t, 2), Z, nh, L, ld], [Out("s", buf, ref, srow, zero=dead, extra=row_sums)])


@sweep("srn_softmax_bwd")
def _sw_softmax_bwd():
    k = 0
    for L in (1, 3, 4, 45, 255, 256, 257, 1027, 4100):
        for ld in sorted({(L + 3) // 4 * 4, (L + 3) // 4 * 4 + 8}):
            rows = (1, 5, 4, 133)[k % 4] if L < 1000 else (3, 6)[k % 2]
            scale = (0.125, 1.0)[k % 2]
            yield f"L{L}-ld{ld}-rows{rows}-scale{scale}", (lambda L=L, ld=ld, rows=rows, scale=scale:
                                                             _mk_softmax_bwd(rows, L, ld, scale))
            k += 1


def _mk_softmax_bwd(rows, L, ld, scale):
    r = _Rng(f"smb{rows}-{L}-{ld}")
    p = torch.zeros(rows, ld)
    # (short rows stay mildly peaked: with p -> 1 the row's own dp - sum(dp p) cancels and no fp32 form has digits left)
    p[:, :L] = torch.softmax(r.n(rows, L).double() * (3 if L > 4 else 1), -1).float()
    dp = torch.full((rows, ld), SENT)
    dp[:, :L] = r.n(rows, L)
    pd, gd = p.double()[:, :L], dp.double()[:, :L]
    ref = torch.zeros(rows, ld, dtype=torch.float64)
    ref[:, :L] = f32(scale) * pd * (gd - (gd * pd).sum(-1, keepdim=True))
    buf = Buf(rows * ld, dp)
    live = (torch.arange(ld) < L)[None, :]
    return Case("srn_softmax_bwd", [p, buf, rows, L, ld, scale],
                [Out("dp", buf, ref, (ref[:, :L].pow(2).mean(-1, keepdim=True)).sqrt(), written=live)])


# ------------------------------------------------------------------------------------------------ element-wise
def _geglu_hg(rows, inner):
    r = _Rng(f"geglu{rows}-{inner}")
    hg = r.n(rows, 2 * inner)
    g = (r.n(rows, inner) * 5).clamp(-12, 12)  # gate values out to +-12
    g.view(-1)[0], g.view(-1)[-1] = 12.0, -12.0
    hg[:, inner:] = g
    return r, hg


def _geglu_shapes():
    for inner in (4, 128, 2048):
        for rows in (1, 3, 70):
            yield rows, inner
    yield 8200, 2048  # past the 16384-workgroup cap: the grid-stride loop


@sweep("srn_geglu_fwd")
def _sw_geglu_fwd():
    for rows, inner in _geglu_shapes():
        yield f"rows{rows}-inner{inner}", (lambda rows=rows, inner=inner: _mk_geglu(rows, inner, False))


@sweep("srn_geglu_bwd")
def _sw_geglu_bwd():
    for rows, inner in _geglu_shapes():
        yield f"rows{rows}-inner{inner}", (lambda rows=rows, inner=inner: _mk_geglu(rows, inner, True))


def _mk_geglu(rows, inner, bwd):
    r, hg = _geglu_hg(rows, inner)
    h64 = hg.double().requires_grad_(True)
    a64 = h64[:, :inner] * F.gelu(h64[:, inner:])
    if not bwd:
        a = Buf(rows * inner)
        a64 = a64.detach()
        return Case("srn_geglu_fwd", [hg, a, rows, inner], [Out("a", a, a64, rms(a64, (0, 1)))])
    da = r.n(rows, inner)
    a64.backward(da.double())
    dhg = Buf(rows * 2 * inner)
    return Case("srn_geglu_bwd", [hg, da, dhg, rows, inner], [Out("dhg", dhg, h64.grad, rms(h64.grad, (0, 1)))])


ADAM_N = (1, 3, 4, 1023, 1025, (1 << 20) + 5)


def _adamw_shapes():
    k = 0
    for n in ADAM_N:
        for step in (1, 1000):
            yield n, step, (0.0, 0.01)[k % 2], (0.37, 1.0, 2.5)[k % 3]
            k += 1


def _adamw_case(op, n, step, wd, gscale):
    r = _Rng(f"adam{n}-{step}")
    p, g, m, v = r.n(n), 0.1 * r.n(n), 0.01 * r.n(n), 1e-3 * r.u(n)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    L, B1, B2, E, W, GS = (f32(t) for t in (lr, b1, b2, eps, wd, gscale))
    if op == "srn_adamw_dyn":
        dyn = torch.tensor([lr, 1 - b1 ** step, 1 - b2 ** step, gscale], dtype=torch.float32)
        L, bc1, bc2, GS = (float(t) for t in dyn.double())
    else:
        bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    gi = g.double() * GS
    m64 = B1 * m.double() + (1 - B1) * gi
    v64 = B2 * v.double() + (1 - B2) * gi * gi
    p64 = p.double() * (1 - L * W) - (L / bc1) * m64 / ((v64 / bc2).sqrt() + E)
    pb, mb, vb = Buf(n, p), Buf(n, m), Buf(n, v)
    if op == "srn_adamw_dyn":
        args = [pb, g, mb, vb, n, b1, b2, eps, wd, dyn]
    else:
        args = [pb, g, mb, vb, n, lr, b1, b2, eps, wd, step, gscale]
    outs = [Out(nm, b, t, rms(t, 0)) for nm, b, t in (("p", pb, p64), ("m", mb, m64), ("v", vb, v64))]
    return Case(op, args, outs)


def _sw_adamw(op):
    def gen():
        for n, step, wd, gs in _adamw_shapes():
            yield f"n{n}-step{step}-wd{wd}-gscale{gs}", (lambda n=n, step=step, wd=wd, gs=gs: _adamw_case(op, n, step, wd, gs))
    return gen


SWEEPS["srn_adamw"] = _sw_adamw("srn_adamw")
SWEEPS["srn_adamw_dyn"] = _sw_adamw("srn_adamw_dyn")


def sumsq_blocks(n):
    """srn_sumsq_blocks (pinned against the library by test_hip_rowops.py)"""
    return max(1, min(1024, ((n + 7) // 8 + 255) // 256))


def _dot_case(op, n, second):
    r = _Rng(f"dot{n}")
    a = r.n(n) + 0.3
    b = r.n(n) + 0.3 if second else None
    if op == "srn_sumsq":
        total = (a.double() ** 2).sum()
    else:
        total = (a.double() * (b.double() if second else 1.0)).sum()
    nb = sumsq_blocks(n)
    part = Buf(1024, dtype=torch.float64)  # the caller's 1024 doubles; the first srn_sumsq_blocks(n) are written

    def total_err(g):  # in units of the 1e-12 relative bound's left-hand side
        return (g.view(-1)[:nb].sum() - total).abs() / total.abs()

    # the individual partials are free (their sum is the contract); the entries past them are not written
    out = Out("partial", part, torch.zeros(1024, dtype=torch.float64), written=torch.arange(1024) < nb, free=True,
              extra=total_err)
    args = [a, n, part] if op == "srn_sumsq" else [a, b, n, part]
    return Case(op, args, [out])


@sweep("srn_sumsq")
def _sw_sumsq():
    for n in ADAM_N + ((1 << 21) + 7,):  # the last: past the 1024-block cap
        yield f"n{n}", (lambda n=n: _dot_case("srn_sumsq", n, False))


@sweep("srn_dot")
def _sw_dot():
    for n in ADAM_N + ((1 << 21) + 7,):
        for second in (True, False):
            yield f"n{n}-b{int(second)}", (lambda n=n, second=second: _dot_case("srn_dot", n, second))


@sweep("srn_colsum")
def _sw_colsum():
    k = 0
    for R in (1, 31, 32, 33, 64, 65, 100):
        for N in (1, 255, 256, 257):
            B = (1, 3)[k % 2]
            ld = N + (3, 0, 5)[k % 3]
            yield f"B{B}-R{R}-N{N}-ld{ld}", (lambda B=B, R=R, N=N, ld=ld: _mk_colsum(B, R, N, ld))
            k += 1


def _mk_colsum(B, R, N, ld):
    r = _Rng(f"colsum{B}-{R}-{N}-{ld}")
    x = r.n(B, R, ld) + 0.2
    ref = x.double()[:, :, :N].sum(1)
    part, out = Buf(B * ((R + 31) // 32) * N), Buf(B * N)
    return Case("srn_colsum", [x, part, out, B, R, N, ld],
                [Out("partial", part, scratch=True), Out("out", out, ref, rms(ref, -1))])


@sweep("srn_sinusoidal_emb")
def _sw_sinusoidal():
    for n, dim, ld in ((1, 4, 4), (4, 242, 256), (5, 256, 256), (300, 6, 9), (77, 64, 64)):
        yield f"n{n}-dim{dim}-ld{ld}", (lambda n=n, dim=dim, ld=ld: _mk_sinusoidal(n, dim, ld))


def _mk_sinusoidal(n, dim, ld):
    t = torch.cat([torch.tensor([0.0, 0.1, 0.3, 0.9, 1.0]), _Rng(f"sin{n}").u(max(0, n - 5))])[:n].contiguous()
    half = dim // 2
    # decoder.py:58-62 in fp64 on the fp32 inputs: arguments reach scale * t = 1e3, where one ulp of the fp32 argument
    # is 6e-5 -- the fp32 restatement's error, and so this op's tolerance, is that argument rounding
    f = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000.0) / (half - 1)))
    arg = 1000.0 * t.double()[:, None] * f[None]
    ref = torch.zeros(n, ld, dtype=torch.float64)
    ref[:, :half], ref[:, half:dim] = arg.sin(), arg.cos()
    out = Buf(n * ld)
    return Case("srn_sinusoidal_emb", [t, out, n, dim, ld, 1000.0],
                [Out("out", out, ref, rms(ref[:, :dim], -1), written=(torch.arange(ld) < dim)[None, :])])


@sweep("srn_renorm")
def _sw_renorm():
    for rows, C, trg in ((1, 1, True), (50, 80, True), (50, 80, False), (7, 3, True), (13200, 80, True)):
        yield f"rows{rows}-C{C}-trg{int(trg)}", (lambda rows=rows, C=C, trg=trg: _mk_renorm(rows, C, trg))


def _mk_renorm(rows, C, trg):
    r = _Rng(f"renorm{rows}-{C}")
    x = r.n(rows, C)
    ts, tm = (0.5 + r.u(C), 0.1 * r.n(C)) if trg else (None, None)
    vm, vs = 0.1 * r.n(C), 0.5 + r.u(C)
    v = x.double() * ts.double() + tm.double() if trg else x.double()
    ref = (v - vm.double()) / vs.double()
    y = Buf(rows * C)
    return Case("srn_renorm", [x, ts, tm, vm, vs, y, rows, C], [Out("y", y, ref, rms(ref, (0, 1)))])


@sweep("srn_out_conv_tanh")
def _sw_out_conv_tanh():
    for T in (1, 255, 256, 257, 300):
        yield f"C32k7-T{T}", (lambda T=T: _mk_out_conv(2, T, 32, 7, 0))
    yield "C32k7-T300-unaligned", lambda: _mk_out_conv(2, 300, 32, 7, 1)  # not 16-byte aligned: the generic kernel
    yield "C16k5-T300", lambda: _mk_out_conv(2, 300, 16, 5, 0)
    yield "C8k3-T300", lambda: _mk_out_conv(3, 300, 8, 3, 0)
    yield "reject-k4", lambda: _mk_out_conv(1, 9, 8, 4, 0, error="bad args")


def _mk_out_conv(B, T, C, k, off, error=None):
    r = _Rng(f"oct{B}-{T}-{C}-{k}")
    x = r.n(off + B * T * C)
    w, bias = r.n(k, C) * 0.2, r.n(1)
    slope = 0.01
    xv = F.leaky_relu(x.double()[off:].reshape(B, T, C), f32(slope)).transpose(1, 2)
    y = Buf(B * T)
    if error:
        out = Out("y", y, torch.zeros(B, T, dtype=torch.float64), written=torch.zeros((), dtype=torch.bool))
    else:
        ref = torch.tanh(F.conv1d(xv, w.double().t().unsqueeze(0), bias.double(), padding=(k - 1) // 2))[:, 0]
        out = Out("y", y, ref, rms(ref, (0, 1)))
    return Case("srn_out_conv_tanh", [(x, off) if off else x, w, bias, y, B, T, C, k, slope], [out], error=error)


@sweep("srn_pd_gather")
def _sw_pd_gather():
    for B, T, C, dil in ((1, 1, 4, 1.0), (2, 37, 32, 2.5), (2, 300, 36, 1.0), (1, 2100, 128, 2.5)):
        yield f"B{B}-T{T}-C{C}-dil{dil}", (lambda B=B, T=T, C=C, dil=dil: _mk_pd_gather(B, T, C, dil))


def _mk_pd_gather(B, T, C, dil):
    r = _Rng(f"pdg{B}-{T}-{C}")
    x = r.n(B, T, C)
    # d * dilation stays clear of the .5 ties of rint
    d = (torch.floor(r.u(B, T) * 12) + (r.u(B, T) - 0.5) * 0.3) / dil
    slope = 0.1
    xv = F.leaky_relu(x.double(), f32(slope))
    rr = torch.round(d.double() * dil).long()
    assert bool(((d.double() * dil - rr).abs() < 0.2).all())
    t = torch.arange(T)[None]
    ref = torch.zeros(B, T, 3 * C, dtype=torch.float64)
    ref[:, :, :C] = xv
    for j, idx in ((1, t - rr), (2, t + rr)):
        ok = ((idx >= 0) & (idx < T)).unsqueeze(-1)
        ref[:, :, j * C:(j + 1) * C] = torch.gather(xv, 1, idx.clamp(0, T - 1).unsqueeze(-1).expand(B, T, C)) * ok
    out = Buf(B * T * 3 * C)
    return Case("srn_pd_gather", [x, d, out, B, T, C, dil, slope], [Out("out", out, ref, rms(ref, (0, 1, 2)))])


# ------------------------------------------------------------------------------------------------ data movement
@sweep("srn_copy_channels")
def _sw_copy_channels():
    for B, T, C, lds, sc0, ldd, dc0 in ((2, 9, 3, 5, 1, 16, 3), (1, 1, 1, 1, 0, 1, 0), (3, 33, 80, 96, 16, 81, 1),
                                        (1, 4100, 257, 257, 0, 260, 3)):  # the last: past the 4096-workgroup cap
        yield f"B{B}-T{T}-C{C}-lds{lds}+{sc0}-ldd{ldd}+{dc0}", (lambda a=(B, T, C, lds, sc0, ldd, dc0): _mk_copy_channels(*a))


def _mk_copy_channels(B, T, C, lds, sc0, ldd, dc0):
    src = _Rng(f"cc{B}-{T}-{C}").n(B, T, lds)
    ref = torch.zeros(B, T, ldd, dtype=torch.float64)
    ref[:, :, dc0:dc0 + C] = src[:, :, sc0:sc0 + C].double()
    cols = torch.arange(ldd)
    dst = Buf(B * T * ldd)
    return Case("srn_copy_channels", [src, T * lds, lds, sc0, dst, T * ldd, ldd, dc0, B, T, C],
                [Out("dst", dst, ref, written=((cols >= dc0) & (cols < dc0 + C))[None, None, :], exact=True)])


@sweep("srn_scatter_rows")
def _sw_scatter_rows():
    yield "B2-T9-C5-off-rows", lambda: _mk_scatter(2, 9, 5, 16, 8, 2, [3, 7], [9, 4])
    yield "B2-T9-C5-noff-rows", lambda: _mk_scatter(2, 9, 5, 9, 8, 0, None, [1, 9])
    yield "B3-T33-C80-off-norows", lambda: _mk_scatter(3, 33, 80, 40, 81, 1, [0, 7, 3], None)
    yield "B1-T1030-C257", lambda: _mk_scatter(1, 1030, 257, 1040, 260, 3, [10], [1029])  # past the 1024-workgroup cap


def _mk_scatter(B, T, C, Td, ldd, dc0, row_off, n_rows):
    src = _Rng(f"sc{B}-{T}-{C}").n(B, T, C)
    ref = torch.zeros(B, Td, ldd, dtype=torch.float64)
    w = torch.zeros(B, Td, ldd, dtype=torch.bool)
    for b in range(B):
        off = 0 if row_off is None else row_off[b]
        n = T if n_rows is None else min(n_rows[b], T)
        ref[b, off:off + n, dc0:dc0 + C] = src[b, :n].double()
        w[b, off:off + n, dc0:dc0 + C] = True
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32)
    dst = Buf(B * Td * ldd)
    return Case("srn_scatter_rows", [src, T * C, C, dst, Td * ldd, ldd, dc0, i32(row_off), i32(n_rows), B, T, C],
                [Out("dst", dst, ref, written=w, exact=True)])


TR_SIZES = (1, 15, 16, 17, 33)


def _tr_entry(r, B, R, Cc, pad):
    """one transpose problem: (src, dst Buf, B, R, Cc, src_bs, ld_src, dst_bs, ld_dst), its Out"""
    lds, ldd = Cc + pad, R + 2 * pad
    src = r.n(B, R, lds)
    ref = torch.zeros(B, Cc, ldd, dtype=torch.float64)
    ref[:, :, :R] = src[:, :, :Cc].double().transpose(1, 2)
    dst = Buf(B * Cc * ldd)
    out = Out(f"dst{R}x{Cc}", dst, ref, written=(torch.arange(ldd) < R)[None, None, :], exact=True)
    return (src, dst, B, R, Cc, R * lds, lds, Cc * ldd, ldd), out


@sweep("srn_transpose_ct")
def _sw_transpose_ct():
    for R in TR_SIZES:
        for Cc in TR_SIZES:
            yield f"R{R}-Cc{Cc}", (lambda R=R, Cc=Cc: _mk_transpose_ct(R, Cc))
    yield "R80-Cc37", lambda: _mk_transpose_ct(80, 37)


def _mk_transpose_ct(R, Cc):
    e, out = _tr_entry(_Rng(f"tr{R}-{Cc}"), 2, R, Cc, (R + Cc) % 3)
    src, dst, B, R, Cc, sbs, lds, dbs, ldd = e
    return Case("srn_transpose_ct", [src, dst, B, R, Cc, sbs, lds, dbs, ldd], [out])


@sweep("srn_transpose_multi")
def _sw_transpose_multi():
    small = [(R, Cc) for R in TR_SIZES for Cc in TR_SIZES if R < 16 or Cc < 16]
    tiled = [(R, Cc) for R in TR_SIZES for Cc in TR_SIZES if R >= 16 and Cc >= 16]
    mixed = [(R, Cc) for R in TR_SIZES for Cc in TR_SIZES]  # 25 entries, both paths interleaved
    yield "narrow-only", lambda: _mk_transpose_multi(small)
    yield "tiled-only", lambda: _mk_transpose_multi(tiled)
    yield "mixed-25", lambda: _mk_transpose_multi(mixed)
    yield "one-3x1100", lambda: _mk_transpose_multi([(3, 1100)])  # the narrow path over more than one block
    yield "full-list-40", lambda: _mk_transpose_multi((mixed + small)[:40])


def _mk_transpose_multi(shapes):
    r = _Rng(f"trm{len(shapes)}")
    entries, outs = [], []
    for k, (R, Cc) in enumerate(shapes):
        e, o = _tr_entry(r, 1 + k % 2, R, Cc, k % 3)
        o.name = f"entry{k}:{R}x{Cc}"
        entries.append(e)
        outs.append(o)
    return Case("srn_transpose_multi", entries, outs, kind="transpose_multi")


COPY_LIST_MAX = 160


@sweep("srn_multi_copy")
def _sw_multi_copy():
    yield "odd-and-empty", lambda: _mk_multi_copy([7, 0, 1, 33, 4, 1021], False)
    yield "full-list-160", lambda: _mk_multi_copy([(3 * k) % 17 + (k % 5 == 0) * 40 for k in range(COPY_LIST_MAX)], False)
    yield "long-aligned", lambda: _mk_multi_copy([300000, 8, 12], True)   # several blocks per entry, float4 path
    yield "long-unaligned", lambda: _mk_multi_copy([300001, 5], False)           # the scalar path over several blocks


def _mk_multi_copy(lens, aligned):
    """sources are (pool, offset) pairs into one tensor, so that their alignment survives the copy to the device"""
    r = _Rng(f"mc{len(lens)}-{sum(lens)}")
    step = (lambda v: (v + 3) // 4 * 4 + 4) if aligned else (lambda v: v + 3)
    pool = r.n(sum(lens) + 8 * len(lens) + 16)
    srcs, offs, rng = [], [], []
    pos, dpos = (0, 8) if aligned else (1, 5)
    for n in lens:
        srcs.append((pool, pos))  # a zero-length entry still carries a valid pointer
        offs.append(dpos)
        rng.append((pos, dpos, n))
        pos, dpos = pos + step(max(n, 1)), dpos + step(n)
    total = dpos + 8
    ref = torch.zeros(total, dtype=torch.float64)
    w = torch.zeros(total, dtype=torch.bool)
    for so, do, n in rng:
        ref[do:do + n] = pool[so:so + n].double()
        w[do:do + n] = True
    dst = Buf(total)
    return Case("srn_multi_copy", (srcs, offs, list(lens), dst), [Out("dst", dst, ref, written=w, exact=True)],
                kind="multi_copy")


# ------------------------------------------------------------------------------------------------ weight norm
@sweep("srn_weight_norm_fwd")
def _sw_wn_fwd():
    for N, C, k, wd in ((3, 5, 3, True), (16, 80, 7, True), (4, 300, 1, False), (1, 1, 1, True)):
        yield f"N{N}-C{C}-k{k}-wd{int(wd)}", (lambda a=(N, C, k, wd): _mk_wn_fwd(*a))


def _wn_inputs(N, C, k):
    r = _Rng(f"wn{N}-{C}-{k}")
    return r, r.n(N, C, k) + 0.1, 0.5 + r.u(N)


def _mk_wn_fwd(N, C, k, with_wd):
    _, v, g = _wn_inputs(N, C, k)
    nrm = v.double().reshape(N, -1).norm(dim=1)
    wp = (v.double() * (g.double() / nrm).reshape(N, 1, 1)).permute(0, 2, 1).contiguous()  # (N, k, C)
    w, inv, wd = Buf(N * k * C), Buf(N), Buf(C * k * N) if with_wd else None
    outs = [Out("w", w, wp, rms(wp, (1, 2))), Out("inv_norm", inv, 1.0 / nrm, (1.0 / nrm).abs())]
    if with_wd:
        wdt = wp.permute(2, 1, 0).contiguous()
        outs.append(Out("wd", wd, wdt, rms(wp, (1, 2)).reshape(1, 1, N)))
    return Case("srn_weight_norm_fwd", [v, g, w, wd, inv, N, C, k], outs)


@sweep("srn_weight_norm_bwd")
def _sw_wn_bwd():
    for N, C, k in ((3, 5, 3), (16, 80, 7), (4, 300, 1), (2, 3, 1)):
        yield f"N{N}-C{C}-k{k}", (lambda a=(N, C, k): _mk_wn_bwd(*a))


def _mk_wn_bwd(N, C, k):
    r, v, g = _wn_inputs(N, C, k)
    dw = r.n(N, k, C)
    inv = (1.0 / v.double().reshape(N, -1).norm(dim=1)).float()
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    w = v64 * (g64 / v64.reshape(N, -1).norm(dim=1)).reshape(N, 1, 1)
    w.backward(dw.double().permute(0, 2, 1))
    dv, dg = Buf(N * C * k), Buf(N)
    return Case("srn_weight_norm_bwd", [dw, v, g, inv, dv, dg, N, C, k],
                [Out("dv", dv, v64.grad, rms(v64.grad, (1, 2))), Out("dg", dg, g64.grad, rms(g64.grad, 0))])


def _base_wn_fwd(a):
    v, g, w, wd, inv, N, C, k = a
    nrm = 1.0 / torch.sqrt((v * v).reshape(N, -1).sum(1))
    wp = (v * (g * nrm).reshape(N, 1, 1)).permute(0, 2, 1)
    w.view(N, k, C)[:] = wp
    inv[:] = nrm
    if wd is not None:
        wd.view(C, k, N)[:] = wp.permute(2, 1, 0)


def _base_wn_bwd(a):
    dw, v, g, inv, dv, dg, N, C, k = a
    dd = dw.reshape(N, k, C).permute(0, 2, 1)
    dot = (dd * v).reshape(N, -1).sum(1)
    dg[:] = dot * inv
    dv.view(N, C, k)[:] = (g * inv).reshape(N, 1, 1) * (dd - v * (dot * inv * inv).reshape(N, 1, 1))


BASELINE["srn_weight_norm_fwd"] = _base_wn_fwd
BASELINE["srn_weight_norm_bwd"] = _base_wn_bwd


# ------------------------------------------------------------------------------------------------ GST training kernels
def bn_chunks(rows):
    per = 16 if rows <= 256 * 16 else (rows + 255) // 256  # srn_bn_chunks
    return (rows + per - 1) // per


def _bn_shapes():
    k = 0
    for rows in (1, 2, 31, 32, 33, 4097):
        for C in (4, 32, 128):
            yield rows, C, k % 2 == 0
            k += 1
    yield 33, 1028, True  # more than 256 channel quads: two channel blocks in the partial-sum kernel


def _bn_inputs(rows, C):
    r = _Rng(f"bn{rows}-{C}")
    x = r.n(rows, C) * 2 + 0.3
    gamma, beta = 0.5 + r.u(C), 0.3 * r.n(C)
    beta[C // 2] = -100.0  # a column whose pre-activation is negative on every row
    return r, x, gamma, beta


def _bn_forward64(x64, gamma64, beta64, rm64, rv64, eps, mom):
    """F.batch_norm(training=True) + relu; one row: torch refuses, and the contract is variance 0 (the header)"""
    rows = x64.shape[0]
    if rows > 1:
        return torch.relu(F.batch_norm(x64, rm64, rv64, gamma64, beta64, True, mom, eps))
    mean = x64.mean(0)
    if rm64 is not None:
        rm64.mul_(1 - mom).add_(mom * mean.detach())
        rv64.mul_(1 - mom)  # + mom * 0
    return torch.relu((x64 - mean) / math.sqrt(eps) * gamma64 + beta64)


@sweep("srn_bn_relu_fwd")
def _sw_bn_fwd():
    for rows, C, run in _bn_shapes():
        yield f"rows{rows}-C{C}-run{int(run)}", (lambda a=(rows, C, run): _mk_bn_fwd(*a))
    yield "reject-C6", lambda: _mk_bn_fwd(5, 6, True, error="bad args")


def _mk_bn_fwd(rows, C, run, error=None):
    r, x, gamma, beta = _bn_inputs(rows, C)
    eps, mom = 1e-5, 0.1
    rm, rv = (0.1 * r.n(C), 0.5 + r.u(C))
    rm64, rv64 = (rm.double().clone(), rv.double().clone()) if run else (None, None)
    x64 = x.double()
    y64 = _bn_forward64(x64, gamma.double(), beta.double(), rm64, rv64, f32(eps), f32(mom))
    st64 = torch.stack([x64.mean(0), 1.0 / torch.sqrt(x64.var(0, unbiased=False) + f32(eps))])
    part, stats, y = Buf(bn_chunks(rows) * 2 * C), Buf(2 * C), Buf(rows * C)
    none = torch.zeros((), dtype=torch.bool) if error else None
    cs = rms(y64, 0).clamp_min(1e-30)
    outs = [Out("partial", part, scratch=True),
            Out("stats", stats, st64, torch.stack([rms(x64, 0, False), st64[1].abs()]), written=none),
            Out("y", y, y64, cs, written=none)]
    rmb = rvb = None
    if run:
        rmb, rvb = Buf(C, rm), Buf(C, rv)
        outs += [Out("run_mean", rmb, rm64, rms(x64, 0, False), written=none),
                 Out("run_var", rvb, rv64, rv64.abs(), written=none)]
    return Case("srn_bn_relu_fwd", [x, gamma, beta, rmb, rvb, part, stats, y, rows, C, eps, mom], outs, error=error)


@sweep("srn_bn_relu_bwd")
def _sw_bn_bwd():
    for rows, C, _ in _bn_shapes():
        yield f"rows{rows}-C{C}", (lambda a=(rows, C): _mk_bn_bwd(*a))


def _mk_bn_bwd(rows, C):
    r, x, gamma, beta = _bn_inputs(rows, C)
    dy = r.n(rows, C)
    eps = f32(1e-5)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64 = _bn_forward64(x64, g64, b64, None, None, eps, 0.1)
    y64.backward(dy.double())
    xd = x.double()
    stats = torch.stack([xd.mean(0), 1.0 / torch.sqrt(xd.var(0, unbiased=False) + eps)]).float()
    sums64 = torch.stack([b64.grad, g64.grad])
    part, sums, dx = Buf(bn_chunks(rows) * 2 * C), Buf(2 * C), Buf(rows * C)
    s_dx = rms(x64.grad, 0).clamp_min(1e-30)
    if rows <= 2:  # dx cancels to O(eps / var): the unit is the size of the terms that cancel (module docstring)
        s_dx = (gamma.double().abs() * stats[1].double() * rms(dy.double(), 0)).clamp_min(1e-30)
    # the kernel is handed the forward's y (its sign is the relu mask) and statistics, in fp32
    return Case("srn_bn_relu_bwd", [x, y64.detach().float(), dy, stats, gamma, part, sums, dx, rows, C],
                [Out("partial", part, scratch=True), Out("sums", sums, sums64, rms(sums64, -1)),
                 Out("dx", dx, x64.grad, s_dx, ill=torch.ones((), dtype=torch.bool) if rows == 2 else None)])


def _base_bn_fwd(a):
    """fp32 with the kernel's formula: column sums of x - x[0] and of its square, variance as their E[d^2] - E[d]^2"""
    x, gamma, beta, rm, rv, part, stats, y, rows, C, eps, mom = a
    d = x - x[0]
    s0, s1 = d.sum(0), (d * d).sum(0)
    mean = x[0] + s0 / rows
    var = (s1 / rows - (s0 / rows) ** 2).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    stats.view(2, C)[0], stats.view(2, C)[1] = mean, rstd
    y.view(rows, C)[:] = torch.relu((x - mean) * rstd * gamma + beta)
    if rm is not None:
        unb = var * (rows / (rows - 1)) if rows > 1 else var
        rm.mul_(1 - mom).add_(mom * mean)
        rv.mul_(1 - mom).add_(mom * unb)


def _base_bn_bwd(a):
    x, y, dy, stats, gamma, part, sums, dx, rows, C = a
    st = stats.view(2, C)
    g = dy * (y > 0)
    xhat = (x - st[0]) * st[1]
    s0, s1 = g.sum(0), (g * xhat).sum(0)
    sums.view(2, C)[0], sums.view(2, C)[1] = s0, s1
    dx.view(rows, C)[:] = gamma * st[1] * (g - (s0 + xhat * s1) / rows)


BASELINE["srn_bn_relu_fwd"] = _base_bn_fwd
BASELINE["srn_bn_relu_bwd"] = _base_bn_bwd


IM_HW = ((1, 1), (1, 2), (2, 1), (2, 5), (5, 2), (5, 80), (80, 5), (80, 80), (80, 1))


def im2col_shapes():
    k = 0
    for H, W in IM_HW:
        C = (4, 32)[k % 2]
        B = (1, 2)[(k // 2) % 2]
        yield B, H, W, C, 9 * C + 4 * (k % 2 == 0)
        k += 1
    yield 2, 5, 5, 32, 9 * 32 + 4
    yield 1, 2, 2, 4, 9 * 4


def _unfold64(x64):
    """(B, H, W, C) -> (B, Ho, Wo, 9 C) in (kh, kw, c) order, by F.unfold"""
    B, H, W, C = x64.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    u = F.unfold(x64.permute(0, 3, 1, 2), 3, padding=1, stride=2)  # (B, C * 9, Ho * Wo), rows ordered (c, kh, kw)
    return u.reshape(B, C, 9, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(B, Ho, Wo, 9 * C)


@sweep("srn_im2col_s2")
def _sw_im2col():
    for B, H, W, C, ld in im2col_shapes():
        yield f"B{B}-H{H}-W{W}-C{C}-ld{ld}", (lambda a=(B, H, W, C, ld): _mk_im2col(*a))
    yield "reject-ld-short", lambda: _mk_im2col(1, 5, 5, 8, 68, error="bad args")


def _mk_im2col(B, H, W, C, ld, error=None):
    x = _Rng(f"im{B}-{H}-{W}-{C}").n(B, H, W, C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ref = torch.zeros(B, Ho, Wo, ld, dtype=torch.float64)
    if not error:
        ref[..., :9 * C] = _unfold64(x.double())
    col = Buf(B * Ho * Wo * ld)
    w = torch.zeros((), dtype=torch.bool) if error else (torch.arange(ld) < 9 * C)[None, None, None, :]
    return Case("srn_im2col_s2", [x, col, B, H, W, C, ld], [Out("col", col, ref, written=w, exact=True)], error=error)


@sweep("srn_col2im_s2")
def _sw_col2im():
    for B, H, W, C, ld in im2col_shapes():
        yield f"B{B}-H{H}-W{W}-C{C}-ld{ld}", (lambda a=(B, H, W, C, ld): _mk_col2im(*a))


def _mk_col2im(B, H, W, C, ld):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    col = _Rng(f"c2i{B}-{H}-{W}-{C}").n(B, Ho, Wo, ld)  # the pad columns hold data the kernel must not read
    c64 = col.double()[..., :9 * C].reshape(B, Ho * Wo, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, Ho * Wo)
    ref = F.fold(c64, (H, W), 3, padding=1, stride=2).permute(0, 2, 3, 1).contiguous()  # (B, H, W, C)
    x = _Rng("adj").n(B, H, W, C).double()  # the adjoint of the gather: <im2col(x), c> == <x, col2im(c)>
    lhs, rhs = (_unfold64(x) * col.double()[..., :9 * C]).sum(), (x * ref).sum()
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))
    dx = Buf(B * H * W * C)
    return Case("srn_col2im_s2", [col, dx, B, H, W, C, ld], [Out("dx", dx, ref, rms(ref, (0, 1, 2, 3)))])


def adjoint_pair(shape, run, dev):
    """(<im2col(x), c>, <x, col2im(c)>) in fp64 from the outputs of the two calls; run(case, args) makes a call"""
    B, H, W, C, ld = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ci, cc = _mk_im2col(B, H, W, C, ld), _mk_col2im(B, H, W, C, ld)
    got = []
    for case in (ci, cc):
        args, bufs = materialize(case, dev)
        run(case, args)
        got.append(bufs[id(case.outs[0].buf)].cpu()[G:-G].double())
    col = got[0].view(B, Ho, Wo, ld)[..., :9 * C]
    dx = got[1].view(B, H, W, C)
    x, c = ci.args[0].double(), cc.args[0].double()[..., :9 * C]
    return float((col * c).sum()), float((x * dx).sum())


def _gru_inputs(B, T, H):
    r = _Rng(f"gru{B}-{T}-{H}")
    gi = r.n(B, T, 3 * H)
    w_hh = r.n(3 * H, H) / math.sqrt(H)
    b_hh = 0.1 * r.n(3 * H)
    return r, gi, w_hh, b_hh


def _gru_forward64(gi, w_hh, b_hh, grad=False):
    """the recurrence in fp64, step by step (the gates are outputs); equal to torch.nn.GRU, checked by the caller"""
    B, T, G3 = gi.shape
    H = G3 // 3
    h = torch.zeros(B, H, dtype=torch.float64)
    hs, gates, ghs = [h], [], []
    for t in range(T):
        gh = h @ w_hh.t() + b_hh
        if grad:  # a zero added to W_hh h + b_hh: its gradient is dgh of this step
            ghs.append(torch.zeros(B, G3, dtype=torch.float64, requires_grad=True))
            gh = gh + ghs[-1]
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs.append(h)
        gates.append(torch.cat([r, z, n, gh[:, 2 * H:]], dim=1))
    return torch.stack(hs, 1), torch.stack(gates, 1), ghs


def _nn_gru64(gi, w_hh, b_hh):
    """torch.nn.GRU in fp64 with the same weights; the hoisted input projection enters through W_ih = I, b_ih = 0"""
    H = w_hh.shape[1]
    gru = torch.nn.GRU(3 * H, H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H, dtype=torch.float64))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(w_hh)
        gru.bias_hh_l0.copy_(b_hh)
    return gru(gi)[0]


def _gru_shapes():
    for H in (32, 128, 340):
        for T in (1, 2, 5, 64):
            yield (1, 3)[(T + H // 32) % 2], T, H
    yield 3, 1, 32
    yield 1, 64, 340
    yield 3, 5, 128


@sweep("srn_gru_train_fwd")
def _sw_gru_fwd():
    for B, T, H in sorted(set(_gru_shapes())):
        yield f"B{B}-T{T}-H{H}", (lambda a=(B, T, H): _mk_gru_fwd(*a))
    yield "reject-H344", lambda: _mk_gru_fwd(1, 2, 344, error="bad args")


def _mk_gru_fwd(B, T, H, error=None):
    _, gi, w_hh, b_hh = _gru_inputs(B, T, H)
    with torch.no_grad():
        hs64, gates64, _ = _gru_forward64(gi.double(), w_hh.double(), b_hh.double())
        assert float((hs64[:, 1:] - _nn_gru64(gi.double(), w_hh.double(), b_hh.double())).abs().max()) < 1e-12
    hs, gates = Buf(B * (T + 1) * H), Buf(B * T * 4 * H)
    none = torch.zeros((), dtype=torch.bool) if error else None
    first = torch.zeros(1, T + 1, 1, dtype=torch.bool)
    first[0, 0, 0] = True  # the zero initial state is written, exactly
    return Case("srn_gru_train_fwd", [gi, w_hh.t().contiguous(), b_hh, hs, gates, B, T, H],
                [Out("hs", hs, hs64, rms(hs64, -1), written=none, zero=None if error else first),
                 Out("gates", gates, gates64, rms(gates64, -1), written=none)], error=error)


@sweep("srn_gru_train_bwd")
def _sw_gru_bwd():
    for B, T, H in sorted(set(_gru_shapes())):
        yield f"B{B}-T{T}-H{H}", (lambda a=(B, T, H): _mk_gru_bwd(*a))


def _mk_gru_bwd(B, T, H):
    r, gi, w_hh, b_hh = _gru_inputs(B, T, H)
    dh_last = r.n(B, H)
    gi64 = gi.double().requires_grad_(True)
    hs64, gates64, ghs = _gru_forward64(gi64, w_hh.double(), b_hh.double(), grad=True)
    hs64[:, -1].backward(dh_last.double())
    dgi64 = gi64.grad
    dgh64 = torch.stack([g.grad for g in ghs], 1)
    dgi, dgh = Buf(B * T * 3 * H), Buf(B * T * 3 * H)
    # the kernel back-propagates from the forward's saved states and gates, in fp32
    return Case("srn_gru_train_bwd", [dh_last, w_hh, hs64.detach().float(), gates64.detach().float(), dgi, dgh, B, T, H],
                [Out("dgi", dgi, dgi64, rms(dgi64, -1)), Out("dgh", dgh, dgh64, rms(dgh64, -1))])


def _attn_inputs(B, n_tok, Fd, nh):
    r = _Rng(f"ta{B}-{n_tok}-{Fd}-{nh}")
    return r, r.n(B, Fd), r.n(n_tok, Fd), r.n(n_tok, Fd)


def _attn64(q, k, v, nh):
    B, Fd = q.shape
    n_tok, dk = k.shape[0], Fd // nh
    sc = torch.einsum("bhd,thd->bht", q.view(B, nh, dk), k.view(n_tok, nh, dk)) / math.sqrt(dk)
    p = torch.softmax(sc, -1)
    return p, torch.einsum("bht,thd->bhd", p, v.view(n_tok, nh, dk)).reshape(B, Fd)


def _attn_shapes():
    k = 0
    for n_tok in (1, 10):
        for nh in (1, 4):
            for Fd in (64, 256):
                yield (1, 3)[k % 2], n_tok, Fd, nh
                k += 1
    yield 2, 50, 256, 4  # the product's shape


@sweep("srn_token_attn_fwd")
def _sw_attn_fwd():
    for a in _attn_shapes():
        yield "B{}-tok{}-F{}-h{}".format(*a), (lambda a=a: _mk_attn_fwd(*a))
    yield "lds-limit-B2-tok4032-F256-h4", lambda: _mk_attn_fwd(2, 4032, 256, 4)     # (F + h * tok) * 4 = 64 KiB exactly
    yield "reject-lds-B2-tok4033-F256-h4", lambda: _mk_attn_fwd(2, 4033, 256, 4, error="LDS")


def _mk_attn_fwd(B, n_tok, Fd, nh, error=None):
    _, q, k, v = _attn_inputs(B, n_tok, Fd, nh)
    p64, ctx64 = _attn64(q.double(), k.double(), v.double(), nh)
    p, ctx = Buf(B * nh * n_tok), Buf(B * Fd)
    none = torch.zeros((), dtype=torch.bool) if error else None
    return Case("srn_token_attn_fwd", [q, k, v, p, ctx, B, n_tok, Fd, nh],
                [Out("p", p, p64, rms(p64, -1), written=none), Out("ctx", ctx, ctx64, rms(ctx64, -1), written=none)],
                error=error)


@sweep("srn_token_attn_bwd")
def _sw_attn_bwd():
    for a in _attn_shapes():
        yield "B{}-tok{}-F{}-h{}".format(*a), (lambda a=a: _mk_attn_bwd(*a))
    yield "lds-limit-B2-tok1984-F256-h4", lambda: _mk_attn_bwd(2, 1984, 256, 4)   # (2 F + 2 h * tok) * 4 = 64 KiB exactly
    yield "reject-lds-B2-tok1985-F256-h4", lambda: _mk_attn_bwd(2, 1985, 256, 4, error="LDS")


def _mk_attn_bwd(B, n_tok, Fd, nh, error=None):
    r, q, k, v = _attn_inputs(B, n_tok, Fd, nh)
    dctx = r.n(B, Fd)
    q64 = q.double().requires_grad_(True)
    # per-item key / value gradients: one copy of k, v per item
    k64 = k.double()[None].repeat(B, 1, 1).requires_grad_(True)
    v64 = v.double()[None].repeat(B, 1, 1).requires_grad_(True)
    dk = Fd // nh
    sc = torch.einsum("bhd,bthd->bht", q64.view(B, nh, dk), k64.view(B, n_tok, nh, dk)) / math.sqrt(dk)
    p64 = torch.softmax(sc, -1)
    ctx = torch.einsum("bht,bthd->bhd", p64, v64.view(B, n_tok, nh, dk)).reshape(B, Fd)
    ctx.backward(dctx.double())
    dq, dkp, dvp = Buf(B * Fd), Buf(B * n_tok * Fd), Buf(B * n_tok * Fd)
    none = torch.zeros((), dtype=torch.bool) if error else None
    # the kernel is handed the forward's softmax weights, in fp32
    return Case("srn_token_attn_bwd", [dctx, q, k, v, p64.detach().float().contiguous(), dq, dkp, dvp, B, n_tok, Fd, nh],
                [Out("dq", dq, q64.grad, rms(q64.grad, -1), written=none),
                 Out("dk_part", dkp, k64.grad, rms(k64.grad, -1).clamp_min(1e-300), written=none),
                 Out("dv_part", dvp, v64.grad, rms(v64.grad, -1).clamp_min(1e-300), written=none)], error=error)


# ------------------------------------------------------------------------------------------------ measuring the table
def baseline_error(op, cid):
    case = make(op, cid)
    args, bufs = materialize(case)
    run_baseline(case, args)
    return check_outputs(case, bufs)


def _main():
    import sys
    ops_ = sys.argv[1:] or list(SWEEPS)
    for op in ops_:
        if op in FIXED_TOL or op in EXACT_OPS:
            continue
        worst, per_case = 0.0, {}
        for cid in case_ids(op):
            if cid.startswith("reject-"):
                continue
            e, e_ill = baseline_error(op, cid)
            worst = max(worst, e)
            if ill_conditioned(op, cid):
                per_case[cid] = e_ill
        print(f"TOL    {op!r}: ({worst:.3e}, {_round_up(max(4 * worst, FLOOR)):.1e}),", flush=True)
        for cid, e in per_case.items():
            print(f"CASE   ({op!r}, {cid!r}): ({e:.3e}, {_round_up(max(4 * e, FLOOR)):.1e}),", flush=True)


def _round_up(v):
    e = math.floor(math.log10(v))
    return math.ceil(v / 10 ** e * 10 - 1e-9) / 10 * 10 ** e


if __name__ == "__main__":
    _main()
