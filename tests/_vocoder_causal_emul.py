"""TEST-ONLY executable specification of the entry points of the causal vocoder (include/serenade_hip.h:
srn_hifigan_resunit_causal, srn_out_conv_tanh_causal, srn_replicate_first_row), on top of tests/_emulator.py.

``installed()`` is ``_emulator.installed()`` plus these three (and srn_zero_rows_ragged, borrowed from
tests/_serenade_ragged_emul.py: a causal generator's ragged calls end on it).  The residual unit is stated the way the
header states it: item b is the unit applied to an utterance that starts v_b = clamp(lead[b], 0, H) rows before the
call's first row -- the item's rows [H - v_b, H + T) are cut out, both convs are left-padded with zeros over exactly those
rows, and the last T rows of the result are the call's.  Rows before H - v_b are never touched, whatever they hold.
``causal_unit`` takes the dtype, so the GPU tests use the same statement in float64 as their reference.  Like the
emulator it wraps, this is never importable from the product and is not a fallback.
"""
import torch

from serenade_amd import ops
from tests import _emulator
from tests._serenade_ragged_emul import emul_zero_rows_ragged


def _lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def _causal_conv(a, w, b, k, d):
    """a (n, C) rows of ONE utterance from its row 0 -> (n, C): out[t] = b + sum_j w[:, j] a[t - (k - 1 - j) d], zero
    before row 0.  w: packed [C_out][k][C_in].  Also returns sum_j |w[:, j]| |a[..]| (the size of the terms summed)."""
    n, C = a.shape
    pad = torch.cat([torch.zeros((k - 1) * d, C, dtype=a.dtype), a])
    A = torch.stack([pad[j * d:j * d + n] for j in range(k)], dim=1).reshape(n, k * C)
    W = w.reshape(w.shape[0], k * C)
    return A @ W.t() + b, A.abs() @ W.abs().t()


def causal_unit(kw, dt=torch.float32):
    """the contract of srn_hifigan_resunit_causal in dtype dt: [(y, s)] per item, y and s (T, C) -- the value of every
    output element and the size of the terms summed into it (the bound of tests/_mfma_cases.py's residual unit:
    (|lrelu(xt)| (*) |w2|) + |b2| + |x| + |res2|, divided by post_div where it divides)"""
    g = kw.get
    B, T, C, k, d = g("n_batch"), g("T"), g("C"), g("k"), g("dilation")
    slope = float(torch.tensor(float(g("slope")), dtype=torch.float32))
    pdiv = float(torch.tensor(float(g("post_div", 0.0) or 0.0), dtype=torch.float32))
    H = (k - 1) * (d + 1)
    xf, xo = _emulator._flat(g("x"))
    x_bs = g("x_bs") or (H + T) * C
    w1, w2 = g("w1").reshape(C, k, C).to(dt), g("w2").reshape(C, k, C).to(dt)
    b1, b2 = g("b1").to(dt), g("b2").to(dt)
    lead = g("lead").view(-1)
    qf, qo = _emulator._flat(g("res2")) if g("res2") is not None else (None, 0)
    q_bs = g("res2_bs") or T * C
    out = []
    for b in range(B):
        v = max(0, min(int(lead[b]), H))
        base = xo + b * x_bs + (H - v) * C
        x = xf[base:base + (v + T) * C].reshape(v + T, C).to(dt)  # the utterance so far: nothing before it is touched
        xt, _ = _causal_conv(_lrelu(x, slope), w1, b1, k, d)
        y, s = _causal_conv(_lrelu(xt, slope), w2, b2, k, 1)
        y, s = (y + x)[v:], (s + b2.abs() + x.abs())[v:]
        if qf is not None:
            q = qf[qo + b * q_bs:qo + b * q_bs + T * C].reshape(T, C).to(dt)
            y, s = y + q, s + q.abs()
        if pdiv not in (0.0, 1.0):
            y, s = y / pdiv, s / abs(pdiv)
        out.append((y, s))
    return out


def emul_resunit_causal(kw):
    g = kw.get
    T, C = g("T"), g("C")
    of, oo = _emulator._flat(g("out"))
    o_bs = g("out_bs") or T * C
    for b, (y, _) in enumerate(causal_unit(kw)):  # every item is read before any is written: res2 may be out
        of[oo + b * o_bs:oo + b * o_bs + T * C] = y.reshape(-1)


def out_conv_tanh_causal(x, w, bias, B, T, C, k, slope, dt=torch.float32):
    """the contract of srn_out_conv_tanh_causal in dtype dt -> (y (B, T), the pre-activation's term sizes (B, T))"""
    xv = _lrelu(_emulator._v(x, B * (k - 1 + T) * C).reshape(B, k - 1 + T, C).to(dt), slope)
    wv = _emulator._v(w, k * C).reshape(k, C).to(dt)
    A = torch.stack([xv[:, i:i + T] for i in range(k)], dim=2).reshape(B, T, k * C)
    pre = A @ wv.reshape(-1) + bias.view(-1)[0].to(dt)
    return torch.tanh(pre), A.abs() @ wv.reshape(-1).abs() + bias.view(-1)[0].to(dt).abs()


def emul_out_conv_tanh_causal(a):
    x, w, bias, y, B, T, C, k, slope = a
    _emulator._v(y, B * T).reshape(B, T)[:] = out_conv_tanh_causal(x, w, bias, B, T, C, k, slope)[0]


def emul_replicate_first_row(a):
    """srn_replicate_first_row: where lead[b] <= 0, row 0 of item b becomes its row 1; other items are not touched"""
    x, bs, n_cols, lead, B = a
    assert B == 1 or bs >= 2 * n_cols, "items overlap"
    f, o = _emulator._flat(x)
    lead = lead.view(-1)
    for b in range(B):
        if int(lead[b]) <= 0:
            f[o + b * bs:o + b * bs + n_cols] = f[o + b * bs + n_cols:o + b * bs + 2 * n_cols].clone()


_CALLS = {"srn_out_conv_tanh_causal": emul_out_conv_tanh_causal, "srn_replicate_first_row": emul_replicate_first_row,
          "srn_zero_rows_ragged": emul_zero_rows_ragged}


class installed(_emulator.installed):
    """_emulator.installed() that also knows the causal vocoder's ops"""

    def __enter__(self):
        super().__enter__()
        base_call = ops.CallOp.__call__  # the emulator's

        def call(self_, stream=None):
            if self_.name in _CALLS:
                _CALLS[self_.name](self_.targs)
            else:
                base_call(self_, stream)
        ops.CallOp.__call__ = call
        base_unit = ops.ResUnitOp.__call__  # the emulator's

        def unit(self_, stream=None):
            if self_.name == "srn_hifigan_resunit_causal":
                emul_resunit_causal(self_.kw)
            else:
                base_unit(self_, stream)
        ops.ResUnitOp.__call__ = unit
        return self  # (_emulator.installed.__exit__ restores both __call__s as they were before both layers)
