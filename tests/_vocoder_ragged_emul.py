"""TEST-ONLY executable specification of the two ragged vocoder entry points (include/serenade_hip.h:
srn_hifigan_resunit_ragged, srn_out_conv_tanh_ragged), on top of tests/_emulator.py.

``installed()`` is ``_emulator.installed()`` plus these two: each is stated as the dense specification applied to one
item at a time, on the item's own rows only -- rows at or past an item's length are neither read (whatever they hold)
nor, for the residual unit, written; the output stage writes zeros there.  Like the emulator it wraps, this is never
importable from the product and is not a fallback.
"""
import torch

from serenade_amd import ops
from tests import _emulator


def _item(t, off):
    """`t` (tensor or (tensor, element offset)) moved on by `off` elements"""
    if t is None:
        return None
    if isinstance(t, tuple):
        return (t[0], t[1] + off)
    return (t, off)


def emul_resunit_ragged(kw):
    """srn_hifigan_resunit_ragged: item b = the dense unit with n_batch = 1, T = min(lens[b], T) on that item alone;
    output rows at or past the length keep what they held"""
    g = kw.get
    B, T, C = g("n_batch"), g("T"), g("C")
    lens = g("lens").view(-1)
    step = lambda name: T * C if g(name) is None else g(name)
    for b in range(B):
        L = min(int(lens[b]), T)
        assert L >= 1, "lens: each >= 1"
        one = {k: v for k, v in kw.items() if k != "lens"}
        one.update(n_batch=1, T=L, x=_item(g("x"), b * step("x_bs")), out=_item(g("out"), b * step("out_bs")),
                   res2=_item(g("res2"), b * step("res2_bs")), x_bs=L * C, out_bs=L * C, res2_bs=L * C)
        _emulator.emul_resunit(one)


def emul_out_conv_tanh_ragged(a):
    """srn_out_conv_tanh_ragged: item b = the dense stage with B = 1, T = min(lens[b], T) on that item's rows; zeros
    behind them"""
    x, w, bias, y, lens, B, T, C, k, slope = a
    lens = lens.view(-1)
    yv = _emulator._v(y, B * T).reshape(B, T)
    for b in range(B):
        L = min(int(lens[b]), T)
        assert L >= 1, "lens: each >= 1"
        _emulator.emul_call("srn_out_conv_tanh", (_item(x, b * T * C), w, bias, _item(y, b * T), 1, L, C, k, slope))
        yv[b, L:] = 0


class installed(_emulator.installed):
    """_emulator.installed() that also knows the two ragged ops"""

    def __enter__(self):
        super().__enter__()
        base_call = ops.CallOp.__call__  # the emulator's

        def call(self_, stream=None):
            if self_.name == "srn_out_conv_tanh_ragged":
                emul_out_conv_tanh_ragged(self_.targs)
            else:
                base_call(self_, stream)
        ops.CallOp.__call__ = call
        base_unit = ops.ResUnitOp.__call__  # the emulator's

        def unit(self_, stream=None):
            if self_.name == "srn_hifigan_resunit_ragged":
                emul_resunit_ragged(self_.kw)
            else:
                base_unit(self_, stream)
        ops.ResUnitOp.__call__ = unit
        return self  # (_emulator.installed.__exit__ restores both __call__s as they were before both layers)
