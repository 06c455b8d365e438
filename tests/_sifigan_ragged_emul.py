"""TEST-ONLY executable specification of the ragged SiFiGAN entry point (include/serenade_hip.h: srn_pd_gather_ragged),
on top of tests/_vocoder_ragged_emul.py.

``installed()`` is ``_vocoder_ragged_emul.installed()`` plus this one op, stated as the emulator's ``srn_pd_gather``
applied to one item at a time on the item's own L_b rows -- nothing is read or written behind them.  Like the emulators
it wraps, this is never importable from the product and is not a fallback.
"""
from serenade_amd import ops
from tests import _emulator, _vocoder_ragged_emul
from tests._vocoder_ragged_emul import _item


def emul_pd_gather_ragged(a):
    """srn_pd_gather_ragged: item b = the dense gather with B = 1, T = min(lens[b], T) on that item's rows"""
    x, d, lens, out, B, T, C, dil, slope = a
    lens = lens.view(-1)
    for b in range(B):
        L = min(int(lens[b]), T)
        assert L >= 1, "lens: each >= 1"
        _emulator.emul_call("srn_pd_gather", (_item(x, b * T * C), _item(d, b * T), _item(out, b * T * 3 * C), 1, L, C,
                                              dil, slope))


class installed(_vocoder_ragged_emul.installed):
    """_vocoder_ragged_emul.installed() that also knows srn_pd_gather_ragged"""

    def __enter__(self):
        super().__enter__()
        base_call = ops.CallOp.__call__  # the vocoder layer's

        def call(self_, stream=None):
            if self_.name == "srn_pd_gather_ragged":
                emul_pd_gather_ragged(self_.targs)
            else:
                base_call(self_, stream)
        ops.CallOp.__call__ = call
        return self
