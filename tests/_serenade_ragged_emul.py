"""TEST-ONLY executable specification of the two entry points of the ragged style encoder (include/serenade_hip.h:
srn_zero_rows_ragged, srn_gru_recur_last_ragged), on top of tests/_emulator.py.

``installed()`` is ``_emulator.installed()`` plus these two.  Each is stated as the dense rule applied to one item's own
rows: the recurrence is the emulator's ``srn_gru_recur_last`` with B = 1, T = min(n_steps[b], T_cap) on the item's first
rows of gi -- rows at or past the step count are not read, whatever they hold; the mask is "zero" written to the rows
from n_rows[b] to the cap, the rows before them left as they are.  Like the emulator it wraps, this is never importable
from the product and is not a fallback.
"""
from serenade_amd import ops
from tests import _emulator
from tests._vocoder_ragged_emul import _item


def emul_gru_recur_last_ragged(a):
    """srn_gru_recur_last_ragged: item b = the dense recurrence with B = 1, T = min(n_steps[b], T_cap) on its own rows"""
    gi, w_hh_t, b_hh, h, n_steps, B, T_cap, H = a
    n_steps = n_steps.view(-1)
    for b in range(B):
        n = min(int(n_steps[b]), T_cap)
        assert n >= 1, "n_steps: each >= 1"
        _emulator.emul_call("srn_gru_recur_last", (_item(gi, b * T_cap * 3 * H), w_hh_t, b_hh, _item(h, b * H), 1, n, H))


def emul_zero_rows_ragged(a):
    """srn_zero_rows_ragged: rows [n_rows[b], rows_cap) of item b become +0.0, nothing else is written"""
    x, bs, n_cols, n_rows, B, rows_cap = a
    assert B == 1 or bs >= rows_cap * n_cols, "items overlap"
    n_rows = n_rows.view(-1)
    t, off = x if isinstance(x, tuple) else (x, 0)
    flat = t.view(-1)
    for b in range(B):
        n = int(n_rows[b])
        assert n >= 0, "n_rows: each >= 0"
        if n < rows_cap:
            flat[off + b * bs + n * n_cols: off + b * bs + rows_cap * n_cols] = 0.0


class installed(_emulator.installed):
    """_emulator.installed() that also knows the two ragged style-encoder ops"""

    def __enter__(self):
        super().__enter__()
        base_call = ops.CallOp.__call__  # the emulator's

        def call(self_, stream=None):
            if self_.name == "srn_gru_recur_last_ragged":
                emul_gru_recur_last_ragged(self_.targs)
            elif self_.name == "srn_zero_rows_ragged":
                emul_zero_rows_ragged(self_.targs)
            else:
                base_call(self_, stream)
        ops.CallOp.__call__ = call
        return self  # (_emulator.installed.__exit__ restores the __call__ as it was before both layers)
