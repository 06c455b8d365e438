"""TEST-ONLY executable specification of srn_history_carry_ragged (include/serenade_hip.h), layered on
tests/_vocoder_causal_emul.py, and the session schedule the CPU and GPU tests of the ragged causal stream share.

``history_carry`` states the entry point by its indexing rule on a snapshot of the arena, so overlapping spans come out
as a memmove's; the GPU tests compare the kernel with it bit for bit.  ``installed()`` is the causal emulator plus that
call.  Like the emulators it wraps, this is never importable from the product and is not a fallback.
"""
import numpy as np
import torch

from serenade_amd import ops
from tests import _emulator
from tests import _vocoder_causal_emul as E


def history_carry(flat, base, entries, n):
    """the rule of srn_history_carry_ragged on `flat` (1-D fp32, the arena at element `base`), in place.  entries:
    (off, bs, H, T, C, scale) per buffer; n: the per-item counts as ints."""
    snap = flat.clone()  # every read sees the arena as it was before the launch
    for off, bs, H, T, C, scale in entries:
        for b, nb in enumerate(n):
            at = base + off + b * bs
            if nb < 0:
                flat[at:at + H * C] = 0.0
            elif nb > 0:
                m = min(nb, T // scale) * scale
                if m:
                    flat[at:at + H * C] = snap[at + m * C:at + (m + H) * C]


def table_entries(table):
    return [(e.off, e.bs, e.H, e.T, e.C, e.scale) for e in table.e[:table.n]]


def emul_history_carry_ragged(a):
    arena, table, n, B = a
    f, o = _emulator._flat(arena)
    history_carry(f, o, table_entries(table), [int(v) for v in n.view(-1)[:B]])


class installed(E.installed):
    """_vocoder_causal_emul.installed() that also knows srn_history_carry_ragged"""

    def __enter__(self):
        super().__enter__()
        base_call = ops.CallOp.__call__  # the causal emulator's

        def call(self_, stream=None):
            if self_.name == "srn_history_carry_ragged":
                emul_history_carry_ragged(self_.targs)
            else:
                base_call(self_, stream)
        ops.CallOp.__call__ = call
        return self  # (_emulator.installed.__exit__ restores the __call__s as they were before every layer)


# ---------------------------------------------------------------------------------------------------- the schedule
# B = 3 sessions, chunk_frames = 4.  Per push: (n_max, lengths, restart).  Session 0 speaks utterance U0 (9 frames),
# session 1 utterance A (5 frames, amplitude x 100: history leaking into its successor would show) and then, restarting
# on the very next push, utterance B (6 frames); session 2 utterance U2 (7 frames), idle for a push in the middle and 1
# frame at a time while session 0 gives 4.
CHUNK, SESSIONS = 4, 3
UTTERANCES = {"U0": (0, 9, 1.0), "A": (1, 5, 100.0), "B": (1, 6, 1.0), "U2": (2, 7, 1.0)}  # name: (session, frames, gain)
SCHEDULE = [
    # n_max, {session: (utterance, frames)}, restart
    (4, {0: ("U0", 4), 1: ("A", 3), 2: ("U2", 1)}, (False, False, False)),  # 1 frame beside 4; every slot begins restarted
    (3, {0: ("U0", 1), 1: ("A", 2)}, (False, False, False)),                # session 2 idle; A ends
    (4, {0: ("U0", 4), 1: ("B", 2), 2: ("U2", 4)}, (False, True, False)),   # B begins where A ended
    (4, {1: ("B", 4), 2: ("U2", 2)}, (False, False, False)),                # session 0 idle (U0 is complete)
]


def utterances(in_channels, seed=5):
    rng = np.random.default_rng(seed)
    return {name: torch.from_numpy((gain * rng.standard_normal((frames, in_channels))).astype(np.float32))
            for name, (_, frames, gain) in UTTERANCES.items()}


def pushes(utt):
    """[(c (3, n_max, C) with NaN in every row past an item's length, lengths, restart, {session: utterance})]"""
    at = {name: 0 for name in utt}
    out = []
    for n_max, items, restart in SCHEDULE:
        C = next(iter(utt.values())).shape[1]
        c = torch.full((SESSIONS, n_max, C), float("nan"))
        lens = [0] * SESSIONS
        for b, (name, n) in items.items():
            c[b, :n] = utt[name][at[name]:at[name] + n]
            at[name] += n
            lens[b] = n
        out.append((c, lens, list(restart), {b: name for b, (name, _) in items.items()}))
    assert all(at[name] == utt[name].shape[0] for name in utt), "the schedule delivers every utterance whole"
    return out


def run_schedule(stream, utt, hop, to=lambda t: t):
    """push the schedule through `stream` -> ({utterance: its concatenated valid output}, the raw outputs per push)"""
    got, raw = {name: [] for name in utt}, []
    for c, lens, restart, names in pushes(utt):
        y = stream.push(to(c), lens, restart).cpu()
        assert y.shape == (SESSIONS, c.shape[1] * hop)
        for b in range(SESSIONS):
            assert bool((y[b, lens[b] * hop:].view(torch.int32) == 0).all()), "the output past an item's length is +0.0"
            if b in names:
                got[names[b]].append(y[b, :lens[b] * hop])
        raw.append(y)
    return {name: torch.cat(v) for name, v in got.items()}, raw
