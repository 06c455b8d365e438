"""Writes tests/golden/train_step_trace.json: every launch of one whole-model training step, in the order the step
issues them -- which entry point, with which arguments, on which buffer.

    python tests/golden/make_golden_train_trace.py

Needs the built library (the ops look their entry points up) but no GPU: the step runs on the CPU under
tests/_emulator.installed().  tests/test_train_trace_emulated.py runs the same step and compares.

The step: TrainSerenade(serenade_weights(), cpu, dropout=0.0) at B = 2, T = 64, lengths (64, 41), inputs and draws from
fixed generator seeds; forward -> model.backward(cfm + prior) -> AdamW.step().  The optimizer is built with
max_grad_norm=0: the clip factor is the one launch argument that is computed from the data, and its last bits would pin
the CPU's summation order into the fixture; without clipping it is 1.0 and the launches are the same (srn_sumsq still
runs, step() returns the norm).

A launch is the __call__ of ConvOp, CallOp, TnGemmOp, ResUnitOp, MultiCopyOp or TransposeMultiOp.  Its signature is
[entry name, arguments]: `op.kw` for the struct ops, `op.targs` for a CallOp, the entry table for the two multi ops.
Scalars appear as they are; a tensor, or a (tensor, element offset) pair, appears as ["buf", i, offset in 4-byte
elements from the start of its storage, dtype, numel], where i numbers the storages by first appearance (the recorder
keeps every tensor alive until the trace is complete, so no address is met twice).  A keyword that is None or equals
the default in the signature of the op's filler is dropped, so a builder that spells a default and one that omits it
compare equal.  No address enters the trace."""
import inspect
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from serenade_amd import ops, training  # noqa: E402
from tests import _emulator  # noqa: E402
from tests._weights import serenade_weights  # noqa: E402

FIXTURE = os.path.join(HERE, "train_step_trace.json")
STRUCT_OPS = (ops.ConvOp, ops.TnGemmOp, ops.ResUnitOp)
B, T, LENGTHS = 2, 64, (64, 41)


def _defaults():
    """{struct op class: {keyword: default}} from the filler's signature (read before the emulator is installed)"""
    out = {}
    for cls in STRUCT_OPS:
        fill = getattr(cls, "_fill", None) or cls.__init__
        out[cls] = {k: p.default for k, p in inspect.signature(fill).parameters.items()
                    if p.default is not inspect.Parameter.empty}
    return out


class Recorder:
    """wraps the __call__ of the six op classes (the emulator's, when it is installed first) and appends the
    signature of every launch to `self.trace`"""

    def __init__(self, defaults):
        self.defaults, self.trace, self._storages, self._alive = defaults, [], {}, []

    def _buf(self, t, off):
        self._alive.append(t)
        i = self._storages.setdefault(t.untyped_storage().data_ptr(), len(self._storages))
        return ["buf", i, t.storage_offset() * t.element_size() // 4 + int(off), str(t.dtype), t.numel()]

    def _enc(self, v):
        if isinstance(v, torch.Tensor):
            return self._buf(v, 0)
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], torch.Tensor):
            return self._buf(*v)
        if isinstance(v, (list, tuple, range)):
            return [self._enc(x) for x in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"{type(v).__name__} in an op's arguments")

    def _args(self, op):
        if isinstance(op, STRUCT_OPS):
            dflt = self.defaults[type(op)]
            same = lambda k, v: k in dflt and not isinstance(v, torch.Tensor) and (
                v == dflt[k] or (isinstance(v, (list, tuple, range)) and list(v) == list(dflt[k] or ())))
            return {k: self._enc(v) for k, v in sorted(op.kw.items()) if v is not None and not same(k, v)}
        if isinstance(op, ops.CallOp):
            return [self._enc(a) for a in op.targs]
        if isinstance(op, ops.MultiCopyOp):
            return {"srcs": self._enc(op.srcs), "offs": list(op.offs), "dst": self._enc(op.dst)}
        return [self._enc(e) for e in op.entries]

    def __enter__(self):
        self._saved = []
        for cls in (*STRUCT_OPS, ops.CallOp, ops.MultiCopyOp, ops.TransposeMultiOp):
            inner = cls.__call__
            self._saved.append((cls, inner))
            cls.__call__ = self._wrap(cls, inner)
        return self

    def _wrap(self, cls, inner):
        names = {ops.MultiCopyOp: "srn_multi_copy", ops.TransposeMultiOp: "srn_transpose_multi"}

        def call(op, stream=None):
            self.trace.append([names.get(cls) or op.name, self._args(op)])
            return inner(op, stream)
        return call

    def __exit__(self, *exc):
        for cls, inner in self._saved:
            cls.__call__ = inner


def case():
    g = torch.Generator().manual_seed(20)
    r = lambda *s: torch.randn(*s, generator=g)
    inputs = dict(x=r(B, T, 768), lengths=torch.tensor(LENGTHS), logmel=r(B, T, 80), midi=r(B, T, 1), lft=r(B, T, 1))
    draws = {"uniform": 0.3, "seg_start": 10, "t": torch.rand(B, 1, 1, generator=g), "z": r(B, 80, T)}
    return inputs, draws


def trace():
    """the launches of forward -> backward -> AdamW.step(), as a list of [entry name, arguments]"""
    defaults = _defaults()
    inputs, draws = case()
    with _emulator.installed(), Recorder(defaults) as rec:
        model = training.TrainSerenade(serenade_weights(), torch.device("cpu"), dropout=0.0)
        opt = training.AdamW(model, max_grad_norm=0)
        ret = model(inputs["x"], inputs["lengths"], inputs["logmel"], inputs["midi"], inputs["lft"], draws=draws)
        model.backward(ret["cfm_loss"] + ret["prior_loss"])
        opt.step()
    return rec.trace


def dumps(tr):
    """one launch per line, so that a diff of the fixture reads launch by launch"""
    return "[\n" + ",\n".join(json.dumps(op, sort_keys=True) for op in tr) + "\n]\n"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(dumps(trace()))
    print("wrote", FIXTURE)
