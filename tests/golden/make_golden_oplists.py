"""Writes tests/golden/vocoder_oplists.json: the op list of every HiFi-GAN / SiFiGAN plan below, dense and ragged, as
the plan builders emit it -- which entry point each op calls, with which arguments, on which buffer.

    python tests/golden/make_golden_oplists.py

Needs the built library (the ops look their entry points up) but no GPU: the plans are built on the CPU under
tests/_emulator.installed() and never run.  Plans are reached only through `gen.plan(B, T)` and
`gen.plan_ragged(B, T_max, bucket=1)`.  tests/test_vocoder_oplists_emulated.py rebuilds the same plans and compares.

Signature of a plan = [[entry name, arguments]] over plan.ops.  The arguments are `op.kw` for the struct ops (None
values dropped) and `op.targs` for a CallOp; scalars appear as they are; a tensor, or a (tensor, element offset) pair,
appears as ["buf", i, offset in 4-byte elements from the start of its storage, dtype, numel], where i numbers the
storages by first appearance along the op list.  No address enters it."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from serenade_amd import _shapes, sifigan, vocoder  # noqa: E402
from serenade_amd.utils.synth import HIFIGAN_PARAMS, fill_state_dict  # noqa: E402
from tests import _emulator  # noqa: E402
from tests._weights import hifigan_weights  # noqa: E402
from tests.test_sifigan import SMALL  # noqa: E402

FIXTURE = os.path.join(HERE, "vocoder_oplists.json")


def signature(plan):
    storages = {}

    def buf(t, off):
        i = storages.setdefault(t.untyped_storage().data_ptr(), len(storages))
        return ["buf", i, t.storage_offset() * t.element_size() // 4 + int(off), str(t.dtype), t.numel()]

    def enc(v):
        if isinstance(v, torch.Tensor):
            return buf(v, 0)
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], torch.Tensor):
            return buf(*v)
        if isinstance(v, (list, tuple)):
            return [enc(x) for x in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"{type(v).__name__} in an op's arguments")

    sig = []
    for op in plan.ops:
        if hasattr(op, "kw"):
            args = {k: enc(op.kw[k]) for k in sorted(op.kw) if op.kw[k] is not None}
        else:
            args = [enc(a) for a in op.targs]
        sig.append([op.name, args])
    return sig


def _hifigan(**over):
    params = dict(HIFIGAN_PARAMS if over.pop("full", False) else hifigan_weights(small=True)[1], **over)
    g = vocoder.HiFiGANGenerator(**params)
    g.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**params, weight_norm=True)), seed=0))
    return g.eval()


def _sifigan(cfg):
    g = sifigan.SiFiGANGenerator(**cfg)
    g.load_state_dict(fill_state_dict(_shapes.as_meta(sifigan.sifigan_shapes(**cfg)), seed=0))
    return g.eval()


SHARED = dict(SMALL, share_upsamples=True, share_downsamples=True,
              source_network_params=dict(SMALL["source_network_params"], use_additional_convs=False))
# (name, generator, dense (B, T), ragged (B, T_max) at bucket = 1)
GENERATORS = [("hifigan_small", lambda: _hifigan(), (2, 5), (2, 8)),
              ("hifigan_small_single_conv", lambda: _hifigan(use_additional_convs=False), (2, 5), (2, 8)),
              ("hifigan_full", lambda: _hifigan(full=True), (2, 5), (2, 8)),
              ("sifigan_small", lambda: _sifigan(SMALL), (2, 11), (2, 16)),
              ("sifigan_small_shared", lambda: _sifigan(SHARED), (2, 11), (2, 16))]


def signatures():
    """{plan name: signature}, in the order of GENERATORS, dense before ragged"""
    out = {}
    with _emulator.installed():
        for name, make, dense, ragged in GENERATORS:
            g = make()
            out[f"{name}/dense{dense}"] = signature(g.plan(*dense))
            out[f"{name}/ragged{ragged}"] = signature(g.plan_ragged(*ragged, bucket=1))
    return out


def dumps(sigs):
    """one op per line, so that a diff of the fixture reads op by op"""
    plans = []
    for name, sig in sigs.items():
        lines = ",\n".join("  " + json.dumps(op, sort_keys=True) for op in sig)
        plans.append(f"{json.dumps(name)}: [\n{lines}\n]")
    return "{\n" + ",\n".join(plans) + "\n}\n"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(dumps(signatures()))
    print("wrote", FIXTURE)
