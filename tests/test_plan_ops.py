"""CPU check that every plan issues the same launches: each plan below is built without a GPU, its flat op list is
serialised in order -- entry point, every argument, every operand as (buffer ordinal, element offset, buffer size) -- and
the digest is compared with the committed table tests/plan_ops.json.  A change of a stride, an offset, a default or of
which buffer an op reads or writes changes the digest; allocation order and addresses do not.

The front-ends that build part of their launches per call (pYIN, Harvest, the WORLD analysis) are digested through their
public entry points instead: run on CPU tensors with the device guards lifted and every op's `__call__` replaced by a
recorder, the same mechanism as `_emulator.installed`.

How one op serialises: its class, the C-ABI entry point and every argument of `op.kw` (the struct-parameter ops; keys
sorted) or `op.targs` (CallOp).  A tensor or a (tensor, element offset) pair becomes [ordinal of the first appearance of its storage
in this op list, element offset including the storage offset, the storage's element count, dtype]; scalars go by value,
ranges and tuples as lists.  The struct-parameter ops also write the non-pointer fields of the filled params struct, so
resolved defaults (the precision, the tap table) are covered.

    python -m tests.test_plan_ops          # prints the table for tests/plan_ops.json
    python -m tests.test_plan_ops NAME     # prints the serialised op list of one plan (diff two checkouts with it)
"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import serenade_amd
from serenade_amd import (_shapes, contentvec, features, harvest, models, ops, pitch, plan, sifigan, transcriber, vocoder,
                          world)
from serenade_amd.utils.synth import HIFIGAN_PARAMS, SERENADE_PARAMS, fill_state_dict
from tests import _emulator
from tests._weights import serenade_weights
from tests.test_sifigan import SMALL as SIFIGAN_SMALL

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_ops.json")
CPU = torch.device("cpu")
# test_contentvec_host.SMALL (that module skips itself without transformers, so it is not imported here)
CVEC_SMALL = dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64, conv_dim=[16] * 7,
                  num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


# ---------------------------------------------------------------------------------------------- serialisation
def _is_operand(v):
    return isinstance(v, torch.Tensor) or (isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], torch.Tensor))


def _value(v, storages):
    if _is_operand(v):
        t, off = v if isinstance(v, tuple) else (v, 0)
        st = t.untyped_storage()
        ordinal = storages.setdefault(st._cdata, len(storages))
        return ["tensor", ordinal, t.storage_offset() + int(off), st.nbytes() // t.element_size(), str(t.dtype)]
    if isinstance(v, (list, tuple, range)):
        return [_value(x, storages) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"cannot serialise {type(v).__name__}")


def _struct(p):
    """the non-pointer fields of a filled params struct"""
    out = {}
    for name, ctype in p._fields_:
        if ctype is ctypes.c_void_p or getattr(ctype, "_type_", None) is ctypes.c_void_p:  # pointers, arrays of them
            continue
        v = getattr(p, name)
        out[name] = list(v) if isinstance(v, ctypes.Array) else v
    return out


def serialise(op_list):
    storages = {}  # storage identity -> ordinal of its first appearance (the ops pin their tensors, so ids are unique)
    out = []
    for op in op_list:
        if isinstance(op, ops.CallOp):
            out.append(["CallOp", op.name, [_value(a, storages) for a in op.targs]])
        else:
            args = {k: _value(op.kw[k], storages) for k in sorted(op.kw)}
            out.append([type(op).__name__, op.name, args, _struct(op.p)])
    return out


def digest(op_list):
    ser = serialise(op_list)
    text = json.dumps(ser, sort_keys=True, separators=(",", ":"))
    return {"n_ops": len(ser), "sha256": hashlib.sha256(text.encode()).hexdigest()}


# ---------------------------------------------------------------------------------------------- the plans
def _seeded(shapes, seed=0):
    """a state dict of the given shapes (values do not enter the digest; variances are kept positive for the folds)"""
    g = torch.Generator().manual_seed(seed)
    return {k: (0.5 + torch.rand(s, generator=g) if k.endswith("running_var") else 0.1 * torch.randn(s, generator=g))
            for k, s in shapes.items()}


@contextlib.contextmanager
def _precision(prec):
    serenade_amd.set_precision(prec)
    try:
        yield
    finally:
        serenade_amd.set_precision("fp32")


def _serenade():
    model = models.Serenade(**SERENADE_PARAMS)
    model.load_state_dict(serenade_weights())
    return model.eval()


def _decoder_ops(pl):
    return pl.load_ops + pl.pre + [op for ol in pl.steps for op in ol] + [pl.store_op]


def _inference(B, T, prec):
    with _precision(prec), _emulator.installed():
        ip = _serenade()._inference_plan(B, T, 256, 10)
        ip.pl.set_schedule(*ip._sched)  # the Euler steps' op lists are built with the schedule
        return ip.ops + _decoder_ops(ip.pl)


def _ragged():
    with _emulator.installed():
        rp = models.RaggedInferencePlan(_serenade(), [(24, 16), (17, 21), (31, 9)], 10)
        rp.pl.set_schedule(*rp._sched)
        return rp.ops + _decoder_ops(rp.pl)


def _per_sample_t():
    with _emulator.installed():
        pl = _serenade().cfm_decoder.estimator.plan(2, 65, 1, euler=False, per_sample_t=True)
        pl.set_schedule([0.25, 0.75], None)
        return _decoder_ops(pl)


def _hifigan():
    gen = vocoder.HiFiGANGenerator(**HIFIGAN_PARAMS)
    gen.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**HIFIGAN_PARAMS, weight_norm=True))))
    return gen.eval().plan(2, 64).ops


def _sifigan():
    gen = sifigan.SiFiGANGenerator(**SIFIGAN_SMALL)
    gen.load_state_dict(fill_state_dict(_shapes.as_meta(sifigan.sifigan_shapes(**SIFIGAN_SMALL))))
    return gen.eval().plan(2, 11).ops


def _contentvec_base():
    cv = contentvec.ContentVec(device="cpu")
    cv.load_state_dict(_seeded(cv.state_shapes()))
    return contentvec._Plan(cv, CPU, 3, 48000, [16000, 23700, 48000]).ops


def _contentvec_head_chunks():
    """the score budget holds one (item, head) pair, so attention_chunks splits by heads inside an item"""
    cv = contentvec.ContentVec(device="cpu", **CVEC_SMALL)
    cv.load_state_dict(_seeded(cv.state_shapes()))
    T = cv.frames(4000)
    saved = plan.S_BUDGET
    plan.S_BUDGET = T * plan.rup(T, 32) * 4
    try:
        ol = contentvec._Plan(cv, CPU, 2, 4000, [4000, 3100]).ops
    finally:
        plan.S_BUDGET = saved
    assert sum(op.name == "srn_softmax_rows" for op in ol if isinstance(op, ops.CallOp)) == 2 * 2  # items x heads
    return ol


def _transcriber():
    m = transcriber.TranscriptionModel(device="cpu")
    m.load_state_dict(_seeded(m.state_shapes()))
    return transcriber._Plan(m, CPU, 2, 32000, [32000, 23111]).ops


# ---------------------------------------------------------------------------------------------- the front-ends
@contextlib.contextmanager
def _recorded():
    """the ops the front-ends run, in order, instead of their launches (CPU tensors pass the lifted guards)"""
    classes, mods = (ops.CallOp, ops.WorldOp, ops.ExcitationOp), (world, pitch, harvest)
    guards = [m._require_cuda for m in mods]
    run_call, ran = ops.CallOp.__call__, []
    for c in classes:
        c.__call__ = lambda self_, stream=None: ran.append(self_)
    for m in mods:
        m._require_cuda = lambda *a, **k: None
        getattr(m, "_PLANS", {}).clear()  # plans are keyed without the budgets lowered below
    try:
        yield ran
    finally:
        ops.CallOp.__call__ = run_call
        del ops.WorldOp.__call__, ops.ExcitationOp.__call__  # inherited from the base again
        for m, guard in zip(mods, guards):
            m._require_cuda = guard
            getattr(m, "_PLANS", {}).clear()


def _names(ol):
    return [op.name for op in ol]


def _pyin():
    with _recorded() as ol:
        pitch.pyin(torch.zeros(2, 8000), [8000, 5111], sr=16000, fmin=65, fmax=2093, frame_length=1024, hop_length=320)
    assert _names(ol) == ["srn_pyin_observe", "srn_pyin_viterbi"]
    return ol


def _harvest(budget, value, n_ops, *args, **kw):
    """harvest.harvest with one of the module's budgets lowered (as _contentvec_head_chunks lowers S_BUDGET)"""
    saved = getattr(harvest, budget)
    setattr(harvest, budget, saved if value is None else value)
    try:
        with _recorded() as ol:
            harvest.harvest(*args, **kw)
    finally:
        setattr(harvest, budget, saved)
    assert len(ol) == n_ops
    return ol


def _harvest_24k():
    """the event scratch holds 60 of the 152 channels: three srn_harvest_channels launches"""
    ev_cap = -(-6000 // 3) // 2
    ol = _harvest("EVENT_BUDGET", 60 * 2 * 4 * ev_cap * 8, 1 + 3 + 3, torch.zeros(2, 6000), 24000, 71.0, 800.0, 5.0,
                  lengths=[6000, 4111])
    assert [op.targs[13:15] for op in ol[1:4]] == [(0, 60), (60, 60), (120, 32)]  # ch0, channels of the launch
    return ol


def _harvest_8k():
    ol = _harvest("EVENT_BUDGET", None, 5, torch.zeros(2, 3000, dtype=torch.float64), 8000, lengths=[3000, 2111])
    assert ol[0].targs[1] == 1 and ol[0].targs[5] is None  # float64 input, no decimation workspace
    return ol


def _harvest_two_floors():
    """the workspace budget holds one item: the two items of the first group run as two plans"""
    one = harvest._sizes(harvest.harvest_geometry(24000, 71.0, 800.0), [4000, 3111], 24000)[4]
    ol = _harvest("WORKSPACE_BUDGET", one, 3 * 5, torch.zeros(3, 4000), 24000, f0_floor=[71, 71, 90],
                  lengths=[4000, 3111, 3500])
    assert [op.targs[9] for op in ol[::5]] == [1, 1, 1] and [op.targs[-2] for op in ol[1::5]] == [71.0, 71.0, 90.0]
    return ol


def _world_analyzer():
    with _recorded() as ol:
        world.Analyzer()(torch.zeros(2, 4800), [4800, 3333], [np.full(30, 220.0), np.full(21, 180.0)],
                         noise=torch.zeros(2, 1, 41 * 120))
    assert _names(ol) == ["srn_wave_to_f64", "srn_f0_match_length", "srn_world_cheaptrick", "srn_world_project",
                          "srn_world_d4c", "srn_world_pack_features", "srn_cont_f0", "srn_sifigan_excitation"]
    return ol


def _world_wrappers():
    x, f0 = torch.zeros(2400, dtype=torch.float64), torch.full((21,), 200.0, dtype=torch.float64)
    t = np.arange(21) * 0.005
    with _recorded() as ol:
        world.cheaptrick(x, f0, t, 24000)
        world.d4c_band_aperiodicity(x, f0, t, 24000)
        world.sp2mc(torch.ones(21, 513, dtype=torch.float64), 39, 0.466)
        world.convert_continuos_f0(f0)
    assert _names(ol) == ["srn_world_cheaptrick", "srn_world_d4c", "srn_world_project", "srn_cont_f0"]
    return ol


PLANS = {
    "serenade B8xT1024 fp32": lambda: _inference(8, 1024, "fp32"),
    "serenade B8xT1024 bf16x3": lambda: _inference(8, 1024, "bf16x3"),
    "serenade B1xT256 fp32": lambda: _inference(1, 256, "fp32"),
    "serenade B1xT256 bf16x3": lambda: _inference(1, 256, "bf16x3"),
    "serenade ragged": _ragged,
    "estimator per_sample_t B2xL65": _per_sample_t,
    "hifigan B2xT64": _hifigan,
    "sifigan small B2xT11": _sifigan,
    "contentvec base 16000/23700/48000": _contentvec_base,
    "contentvec small, chunks of heads": _contentvec_head_chunks,
    "transcriber 32000/23111": _transcriber,
    "stft log-mel 1024/256": lambda: features._Stft(CPU, 2, 24000, 1024, 256, 1024).ops,
    "stft loudness 2048/240 constant": lambda: features._Stft(CPU, 2, 24000, 2048, 240, 2048, "constant").ops,
    "pyin 8000/5111": _pyin,
    "harvest 24k 6000/4111": _harvest_24k,
    "harvest 8k, no decimation": _harvest_8k,
    "harvest two floors, item chunks": _harvest_two_floors,
    "world analyzer 4800/3333 + excitation": _world_analyzer,
    "world wrappers": _world_wrappers,
}


@pytest.fixture(scope="module")
def lib():
    from serenade_amd import build
    build.build(verbose=False)  # no-op when up to date; hipcc cross-compiles without a GPU


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_ops_match_the_table(lib, name):
    want = json.load(open(TABLE))[name]
    assert digest(PLANS[name]()) == want, f"python -m tests.test_plan_ops {name!r} prints the list to diff"


def test_wave_batch_checks():
    """the input checks ContentVec.forward and TranscriptionModel.forward share, up to the upload (the lengths are
    checked after it)"""
    for wave, kw in ((torch.zeros(2, 3, 8), {}), (torch.zeros(2, 2, 8), dict(allow_channel_dim=True)),
                     (np.zeros((1, 2, 1, 8)), dict(allow_channel_dim=True))):
        with pytest.raises(ValueError, match="^Model: "):
            plan.wave_batch(wave, None, "cpu", "Model", **kw)
    for wave, kw in ((np.zeros(8), {}), (torch.zeros(2, 1, 8), dict(allow_channel_dim=True))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # rank and lengths pass; no device to upload to
            plan.wave_batch(wave, None, "cpu", "Model", **kw)


def test_item_lengths():
    assert plan.item_lengths(None, 3, 7, "Model") == (7, 7, 7)
    for lengths in (torch.tensor([7, 1, 4]), [7, 1, 4], np.array([7, 1, 4]), (7.0, 1, 4)):
        got = plan.item_lengths(lengths, 3, 7, "Model")
        assert got == (7, 1, 4) and all(type(v) is int for v in got)
    for bad in ([7, 1], [7, 1, 4, 4], [7, 0, 4], [7, 8, 4], torch.tensor([8, 1, 4]), np.array([0, 1, 4])):
        with pytest.raises(ValueError, match="^Model: "):
            plan.item_lengths(bad, 3, 7, "Model")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        for row in serialise(PLANS[sys.argv[1]]()):
            print(json.dumps(row, sort_keys=True))
    else:
        print(json.dumps({name: digest(make()) for name, make in PLANS.items()}, indent=1))
