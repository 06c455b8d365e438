"""The ragged causal stream (HiFiGANGenerator.stream / Vocoder.stream with ragged=True) and VocoderSessions on the CPU,
through tests/_vocoder_sessions_emul.py: B = 3 independent sessions on the small causal generator over a schedule with
an idle item, 1 frame beside 4, an utterance ending and its slot restarting on the next push (the first at 100 times the
amplitude), and NaN in every row of c past an item's length -- each utterance's concatenated output against the
generator's own one-shot inference at the waveform gate.  Also: the stream without the keyword is what it was, every
refusal comes before anything is built, the ABI's table has the C layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from serenade_amd import _lib, ops, vocoder
from serenade_amd.utils.synth import fill_state_dict
from tests import _vocoder_sessions_emul as S
from tests._weights import hifigan_weights

GATE = 1e-4  # the project's waveform gate (README)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "serenade_hip.h")


def _params(**over):
    return dict(hifigan_weights(small=True)[1], use_causal_conv=True, **over)


def _gen(**over):
    params = _params(**over)
    g = vocoder.HiFiGANGenerator(**params)
    g.load_state_dict(fill_state_dict(vocoder.hifigan_state_shapes(**params, weight_norm=True), seed=1))
    return g.eval()


def err(a, b):
    return float((a - b).abs().max())


@pytest.fixture(scope="module")
def case():
    """(generator, utterances, their one-shot outputs): computed once, shared and left unchanged"""
    g = _gen()
    utt = S.utterances(g.in_channels)
    with S.installed():
        want = {name: g.inference(c)[:, 0] for name, c in utt.items()}
    return g, utt, want


def test_sessions_equal_their_one_shot_calls(case):
    g, utt, want = case
    with S.installed():
        s = g.stream(S.SESSIONS, S.CHUNK, ragged=True)
        assert isinstance(s, vocoder.HiFiGANSessionStream)
        got, _ = S.run_schedule(s, utt, g.hop)
    for name in utt:
        e = err(got[name], want[name])
        print(f"SESSIONS emulated, utterance {name}: vs one-shot {e:.3e} (gate {GATE:.0e})")
        assert got[name].shape == want[name].shape and torch.isfinite(got[name]).all() and e < GATE, name
    assert s._pl is not None and all(pl is not s._pl and k[0] != "stream" for k, pl in g._plans.items()), \
        "the stream owns its plan: the generator's plan cache (which holds the one-shot plans) is not used"


def test_the_plan_is_the_carry_plan_wrapped(case):
    g = case[0]
    with S.installed():
        dense = vocoder.CausalHiFiGANPlan(g, 3, 4, carry=True)
        rag = vocoder.CausalHiFiGANPlan(g, 3, 4, carry="ragged")
    names = lambda pl: [getattr(op, "name", type(op).__name__) for op in pl.ops]
    n_compute = len(names(dense)) - names(dense).count("MultiCopyOp")
    assert names(rag)[0] == "srn_history_carry_ragged" and names(rag)[-1] == "srn_history_carry_ragged"
    assert names(rag)[1:-2] == names(dense)[:n_compute] and names(rag)[-2] == "srn_zero_rows_ragged"
    assert names(rag).count("srn_history_carry_ragged") == 2, "one launch in front, one behind"
    table = S.table_entries(rag.ops[0].targs[1])
    assert len(table) == sum(1 for hb in rag.arena._bufs.values() if hb.H)
    assert {e[5] for e in table} == {1, 4, 8}  # rows per input frame: the mel rate and the two stages'
    with pytest.raises(ValueError):
        vocoder.CausalHiFiGANPlan(g, 3, 4, ragged=True, carry="ragged")


def test_two_streams_do_not_share_state(case):
    g, utt, want = case
    with S.installed():
        s1, s2 = g.stream(1, 4, ragged=True), g.stream(1, 4, ragged=True)
        a, b = utt["U0"], utt["A"]
        outs = []
        for t in range(0, 8, 4):  # interleaved pushes of two utterances through two streams of one shape
            outs.append((s1.push(a[None, t:t + 4], [4]), s2.push(b[None, t:t + 4], [min(4, 5 - t)])))
    assert err(torch.cat([o[0][0] for o in outs]), want["U0"][:8 * g.hop]) < GATE
    assert err(torch.cat([outs[0][1][0], outs[1][1][0, :g.hop]]), want["A"]) < GATE


def test_without_the_keyword_the_stream_is_what_it_was(case):
    g, utt, _ = case
    c = torch.stack([utt["U0"][:8], utt["U2"][:7].repeat(2, 1)[:8]])
    with S.installed():
        s = g.stream(2, 4)
        assert type(s) is vocoder.HiFiGANStream and type(g.stream(2, 4, ragged=False)) is vocoder.HiFiGANStream
        y = torch.cat([s.push(c[:, :4]), s.push(c[:, 4:])], dim=1)
        pl = next(v for k, v in g._plans.items() if k[0] == "stream")
        ref = vocoder.CausalHiFiGANPlan(g, 2, 4, carry=True)
        one = g.inference_batch(c)[:, 0]
    sig = lambda pl: [(getattr(op, "name", type(op).__name__), len(getattr(op, "_lists", ()))) for op in pl.ops]
    assert sig(pl) == sig(ref) and "srn_history_carry_ragged" not in [n for n, _ in sig(pl)]
    assert not hasattr(pl, "push") and err(y, one) < GATE
    g._plans.clear()


def test_what_the_ragged_stream_refuses(case):
    utt = case[1]
    c = torch.stack([utt["U0"][:4]] * 3)
    with S.installed():
        plain = vocoder.HiFiGANGenerator(**dict(_params(), use_causal_conv=False)).eval()
        with pytest.raises(ValueError, match="use_causal_conv"):
            plain.stream(3, 4, ragged=True)
        g = _gen()
        with pytest.raises(ValueError):
            g.stream(3, 0, ragged=True)
        with pytest.raises(ValueError):
            g.stream(0, 4, ragged=True)
        s = g.stream(3, 4, ragged=True)
        bad = [
            (c[0], [4, 4, 4], None, "expected"),                      # rank
            (c[:, :, :79], [4, 4, 4], None, "expected"),              # channels
            (c[:2], [4, 4], None, "3 sessions"),                      # B
            (c[:, :0], [0, 0, 0], None, "1 to 4 frames"),             # n_max = 0
            (torch.cat([c, c], 1)[:, :5], [4, 4, 4], None, "1 to 4 frames"),  # n_max above chunk_frames
            (c[:, :3], [3, 4, 0], None, "lengths"),                   # a length above n_max
            (c, [4, -1, 0], None, "lengths"),                         # a negative length
            (c, [4, 4], None, "lengths holds 2"),                     # lengths of the wrong size
            (c, [4, 4, 4], [True, False], "restart holds 2"),         # restart of the wrong size
        ]
        for cc, lens, rs, msg in bad:
            with pytest.raises(ValueError, match=msg):
                s.push(cc, lens, rs)
        stats = {"mean": np.zeros(80, np.float32), "scale": np.ones(80, np.float32)}
        voc = vocoder.Vocoder.from_generator(g, {"sampling_rate": 24000}, stats, torch.device("cpu"), trg_stats=stats)
        g._packed = None
        vs = voc.stream(3, 4, ragged=True)
        with pytest.raises(ValueError, match="lengths"):
            vs.push(c, [5, 0, 0])
        assert s._pl is None and vs.stream._pl is None and not g._plans and g._packed is None, \
            "a refusal comes before anything is built"
        assert s.push(c, torch.tensor([4, 0, 2]), np.array([True, False, True])).shape == (3, 4 * g.hop)  # and then it runs


def _vocoder(g):
    one = np.ones(80, dtype=np.float32)
    rng = np.random.default_rng(3)
    stats = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one + 0.1}
    trg = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one * 0.9}
    return vocoder.Vocoder.from_generator(g, {"sampling_rate": 24000}, stats, torch.device("cpu"), trg_stats=trg)


def test_vocoder_stream_ragged(case):
    utt = case[1]
    with S.installed():
        voc = _vocoder(_gen())
        want = {name: voc.decode(c)[0] for name, c in utt.items()}
        s = voc.stream(S.SESSIONS, S.CHUNK, ragged=True)
        assert isinstance(s, vocoder.VocoderSessionStream)
        got, _ = S.run_schedule(s, utt, voc.model.hop)
    for name in utt:
        assert err(got[name], want[name]) < GATE, name


def test_vocoder_sessions(case):
    utt = case[1]
    with S.installed():
        voc = _vocoder(_gen())
        want = {name: voc.decode(c)[0] for name, c in utt.items()}
        ses = vocoder.VocoderSessions(voc, slots=2, chunk_frames=4)
        hop = voc.model.hop
        a, b = ses.open(), ses.open()
        assert (a, b) == (0, 1)
        with pytest.raises(RuntimeError, match="in use"):
            ses.open()
        ses.feed(a, utt["U0"][:6])          # 6 frames at once: two steps' worth
        ses.feed(b, utt["A"][:1])
        out = {"U0": [], "A": [], "B": [], "U2": []}
        y = ses.step()                      # a gives 4, b gives 1
        assert set(y) == {a, b} and y[a].shape == (4 * hop,) and y[b].shape == (hop,)
        out["U0"].append(y[a]); out["A"].append(y[b])
        ses.feed(b, utt["A"][1:5])
        ses.close(b)                        # closing: freed by the step that drains it
        with pytest.raises(ValueError, match="closing"):
            ses.feed(b, utt["A"][:1])
        y = ses.step()                      # a gives its other 2, b its last 4
        out["U0"].append(y[a]); out["A"].append(y[b])
        assert ses.queued(a) == 0
        with pytest.raises(ValueError, match="not open"):
            ses.queued(b)
        assert ses.step() == {}             # nothing queued: no push
        b2 = ses.open()                     # the freed slot, reused: utterance B begins where A (x 100) ended
        assert b2 == b
        ses.feed(b2, utt["B"])
        ses.feed(a, utt["U0"][6:])
        y = ses.step()
        out["U0"].append(y[a]); out["B"].append(y[b2])
        y = ses.step()                      # a has nothing queued and stays open; b2 gives its last 2
        assert set(y) == {b2}
        out["B"].append(y[b2])
        ses.close(a); ses.close(b2)
        c = ses.open()                      # a drained slot closes at once
        ses.feed(c, utt["U2"])
        while ses.queued(c):
            out["U2"].append(ses.step()[c])
        with pytest.raises(ValueError, match="expected"):
            ses.feed(c, utt["U2"][:, :40])
        with pytest.raises(ValueError, match="not open"):
            ses.feed(1 - c, utt["U2"])
    for name in out:
        assert err(torch.cat(out[name]), want[name]) < GATE, name


def test_lead_table_per_item():
    from serenade_amd.plan import LeadTable
    t = LeadTable((4, 2), 3, torch.device("cpu"))
    t.set_pushed_items([0, 5, 1 << 29])
    assert t.lead.tolist() == [[0, 5, 1 << 29], [0, 20, LeadTable.CAP], [0, 40, LeadTable.CAP]]
    t.set_pushed(2)  # as it was
    assert t.lead.tolist() == [[2] * 3, [8] * 3, [16] * 3]


def test_carry_rule_is_a_snapshot():
    """the statement the GPU test compares the kernel with: overlapping spans (0 < m < H) come out as a memmove's"""
    H, T, C = 6, 9, 2
    x = torch.arange(3 * (H + T) * C, dtype=torch.float32)
    want = x.clone().view(3, H + T, C)
    want[0, :H] = want[0, 2:2 + H].clone()   # m = 2 < H
    want[1, :H] = 0.0                        # restart
    S.history_carry(x, 0, [(0, (H + T) * C, H, T, C, 1)], [2, -1, 0])
    assert torch.equal(x.view(3, H + T, C), want)


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail differently"""
    lib = _lib.lib()
    t = _lib.SrnCarryTable()
    t.n = 1
    t.e[0].off, t.e[0].bs, t.e[0].H, t.e[0].T, t.e[0].C, t.e[0].scale = 0, 64, 2, 6, 4, 1
    buf = (ctypes.c_float * 256)()
    n = (ctypes.c_int32 * 4)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.srn_history_carry_ragged(None, ctypes.byref(t), p(n), 2, None) == -1
    assert b"history_carry_ragged" in lib.srn_last_error()
    assert lib.srn_history_carry_ragged(p(buf), None, p(n), 2, None) == -1
    assert lib.srn_history_carry_ragged(p(buf), ctypes.byref(t), None, 2, None) == -1
    assert lib.srn_history_carry_ragged(p(buf), ctypes.byref(t), p(n), 0, None) == -1
    for field, v in (("H", -1), ("C", 0), ("scale", 0), ("T", -1), ("off", -4), ("bs", 31)):
        old = getattr(t.e[0], field)
        setattr(t.e[0], field, v)
        assert lib.srn_history_carry_ragged(p(buf), ctypes.byref(t), p(n), 2, None) == -1, field
        setattr(t.e[0], field, old)
    for count in (0, _lib.SRN_CARRY_MAX + 1):
        t.n = count
        assert lib.srn_history_carry_ragged(p(buf), ctypes.byref(t), p(n), 2, None) == -1


@pytest.mark.parametrize("name", ["SrnCarryEntry", "SrnCarryTable"])
def test_carry_table_layout_matches_c(tmp_path, name):
    cls = getattr(_lib, name)
    fields = [f[0] for f in cls._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             f'printf("%zu\\n", sizeof({name}));'] + [f'printf("%zu\\n", offsetof({name}, {f}));' for f in fields]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "probe")]).split()]
    assert out[0] == ctypes.sizeof(cls) and [getattr(cls, f).offset for f in fields] == out[1:]
    assert _lib.SRN_CARRY_MAX == 96 and f"#define SRN_CARRY_MAX {_lib.SRN_CARRY_MAX}" in open(HEADER).read()
