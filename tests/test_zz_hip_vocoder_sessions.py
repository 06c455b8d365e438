"""GPU tests of the ragged causal stream: srn_history_carry_ragged bit for bit against its indexing rule, then the
generator as B independent sessions, eagerly and under hipGraph replay.

* the kernel is a copy, so every check is torch.equal on the bits against tests/_vocoder_sessions_emul.history_carry
  (the rule applied to a snapshot).  The arena lies between guard bands of a NaN sentinel, the gaps between items hold
  the sentinel too, entries are packed back to back (offsets of any alignment).  Per C in {1, 3, 4, 32, 130} and H in
  {1, 6, 60}: one table over T in {1, H - 1, H, H + 1, 2 H + 3} x scale in {1, 8}, at two batch strides (tight, and
  3 floats wider: no multiple of 4), with n = (-1, 0, 1, H - 1, H, H + 1, 2 H + 3, a count past every T) in ONE launch --
  at scale 1 that is m in {1, H - 1, H, H + 1, T} and the clamp; 0 < m < H are the cases an in-place copy gets wrong.
  One table of 96 entries x 2 items has more (buffer, item) pairs than srn_multi_copy takes per launch (160).
* the model: the schedule of tests/_vocoder_sessions_emul.py (an idle item, 1 frame beside 4, a slot restarting behind
  an utterance at 100 times the amplitude, NaN behind every length) on the small causal generator, each utterance
  against its one-shot inference and against its own B = 1 lock-step stream at the waveform gate of 1e-4 (bit equality
  is not required: srn_conv_gemm may tile (3, chunk) differently from (1, chunk); the maxima are printed); the same
  with graphs on -- push 1 eager, push 2 captured, pushes 3 and 4 replayed with other lengths -- torch.equal to the
  eager stream; the full HIFIGAN_PARAMS at B = 2, chunk_frames = 2.

The file's name sorts it behind the suite that was there before it.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from serenade_amd import _lib, ops, vocoder
from serenade_amd.utils.synth import HIFIGAN_PARAMS, fill_state_dict
from tests import _vocoder_sessions_emul as S
from tests._weights import hifigan_weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-4            # the project's waveform gate (README)
SENTINEL = 0x7FC12345  # a quiet NaN with a payload: "never written"
GUARD = 256            # floats of guard band on either side of the arena


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- the kernel
def arena_of(shapes, B, pad, seed):
    """entries (H, T, C, scale) packed back to back behind a guard band, items pad floats apart beyond their rows ->
    (host arena: data random, guards and gaps the sentinel; the table's entries, offsets counted from the guard)"""
    entries, off = [], 0
    for H, T, C, scale in shapes:
        bs = (H + T) * C + pad
        entries.append((off, bs, H, T, C, scale))
        off += B * bs
    buf = torch.full((2 * GUARD + off,), SENTINEL, dtype=torch.int32).view(torch.float32)
    rng = np.random.default_rng(seed)
    for o, bs, H, T, C, _ in entries:
        for b in range(B):
            at = GUARD + o + b * bs
            buf[at:at + (H + T) * C] = torch.from_numpy(rng.standard_normal((H + T) * C).astype(np.float32))
    return buf, entries


def run_and_compare(dev, shapes, n, pad, seed):
    B = len(n)
    host, entries = arena_of(shapes, B, pad, seed)
    want = host.clone()
    S.history_carry(want, GUARD, entries, n)  # from the host tensors, before anything runs
    got = host.to(dev)
    carry = ops.history_carry_ragged_ops((got, GUARD), entries, torch.tensor(n, dtype=torch.int32, device=dev), B)
    for op in carry:
        op()
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(bits(got[:GUARD]), bits(host[:GUARD])) and torch.equal(bits(got[-GUARD:]), bits(host[-GUARD:])), \
        "a guard band was written"
    if not torch.equal(bits(got), bits(want)):
        for o, bs, H, T, C, scale in entries:
            for b in range(B):
                at = GUARD + o + b * bs
                assert torch.equal(bits(got[at:at + bs]), bits(want[at:at + bs])), \
                    f"H {H} T {T} C {C} scale {scale} bs {bs} n {n[b]}: differs from the rule"
        raise AssertionError("a float outside every item was written")
    return len(carry), bool((bits(got) != bits(host)).any())


def table_shapes(C, H):
    return [(H, T, C, scale) for T in sorted({1, H - 1, H, H + 1, 2 * H + 3}) for scale in (1, 8)]  # T = 0 at H = 1


@pytest.mark.parametrize("C", [1, 3, 4, 32, 130])
def test_history_carry_ragged_against_the_rule(dev, C):
    for H in (1, 6, 60):
        n = [-1, 0, 1, H - 1, H, H + 1, 2 * H + 3, 1 << 30]  # H = 1 makes H - 1 a second idle item
        for pad in (0, 3):
            launches, wrote = run_and_compare(dev, table_shapes(C, H), n, pad, seed=100 * C + H + pad)
            assert launches == 1 and wrote
    # every item idle: nothing at all is written
    assert run_and_compare(dev, table_shapes(C, 6), [0] * 4, 3, seed=C) == (1, False)


def test_history_carry_ragged_one_launch_for_more_than_160_pairs(dev):
    rng = np.random.default_rng(0)
    shapes = [(int(rng.integers(0, 61)), int(rng.integers(1, 40)), int(rng.choice([1, 3, 4, 32, 130])),
               int(rng.choice([1, 2, 8]))) for _ in range(_lib.SRN_CARRY_MAX)]
    assert len(shapes) * 2 > _lib.SRN_COPY_LIST_MAX
    assert run_and_compare(dev, shapes, [3, 1], 1, seed=1) == (1, True)
    assert run_and_compare(dev, shapes + shapes[:5], [-1, 2], 0, seed=2) == (2, True)  # a longer table: the next launch


def test_history_carry_ragged_refuses_before_any_launch(dev):
    host, entries = arena_of([(6, 9, 4, 1), (2, 16, 3, 8)], 2, 3, seed=3)
    buf = host.to(dev)
    n = torch.tensor([2, -1], dtype=torch.int32, device=dev)
    op = ops.history_carry_ragged_ops((buf, GUARD), entries, n, 2)[0]
    fn, table = _lib.lib().srn_history_carry_ragged, op.targs[1]
    a, nn = buf.data_ptr() + 4 * GUARD, n.data_ptr()
    assert fn(None, ctypes.byref(table), nn, 2, stream()) == -1 and b"history_carry_ragged" in _lib.lib().srn_last_error()
    assert fn(a, None, nn, 2, stream()) == -1
    assert fn(a, ctypes.byref(table), None, 2, stream()) == -1
    assert fn(a, ctypes.byref(table), nn, 0, stream()) == -1
    for field, v in (("H", -1), ("C", 0), ("scale", 0), ("bs", 20)):
        old = getattr(table.e[1], field)
        setattr(table.e[1], field, v)
        assert fn(a, ctypes.byref(table), nn, 2, stream()) == -1, field
        setattr(table.e[1], field, old)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf.cpu()), bits(host)), "a refused call wrote"
    with pytest.raises(TypeError):
        ops.history_carry_ragged_ops((buf, GUARD), entries, n.float(), 2)
    op()  # and the table as it was runs
    torch.cuda.synchronize()
    want = host.clone()
    S.history_carry(want, GUARD, entries, [2, -1])
    assert torch.equal(bits(buf.cpu()), bits(want))


# ---------------------------------------------------------------------------------------------------- the model
def _gen(dev, full):
    params = dict(HIFIGAN_PARAMS if full else hifigan_weights(small=True)[1], use_causal_conv=True)
    g = vocoder.HiFiGANGenerator(**params)
    g.load_state_dict(fill_state_dict(vocoder.hifigan_state_shapes(**params, weight_norm=True), seed=0 if full else 1))
    g.remove_weight_norm()
    return g.eval().to(dev)


def err(a, b):
    return float((a.cpu() - b.cpu()).abs().max())


@pytest.fixture(scope="module")
def small(dev):
    """(generator, utterances, their one-shot outputs, the eager ragged stream's (per utterance, per push) outputs):
    computed once, shared and left unchanged"""
    g = _gen(dev, False)
    utt = S.utterances(g.in_channels)
    want = {name: g.inference(c.to(dev))[:, 0].cpu() for name, c in utt.items()}
    eager = S.run_schedule(g.stream(S.SESSIONS, S.CHUNK, ragged=True), utt, g.hop, to=lambda t: t.to(dev))
    return g, utt, want, eager


def test_sessions_against_one_shot_and_lock_step(small, dev):
    g, utt, want, (got, _) = small
    for name, c in utt.items():
        s = g.stream(1, S.CHUNK)  # the utterance alone through the lock-step stream (a short last chunk ends it)
        lock = torch.cat([s.push(c[None, t:t + S.CHUNK].to(dev)) for t in range(0, c.shape[0], S.CHUNK)], dim=1)[0].cpu()
        s.reset()
        e1, e2 = err(got[name], want[name]), err(got[name], lock)
        print(f"SESSIONS small, utterance {name}: vs one-shot {e1:.3e}, vs its B = 1 lock-step stream {e2:.3e} "
              f"(bit-equal: {torch.equal(got[name], lock)}), gate {GATE:.0e}")
        assert got[name].shape == want[name].shape and torch.isfinite(got[name]).all()
        assert float(want[name].abs().max()) > 1e-2, "a reference of zeros shows nothing"
        assert e1 < GATE and e2 < GATE, name


def test_sessions_under_graph_replay(small, dev):
    """push 1 runs eagerly, push 2 is captured, pushes 3 and 4 replay the capture with other lengths and restart
    flags than it was captured with: the eager stream's bits"""
    g, utt, _, (_, eager_raw) = small
    was = ops.GRAPHS
    ops.set_graphs(True)
    try:
        s = g.stream(S.SESSIONS, S.CHUNK, ragged=True)
        _, raw = S.run_schedule(s, utt, g.hop, to=lambda t: t.to(dev))
        assert s._pl._runner._graph is not None, "the stream did not replay a captured graph"
    finally:
        ops.set_graphs(was)
    for i, (a, b) in enumerate(zip(raw, eager_raw)):
        assert torch.equal(bits(a), bits(b)), f"push {i + 1}"


def test_sessions_full_generator(dev):
    g = _gen(dev, True)
    c = torch.from_numpy(dict(np.load(os.path.join(GOLDEN, "hifigan_causal.npz")))["c"]).transpose(1, 2).contiguous()
    assert c.shape[0] >= 2 and c.shape[1] >= 5
    first, second, other = c[0, :2], c[0, 2:3], c[1, :5]  # item 0: two utterances; item 1: one of five frames
    want = [g.inference(u.to(dev))[:, 0].cpu() for u in (first, second, other)]
    nan = float("nan")
    s = g.stream(2, 2, ragged=True)
    p1 = torch.stack([first, torch.cat([other[:1], torch.full((1, 80), nan)])])
    p2 = torch.stack([torch.full((2, 80), nan), other[1:3]])
    p3 = torch.stack([torch.cat([second, torch.full((1, 80), nan)]), other[3:5]])
    ys = [s.push(p.to(dev), lens, rs).cpu() for p, lens, rs in
          ((p1, (2, 1), None), (p2, (0, 2), None), (p3, (1, 2), (True, False)))]
    hop = g.hop
    got = [ys[0][0], ys[2][0, :hop], torch.cat([ys[0][1, :hop], ys[1][1], ys[2][1]])]
    for name, a, b in zip(("item 0, first", "item 0, restarted", "item 1"), got, want):
        print(f"SESSIONS full, {name}: vs one-shot {err(a, b):.3e} (gate {GATE:.0e})")
        assert a.shape == b.shape and err(a, b) < GATE and float(b.abs().max()) > 1e-2, name
    assert bool((bits(ys[0][1, hop:]) == 0).all() and (bits(ys[1][0]) == 0).all() and (bits(ys[2][0, hop:]) == 0).all())
    carries = [op for op in s._pl.ops if getattr(op, "name", "") == "srn_history_carry_ragged"]
    print(f"SESSIONS full: {carries[0].targs[1].n} buffers carried by {len(carries) // 2} launch per direction, "
          f"{len(s._pl.ops)} launches per push")
    assert len(carries) == 2 and carries[0].targs[1].n == sum(1 for hb in s._pl.arena._bufs.values() if hb.H)
