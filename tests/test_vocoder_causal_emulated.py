"""The causal HiFi-GAN generator (use_causal_conv) on the CPU, through tests/_vocoder_causal_emul.py: the reference's
causal key names, its state dict, the one-shot result against the reference's own output
(tests/golden/hifigan_causal_small.npz, written by tests/golden/make_golden_causal.py), the stream against the one-shot
result, and what the host refuses.  Small configuration: one fused stage (C = 32), one unfused (C = 16)."""
import json
import os

import numpy as np
import pytest
import torch

from serenade_amd import _shapes, ops, vocoder
from serenade_amd.utils.synth import fill_state_dict
from tests import _vocoder_causal_emul as E
from tests._weights import hifigan_weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-4  # the project's waveform gate (README)
SEED = 1     # tests/golden/make_golden_causal.py


def _params(**over):
    return dict(hifigan_weights(small=True)[1], use_causal_conv=True, **over)


def _gen(**over):
    params = _params(**over)
    g = vocoder.HiFiGANGenerator(**params)
    g.load_state_dict(fill_state_dict(vocoder.hifigan_state_shapes(**params, weight_norm=True), seed=SEED))
    return g.eval()


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "hifigan_causal_small.npz")))
    return {k: torch.from_numpy(v) for k, v in g.items()}


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "hifigan_causal_keys.json")) as f:
        return json.load(f)


def err(a, b):
    return float((a - b).abs().max())


def test_key_names_are_the_reference_class_s(keys):
    tab = lambda d: {k: list(s) for k, (s, _) in d.items()}
    assert tab(_shapes.hifigan_shapes(**_params(), weight_norm=True)) == keys["hifigan_causal_small_wn"]
    assert tab(_shapes.hifigan_shapes(**_params(), weight_norm=False)) == keys["hifigan_causal_small"]
    assert {k: list(v.shape) for k, v in vocoder.hifigan_state_shapes(**_params()).items()} == keys["hifigan_causal_small_wn"]
    names = list(keys["hifigan_causal_small"])
    for n in ("input_conv.conv.weight", "upsamples.0.1.deconv.weight", "blocks.3.convs1.2.1.conv.bias",
              "blocks.1.convs2.0.1.conv.weight", "output_conv.1.conv.bias"):
        assert n in names
    # the non-causal names are what they were
    plain = _shapes.hifigan_shapes(**dict(_params(), use_causal_conv=False), weight_norm=False)
    assert "input_conv.weight" in plain and "upsamples.0.1.weight" in plain and "output_conv.1.bias" in plain


def test_the_reference_state_dict_loads(keys):
    g = _gen()
    assert {k: list(v.shape) for k, v in g.state_dict().items()} == keys["hifigan_causal_small_wn"]
    g.remove_weight_norm()
    assert {k: list(v.shape) for k, v in g.state_dict().items()} == keys["hifigan_causal_small"]
    with pytest.raises(RuntimeError):  # a non-causal state dict has other names
        g.load_state_dict(fill_state_dict(vocoder.hifigan_state_shapes(**dict(_params(), use_causal_conv=False),
                                                                       weight_norm=False), seed=SEED))


def test_one_shot_against_the_reference(gold):
    g = _gen()
    with E.installed():
        y = g(gold["c"])
        y5 = g(gold["c"][:, :, :5])
        again = g(gold["c"])  # the one-shot plan leaves no state behind
        one = g.inference(gold["c"][1].t())
        bat = g.inference_batch(gold["c"].transpose(1, 2))
    print(f"CAUSAL one-shot vs reference: {err(y, gold['y']):.3e}, first 5 frames {err(y5, gold['y5']):.3e}")
    assert y.shape == (2, 1, 72) and err(y, gold["y"]) < GATE and err(y5, gold["y5"]) < GATE
    assert torch.equal(again, y) and torch.equal(bat, y)
    assert one.shape == (72, 1) and err(one[:, 0], gold["y"][1, 0]) < GATE
    names = [op.name for op in g.plan(2, 9).ops]
    assert names.count("srn_hifigan_resunit_causal") == 5 and names.count("srn_hifigan_resunit") == 0  # the C = 32 stage
    assert names[-1] == "srn_out_conv_tanh_causal" and names.count("srn_replicate_first_row") == 2


@pytest.mark.parametrize("chunks,chunk_frames", [((4, 4, 1), 4), ((1,) * 9, 1), ((9,), 9), ((3, 3, 3), 3)])
def test_stream_equals_one_shot(gold, chunks, chunk_frames):
    g = _gen()
    c = gold["c"].transpose(1, 2).contiguous()  # (B, T, 80)
    with E.installed():
        want = g(gold["c"])[:, 0]
        s = g.stream(2, chunk_frames)
        outs, t = [], 0
        for n in chunks:
            outs.append(s.push(c[:, t:t + n]))
            assert outs[-1].shape == (2, n * g.hop)
            t += n
    got = torch.cat(outs, dim=1)
    print(f"CAUSAL stream {chunks} vs one-shot: {err(got, want):.3e}; vs reference {err(got, gold['y'][:, 0]):.3e}")
    assert err(got, want) < GATE and err(got, gold["y"][:, 0]) < GATE


def test_single_conv_units_stream(gold):
    """use_additional_convs=False: the one-conv unit of the causal stage builder"""
    g = _gen(use_additional_convs=False)
    c = gold["c"].transpose(1, 2).contiguous()
    with E.installed():
        want = g(gold["c"])[:, 0]
        s = g.stream(2, 2)
        got = torch.cat([s.push(c[:, t:t + 2]) for t in range(0, 9, 2)], dim=1)
    assert err(got, want) < GATE


def test_reset_begins_a_new_stream(gold):
    g = _gen()
    c = gold["c"].transpose(1, 2).contiguous()
    with E.installed():
        want = g(gold["c"])[:, 0]
        s = g.stream(2, 4)
        s.push(c[:, 5:9])  # some other utterance, left unfinished
        s.reset()
        got = torch.cat([s.push(c[:, 0:4]), s.push(c[:, 4:8]), s.push(c[:, 8:9])], dim=1)
        with pytest.raises(ValueError, match="ended"):
            s.push(c[:, 0:4])  # behind a short chunk
        s.reset()
        first = s.push(c[:, 0:4])
    assert err(got, want) < GATE and torch.equal(first, got[:, :4 * g.hop])


def test_what_stream_refuses(gold):
    c = gold["c"].transpose(1, 2).contiguous()
    with E.installed():
        plain = vocoder.HiFiGANGenerator(**dict(_params(), use_causal_conv=False)).eval()
        with pytest.raises(ValueError, match="use_causal_conv"):
            plain.stream(2, 4)
        g = _gen()
        with pytest.raises(ValueError):
            g.stream(2, 0)
        s = g.stream(2, 4)
        with pytest.raises(ValueError, match="1 to 4 frames"):
            s.push(c[:, :5])
        with pytest.raises(ValueError, match="2 utterances"):
            s.push(c[:1, :4])
        assert not g._plans and g._packed is None, "a refusal comes before anything is built"


def test_lengths_zero_the_tails(gold):
    g = _gen()
    c = gold["c"].transpose(1, 2).contiguous()
    c_nan = c.clone()
    c_nan[1, 5:] = 1e30  # behind item 1's end: anything
    with E.installed():
        y = g.inference_batch(c_nan, lengths=[9, 5])
        rag = g.inference_ragged([c[0], c[1, :5]])
        with pytest.raises(ValueError):
            g.inference_batch(c, lengths=[9, 10])
    assert y.shape == (2, 1, 72)
    assert err(y[0, 0], gold["y"][0, 0]) < GATE and err(y[1, 0, :40], gold["y5"][1, 0]) < GATE
    assert float(y[1, 0, 40:].abs().max()) == 0.0
    assert rag[0].shape == (72,) and rag[1].shape == (40,) and err(rag[1], gold["y5"][1, 0]) < GATE


def test_vocoder_decode_and_stream(gold):
    one = np.ones(80, dtype=np.float32)
    rng = np.random.default_rng(3)
    stats = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one + 0.1}
    trg = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one * 0.9}
    c = gold["c"].transpose(1, 2).contiguous()
    with E.installed():
        voc = vocoder.Vocoder.from_generator(_gen(), {"sampling_rate": 24000}, stats, torch.device("cpu"), trg_stats=trg)
        want = voc.decode_batch(c)
        y0, sr = voc.decode(c[0])
        s = voc.stream(2, 4)
        got = torch.cat([s.push(c[:, 0:4]), s.push(c[:, 4:8]), s.push(c[:, 8:9])], dim=1)
        rag = voc.decode_ragged([c[0], c[1, :5]])
        ref = voc.model(((c * torch.from_numpy(trg["scale"]) + torch.from_numpy(trg["mean"])
                          - torch.from_numpy(stats["mean"])) / torch.from_numpy(stats["scale"])).transpose(1, 2))[:, 0]
    assert sr == 24000 and err(want, ref) < GATE and err(y0, want[0]) < GATE and err(got, want) < GATE
    assert err(rag[0], want[0]) < GATE and err(rag[1], want[1, :40]) < GATE


def test_a_non_causal_generator_builds_the_recorded_op_list():
    """use_causal_conv=False, spelled out: the plans of tests/golden/vocoder_oplists.json, op for op"""
    from tests.golden import make_golden_oplists as G
    with open(G.FIXTURE) as f:
        want = json.load(f)
    with E.installed():
        g = G._hifigan(use_causal_conv=False)
        assert not g.use_causal_conv
        assert json.loads(json.dumps(G.signature(g.plan(2, 5)))) == want["hifigan_small/dense(2, 5)"]
        assert json.loads(json.dumps(G.signature(g.plan_ragged(2, 8, bucket=1)))) == want["hifigan_small/ragged(2, 8)"]


def test_unit_op_takes_either_lens_or_lead():
    x = torch.zeros(4)
    with pytest.raises(TypeError):
        ops.ResUnitOp(lens=torch.zeros(1, dtype=torch.int32), lead=torch.zeros(1, dtype=torch.int32), n_batch=1, x=x)
    with pytest.raises(TypeError):
        ops.ResUnitOp(lead=torch.zeros(1), n_batch=1, x=x)  # not int32
