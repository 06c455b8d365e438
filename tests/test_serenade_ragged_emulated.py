"""Serenade with lengths as data (CPU, through the C-ABI emulator + tests/_serenade_ragged_emul.py): the host logic of
`Serenade.inference_ragged(bucket=)` -- one plan per (B, bucket of the longest prompt + source), lengths rewritten in
place -- of `StyleEncoder.forward(lengths=)`, and of `serenade-decode --ragged-plan`.  The kernels themselves are
tested by tests/test_zz_hip_serenade_ragged.py on the GPU."""
import contextlib
import os
import wave as wavmod
from unittest import mock

import numpy as np
import pytest
import torch

from serenade_amd import models
from serenade_amd.bin import ssc_decode
from serenade_amd.utils.synth import SERENADE_PARAMS, synth_inputs
from tests import _serenade_ragged_emul
from tests import test_cli as cli
from tests._weights import serenade_weights

BUCKET = 16  # small, so that the emulated estimator stays short; the CLI's models.RAGGED_BUCKET is tested below
KEYS = ("x", "midi", "lft", "ref_x", "ref_logmel", "ref_midi", "ref_lft")


def nerr(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def model():
    m = models.Serenade(**SERENADE_PARAMS)
    m.load_state_dict(serenade_weights())
    return m.eval()


def _batch(shapes, seed):
    ds = [synth_inputs(1, t, T_ref=r, seed=seed + i) for i, (t, r) in enumerate(shapes)]
    return ds, [tuple(d[k][0] for k in KEYS) for d in ds]


def _single(model, d):
    return model.inference(d["x"], d["lengths"], d["midi"], d["lft"], d["ref_x"], d["ref_lengths"], d["ref_logmel"],
                           d["ref_midi"], d["ref_lft"], noise=d["z"])


def _bucket_plans(model):
    return {k: v for k, v in model._plans.items() if k[0] == "ragged-bucket"}


def test_bucketed_batch_equals_b1_runs_and_reuses_its_plan(model):
    """every item of a bucketed batch is its own B = 1 inference() (the bound of the shape-keyed plan's test,
    tests/test_plan_emulated.py); a second batch of the same bucket runs on the SAME plan object, after the first one
    left its rows everywhere; a batch across the bucket's edge builds the next plan; the shape-keyed cache is left
    alone"""
    first, second = [(24, 16), (17, 21), (31, 9)], [(9, 25), (30, 18), (5, 4)]  # longest 40 and 48: L_cap 48 both
    across = [(33, 16), (6, 7), (20, 20)]  # longest 49: L_cap 64
    with _serenade_ragged_emul.installed():
        model._plans.clear()
        ds1, items = _batch(first, 70)
        shape_keyed = model.inference_ragged(items, noises=[d["z"][0] for d in ds1])
        keyed = dict(model._plans)
        assert len(keyed) == 1 and next(iter(keyed))[0] == "ragged"
        outs1 = model.inference_ragged(items, noises=[d["z"][0] for d in ds1], bucket=BUCKET)
        plans = _bucket_plans(model)
        assert len(plans) == 1
        (key, plan), = plans.items()
        assert key[:3] == ("ragged-bucket", 3, 48) and plan.Lm == 48
        ds2, items = _batch(second, 80)
        outs2 = model.inference_ragged(items, noises=[d["z"][0] for d in ds2], bucket=BUCKET)
        assert _bucket_plans(model) == {key: plan} and _bucket_plans(model)[key] is plan
        ds3, items = _batch(across, 90)
        model.inference_ragged(items, noises=[d["z"][0] for d in ds3], bucket=BUCKET)
        assert sorted(k[2] for k in _bucket_plans(model)) == [48, 64] and _bucket_plans(model)[key] is plan
        for k, v in keyed.items():  # the shape-keyed plan: same key, same object
            assert model._plans[k] is v
        assert sum(k[0] == "ragged" for k in model._plans) == 1
        # (the B = 1 plans come last: they share the model's LRU with the plans counted above)
        for (t, _), o, k, d in zip(first, outs1, shape_keyed, ds1):
            assert o.shape == (t, 80)
            assert nerr(o, _single(model, d)) < 2e-5 and nerr(o, k) < 2e-5
        for (t, _), o, d in zip(second, outs2, ds2):
            assert o.shape == (t, 80) and nerr(o, _single(model, d)) < 2e-5


def test_bucketed_batch_draws_its_noise_like_the_b1_loop(model):
    """without `noises` the draw is per item on the CPU generator in item order, as a loop of B = 1 calls draws it"""
    shapes = [(12, 9), (7, 14)]
    ds, items = _batch(shapes, 40)
    with _serenade_ragged_emul.installed():
        torch.manual_seed(5)
        outs = model.inference_ragged(items, bucket=BUCKET)
        torch.manual_seed(5)
        singles = [model.inference(d["x"], d["lengths"], d["midi"], d["lft"], d["ref_x"], d["ref_lengths"],
                                   d["ref_logmel"], d["ref_midi"], d["ref_lft"]) for d in ds]
    for o, s in zip(outs, singles):
        assert nerr(o, s) < 2e-5


def test_validation_comes_before_any_plan(model):
    ds, items = _batch([(12, 9), (7, 14)], 40)
    short = list(items[0])
    short[1] = short[1][:-1]  # midi one row short of its source
    short_ref = list(items[1])
    short_ref[5] = short_ref[5][:-2]  # ref_midi two rows short of its prompt
    tiny = [tuple(t[:3] for t in it) for it in items]  # no track reaches the reflection padding's 4 rows
    empty = [tuple(t[:0] if i < 3 else t for i, t in enumerate(items[0]))]
    with _serenade_ragged_emul.installed():
        model._plans.clear()
        model.cfm_decoder.estimator._plans.clear()
        for bad in ([], [tuple(short), items[1]], [items[0], tuple(short_ref)], tiny, empty):
            with pytest.raises(ValueError):
                model.inference_ragged(bad, bucket=BUCKET)
        for bucket in (0, -64, 1.5, True):
            with pytest.raises(ValueError):
                model.inference_ragged(items, bucket=bucket)
        assert model._plans == {} and model.cfm_decoder.estimator._plans == {}


def test_style_encoder_lengths_equal_each_prompt_alone(model):
    """forward(speech, lengths=): odd heights at every layer (33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1), a full item, a short
    one; then a batch of short prompts on the same plan, the rows behind them full of the earlier batch and of NaN"""
    gst = model.gst
    rng = np.random.default_rng(3)
    speech = torch.from_numpy(rng.standard_normal((4, 40, 80)).astype(np.float32))
    with _serenade_ragged_emul.installed():
        gst._plans.clear()
        for lens in ((33, 40, 5, 1), (3, 2, 7, 6)):
            padded = speech.clone()
            for b, n in enumerate(lens):
                padded[b, n:] = float("nan")
            out = gst(padded, lengths=lens)
            assert len(gst._plans) == 1
            for b, n in enumerate(lens):
                assert nerr(out[b:b + 1], gst(speech[b:b + 1, :n].contiguous())) < 5e-5, (lens, b)
        for bad in ((33, 40, 5), (33, 41, 5, 1), (33, 40, 5, 0)):
            with pytest.raises(ValueError):
                gst(speech, lengths=bad)
        assert torch.equal(gst(speech), gst(speech, lengths=None))  # no lengths: today's op list


def test_cli_ragged_plan_flag(tmp_path):
    """--ragged-plan: the one-by-one loop and the batched path both go through inference_ragged(bucket=RAGGED_BUCKET)
    -- never through Serenade.inference -- and write what the default loop writes; without the flag no call carries a
    bucket"""
    assert models.RAGGED_BUCKET == 64
    argv = cli._two_style_tree(tmp_path)
    calls = []
    real_ragged, real_single = models.Serenade.inference_ragged, models.Serenade.inference

    def ragged(self, items, *a, **k):
        calls.append(("ragged", len(items), k.get("bucket")))
        return real_ragged(self, items, *a, **k)

    def single(self, *a, **k):
        calls.append(("single", 1, None))
        return real_single(self, *a, **k)

    outs, seen = {}, {}
    with contextlib.ExitStack() as st:
        st.enter_context(_serenade_ragged_emul.installed())
        st.enter_context(mock.patch.object(torch.cuda, "is_available", return_value=False))
        st.enter_context(mock.patch.object(models.Serenade, "inference_ragged", ragged))
        st.enter_context(mock.patch.object(models.Serenade, "inference", single))
        for name, extra in (("loop", []), ("plan", ["--ragged-plan"]),
                            ("plan_utts", ["--ragged-plan", "--batch-utterances", "2"])):
            del calls[:]
            torch.manual_seed(7)
            ssc_decode.main(argv + ["--outdir", str(tmp_path / name)] + extra)
            outs[name], seen[name] = sorted(os.listdir(tmp_path / name)), list(calls)
    assert seen["loop"] == [("single", 1, None)] * 4
    assert seen["plan"] == [("ragged", 1, 64)] * 4
    assert seen["plan_utts"] == [("ragged", 4, 64)]
    assert outs["loop"] == outs["plan"] == outs["plan_utts"] and len(outs["loop"]) == 12
    for f, other in [(f, o) for f in outs["loop"] for o in ("plan", "plan_utts")]:
        a, b = tmp_path / "loop" / f, tmp_path / other / f
        if f.endswith(".wav"):
            with wavmod.open(str(a)) as fa, wavmod.open(str(b)) as fb:
                pa = np.frombuffer(fa.readframes(fa.getnframes()), dtype="<i2").astype(np.int32)
                pb = np.frombuffer(fb.readframes(fb.getnframes()), dtype="<i2").astype(np.int32)
            assert pa.shape == pb.shape and np.abs(pa - pb).max() <= 1, f
        else:
            assert np.array_equal(np.load(a)["lf0"], np.load(b)["lf0"]), f
    assert not ssc_decode.build_parser().parse_args(argv + ["--outdir", "o"]).ragged_plan
