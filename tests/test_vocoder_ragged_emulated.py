"""The ragged vocoder's host logic on the CPU, through the C-ABI emulator plus the executable specifications of the two
ragged entry points (tests/_vocoder_ragged_emul.py): the ragged HiFiGANPlan (per-stage lengths, len_in on every conv,
bucketed capacity, plan reuse), the public additions of HiFiGANGenerator / Vocoder, and `serenade-decode
--ragged-vocoder`.  The kernels themselves are tests/test_zz_hip_vocoder_ragged.py (GPU)."""
import os
import wave as wavmod

import numpy as np
import pytest
import torch

from oracle import serenade_oracle as O
from serenade_amd import ops, vocoder
from serenade_amd.bin import ssc_decode
from tests import _vocoder_ragged_emul
from tests.test_cli import _emulated, _two_style_tree
from tests.test_plan_emulated import _gen

LENS = (3, 17, 32, 9)
JUNK = 1.0e3  # what rows past an item's end hold (finite: the emulator's conv masks its input by a product)


def nerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _mels(lens, seed=0, width=80):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal((n, width)).astype(np.float32)) for n in lens]


def _padded(mels, T=None):
    T = max(m.shape[0] for m in mels) if T is None else T
    c = torch.full((len(mels), T, mels[0].shape[1]), JUNK)
    for b, m in enumerate(mels):
        c[b, :m.shape[0]] = m
    return c


@pytest.mark.parametrize("small,lens", [(True, LENS), (False, (3, 8, 5))], ids=["small", "full"])
def test_ragged_generator_equals_b1_runs_and_the_oracle(monkeypatch, small, lens):
    """every item of one ragged call = its own B = 1 call = the oracle's HiFi-GAN on that item alone (the bound of the
    dense generator in tests/test_plan_emulated.py); the lengths= form is zero past each item's end.  (The full-size
    generator runs few frames in a bucket of 8: the emulator is slow, and the host logic does not depend on the size.)"""
    if not small:
        monkeypatch.setattr(vocoder, "RAGGED_BUCKET", 8)
    gen, w, params = _gen(small=small)
    mels = _mels(lens, seed=5)
    with _vocoder_ragged_emul.installed():
        outs = gen.inference_ragged(mels)
        singles = [gen.inference_batch(m.unsqueeze(0)) for m in mels]
        yb = gen.inference_batch(_padded(mels), lengths=lens)
    assert yb.shape == (len(lens), 1, max(lens) * gen.hop)
    for n, m, o, s, y in zip(lens, mels, outs, singles, yb):
        assert o.shape == (n * gen.hop,)
        assert nerr(o, s.view(-1)) < 1e-4
        assert nerr(o, O.hifigan_forward(w, m.t().unsqueeze(0), params).view(-1)) < 1e-4
        assert torch.equal(y[0, :n * gen.hop], o) and not y[0, n * gen.hop:].any()


def test_ragged_plan_is_bucketed_reused_and_masks_stale_rows():
    """batch maxima of 64 / 65 frames give capacities 64 / 128; a batch of short items after a batch of long ones runs
    on the same plan object, over the long batch's leftovers, and still equals the B = 1 runs"""
    gen, w, params = _gen(small=True)
    with _vocoder_ragged_emul.installed():
        assert gen.plan_ragged(2, 64).T == 64 and gen.plan_ragged(2, 65).T == 128
        assert gen.plan_ragged(2, 65, bucket=1).T == 65
        long_, short = _mels((40, 33), seed=1), _mels((5, 11), seed=2)
        gen.inference_ragged(long_)
        pl = gen.plan_ragged(2, 40)
        outs = gen.inference_ragged(short)
        assert gen.plan_ragged(2, 11) is pl and pl.T == 64
        assert pl.lens.tolist() == [[5 * s, 11 * s] for s in pl.scales]
        for m, o in zip(short, outs):
            assert nerr(o, gen.inference_batch(m.unsqueeze(0)).view(-1)) < 1e-4
        for bad in ((5,), (0, 11), (5, 12)):
            with pytest.raises(ValueError):
                gen.inference_batch(_padded(short), lengths=bad)
        with pytest.raises(ValueError):
            gen.inference_ragged([])


def test_vocoder_decode_ragged_equals_decode(monkeypatch):
    monkeypatch.setattr(vocoder, "RAGGED_BUCKET", 8)  # few frames of the full-size generator: the emulator is slow
    gen, w, params = _gen()
    one = np.ones(80, dtype=np.float32)
    rng = np.random.default_rng(3)
    stats = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one + 0.1}
    trg = {"mean": rng.standard_normal(80).astype(np.float32) * 0.1, "scale": one * 0.9}
    lens = (3, 8, 5)
    mels = _mels(lens, seed=7)
    with _vocoder_ragged_emul.installed():
        voc = vocoder.Vocoder.from_generator(gen, {"sampling_rate": 24000}, stats, torch.device("cpu"), trg_stats=trg)
        waves = voc.decode_ragged(mels)
        wb = voc.decode_batch(_padded(mels), lengths=lens)
        singles = [voc.decode(m)[0] for m in mels]
    for n, m, o, s, y in zip(lens, mels, waves, singles, wb):
        ref = O.vocoder_decode(w, m, params, {k: torch.from_numpy(v) for k, v in stats.items()},
                               {k: torch.from_numpy(v) for k, v in trg.items()})
        assert (o - s).abs().max().item() < 2e-5 and (o - ref).abs().max().item() < 2e-5
        assert torch.equal(y[:n * gen.hop], o) and not y[n * gen.hop:].any()


def _count_ragged_ops(monkeypatch):
    """the entry names ending in _ragged of every op built from here on"""
    built = []
    for cls in (ops._StructOp, ops.CallOp):  # both take the entry name first
        def init(self_, name, args, _init=cls.__init__):
            if name.endswith("_ragged"):
                built.append(name)
            _init(self_, name, args)
        monkeypatch.setattr(cls, "__init__", init)
    return built


def test_cli_ragged_vocoder_writes_what_the_loop_writes(tmp_path, monkeypatch):
    """--batch-utterances 2 --ragged-vocoder: the same files as the one-by-one loop, lf0 equal, PCM_16 within 1 LSB
    (the criterion tests/test_cli.py applies to --batch-utterances); without the flag no ragged op is ever built"""
    argv = _two_style_tree(tmp_path)
    built = _count_ragged_ops(monkeypatch)
    outs = {}
    with _emulated(), _vocoder_ragged_emul.installed():
        for name, extra in (("loop", []), ("utts", ["--batch-utterances", "2"]),
                            ("ragged", ["--batch-utterances", "2", "--ragged-vocoder"])):
            torch.manual_seed(7)
            ssc_decode.main(argv + ["--outdir", str(tmp_path / name)] + extra)
            outs[name] = sorted(os.listdir(tmp_path / name))
            if name == "utts":
                assert not built, "without --ragged-vocoder nothing builds a ragged op"
        with pytest.raises(SystemExit):
            ssc_decode.main(argv + ["--outdir", str(tmp_path / "bad"), "--ragged-vocoder"])
    assert "srn_hifigan_resunit_ragged" in built and "srn_out_conv_tanh_ragged" in built
    assert outs["loop"] == outs["ragged"] and len(outs["loop"]) == 12
    for f in outs["loop"]:
        a, b = tmp_path / "loop" / f, tmp_path / "ragged" / f
        if f.endswith(".wav"):
            with wavmod.open(str(a)) as fa, wavmod.open(str(b)) as fb:
                pa = np.frombuffer(fa.readframes(fa.getnframes()), dtype="<i2").astype(np.int32)
                pb = np.frombuffer(fb.readframes(fb.getnframes()), dtype="<i2").astype(np.int32)
            assert pa.shape == pb.shape and np.abs(pa - pb).max() <= 1, f
        else:
            assert np.array_equal(np.load(a)["lf0"], np.load(b)["lf0"]), f
