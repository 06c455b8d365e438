"""GPU tests of the ragged SiFiGAN: lengths as data from the gather kernel up to SiFiGANGenerator and the stage-9 CLI.

* srn_pd_gather_ragged: every item of a ragged batch is BIT FOR BIT the dense entry point's B = 1 call on that item
  alone; rows past an item's end are neither read (x and d hold NaN there) nor written (they hold a sentinel NaN
  pattern, as do guard bands around the output);
* the generator: across contraction launches agreement is to fp32 summation order (srn_conv_gemm may pick another tile
  or K split for T_cap than for T_b), so items are held, against their own dense B = 1 call and against the
  restatement, to the bound tests/test_sifigan.py uses: 1e-4 of the item's maximum, 1e-3 in bf16x3; both outputs are
  exactly zero past an item's end; stale rows of a reused plan, the bucket edges and the untouched dense plan likewise;
* serenade-postprocessing batch_utterances=N writes what the one-by-one loop writes.

The file's name sorts it behind every other test file: these cases run after the suite that was there before them.
"""
import ctypes
import logging
import math
import os
import wave as wavmod

import numpy as np
import pytest
import torch

import serenade_amd
from oracle import sifigan_oracle as SO
from serenade_amd import _lib, _shapes, ops, sifigan
from serenade_amd.utils.synth import fill_state_dict
from tests.test_sifigan import SMALL, _inputs, _model, nerr

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # a quiet NaN with a payload: "never written", and poison if it were read as data
GUARD = 256            # floats of guard band on either side of an output
SLOPE = 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def sentinel(n, dev):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def is_sentinel(t):
    return bool((bits(t) == SENTINEL).all())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- the gather
def branchy_r(L, dil, b):
    """r * dilation products for an item of L rows, cycling through every branch of the kernel: r = 0; t - r in {0, -1};
    t + r in {L - 1, L}; r > L; a .5 tie (rounds half-even).  Every product is exact in fp32 for dilation 1 and 4."""
    t = np.arange(L)
    prod = np.select([(t + b) % 7 == k for k in range(7)],
                     [0 * t, t, t + 1, L - 1 - t, L - t, L + 3 + 0 * t, (t % 3) + 0.5]).astype(np.float64)
    return prod, (prod / dil).astype(np.float32)


def gather_case(dev, B, T, C, dil, lens, seed=0):
    """x, d (NaN at every row >= L_b), their finite originals, and the clamped lengths"""
    rng = np.random.default_rng(seed)
    Ls = [min(n, T) for n in lens]
    x_full = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)).to(dev)
    d_full = torch.zeros(B, T, device=dev)
    for b, L in enumerate(Ls):
        d_full[b, :L] = torch.from_numpy(branchy_r(L, dil, b)[1]).to(dev)
    x, d = x_full.clone(), d_full.clone()
    for b, L in enumerate(Ls):
        x[b, L:] = float("nan")
        d[b, L:] = float("nan")
    return x, d, x_full, d_full, Ls


def check_gather(dev, B, T, C, dil, lens):
    x, d, x_full, d_full, Ls = gather_case(dev, B, T, C, dil, lens)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    buf = sentinel(2 * GUARD + B * T * 3 * C, dev)
    out = buf[GUARD:GUARD + B * T * 3 * C].view(B, T, 3 * C)
    ops.pd_gather_op(x, d, (buf, GUARD), B, T, C, dil, SLOPE, lens=lens_dev)()
    torch.cuda.synchronize()
    for b, L in enumerate(Ls):
        ref = sentinel(L * 3 * C, dev)  # compact copies: nothing behind the item
        ops.pd_gather_op(x_full[b, :L].contiguous(), d_full[b, :L].contiguous(), ref, 1, L, C, dil, SLOPE)()
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(bits(out[b, :L]), bits(ref.view(L, 3 * C))), f"item {b} (L = {L}) differs from its dense B = 1 call"
        assert is_sentinel(out[b, L:]), f"item {b}: rows past its end were written"
    assert is_sentinel(buf[:GUARD]) and is_sentinel(buf[-GUARD:])
    return buf, x, d, lens_dev


@pytest.mark.parametrize("dil", [1, 4])
@pytest.mark.parametrize("T", [1, 9, 70])  # 70 x 32 / 4 = 560 float4s: three workgroups
@pytest.mark.parametrize("C", [4, 32, 64])
def test_pd_gather_ragged_is_the_dense_b1_call_bit_for_bit(dev, C, T, dil):
    check_gather(dev, 4, T, C, dil, (1, 2, T // 2 + 1, T))


def test_pd_gather_ragged_clamps_a_length_past_T_and_validates(dev):
    B, T, C = 3, 9, 32
    buf, x, d, lens_dev = check_gather(dev, B, T, C, 4, (T + 5, 3, 1 << 30))
    fn = _lib.lib().srn_pd_gather_ragged
    before = buf.clone()
    out_ptr = buf.data_ptr() + 4 * GUARD
    assert fn(x.data_ptr(), d.data_ptr(), None, out_ptr, B, T, C, 4.0, SLOPE, stream()) == -1
    assert b"pd_gather_ragged" in _lib.lib().srn_last_error()
    for bad in ((None, d.data_ptr(), out_ptr, B, T, C), (x.data_ptr(), None, out_ptr, B, T, C),
                (x.data_ptr(), d.data_ptr(), None, B, T, C), (x.data_ptr(), d.data_ptr(), out_ptr, 0, T, C),
                (x.data_ptr(), d.data_ptr(), out_ptr, B, 0, C), (x.data_ptr(), d.data_ptr(), out_ptr, B, T, 30)):
        xa, da, oa, Ba, Ta, Ca = bad
        assert fn(xa, da, lens_dev.data_ptr(), oa, Ba, Ta, Ca, 4.0, SLOPE, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(before))


def test_pd_gather_ragged_grid_stride_loop_runs_more_than_once(dev):
    """L_b * C / 4 = 16 400 * 128 > 8192 * 256: the grid is capped, the loop's second pass covers the last rows"""
    B, T, C, dil = 2, 16400, 512, 4
    assert T * (C // 4) > 8192 * 256
    lens = (3, T)
    rng = np.random.default_rng(5)
    x_full = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)).to(dev)
    d_full = torch.from_numpy((rng.integers(0, 3 * T, (B, T)) / 8.0).astype(np.float32)).to(dev)  # r up to 1.5 T
    x, d = x_full.clone(), d_full.clone()
    x[0, 3:], d[0, 3:] = float("nan"), float("nan")
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    buf = sentinel(2 * GUARD + B * T * 3 * C, dev)
    out = buf[GUARD:GUARD + B * T * 3 * C].view(B, T, 3 * C)
    ops.pd_gather_op(x, d, (buf, GUARD), B, T, C, dil, SLOPE, lens=lens_dev)()
    torch.cuda.synchronize()
    for b, L in enumerate(lens):
        ref = sentinel(L * 3 * C, dev)
        ops.pd_gather_op(x_full[b, :L].contiguous(), d_full[b, :L].contiguous(), ref, 1, L, C, dil, SLOPE)()
        torch.cuda.synchronize()
        assert torch.equal(bits(out[b, :L]), bits(ref.view(L, 3 * C))), f"item {b}"
        assert is_sentinel(out[b, L:])
    assert is_sentinel(buf[:GUARD]) and is_sentinel(buf[-GUARD:])


# ---------------------------------------------------------------------------------------------------- the generator
@pytest.fixture(params=["fp32", "bf16x3"])
def model_tol(request):
    """the arithmetic modes of tests/test_sifigan.py with its bounds"""
    serenade_amd.set_precision(request.param)
    yield 1e-4 if request.param == "fp32" else 1e-3
    serenade_amd.set_precision("fp32")  # the package default


def items_of(cfg, lens, dev, seed=0):
    """([(x, c, [d_i]) on the CPU], the same on the GPU), each item drawn on its own"""
    host = [_inputs(cfg, 1, T, seed=seed + 10 * b) for b, T in enumerate(lens)]
    return host, [(x.to(dev), c.to(dev), [t.to(dev) for t in d]) for x, c, d in host]


def nan_padded(cfg, items, T=None):
    """the items side by side in dense (B, ., T) tensors, NaN behind every item's end"""
    T = max(c.shape[2] for _, c, _ in items) if T is None else T
    hop = items[0][0].shape[2] // items[0][1].shape[2]
    ups = [d.shape[2] // items[0][1].shape[2] for d in items[0][2]]
    B, dev = len(items), items[0][1].device
    x = torch.full((B, 1, T * hop), float("nan"), device=dev)
    c = torch.full((B, cfg["in_channels"], T), float("nan"), device=dev)
    ds = [torch.full((B, 1, T * u), float("nan"), device=dev) for u in ups]
    for b, (xb, cb, db) in enumerate(items):
        n = cb.shape[2]
        x[b, :, :n * hop], c[b, :, :n] = xb[0], cb[0]
        for dst, src, u in zip(ds, db, ups):
            dst[b, :, :n * u] = src[0]
    return x, c, ds


def check_items(g, items, outs, tol, what, w=None, cfg=None, host=None):
    """every item against its own dense B = 1 forward and, with w, against the restatement on the item alone"""
    for i, ((x, c, d), (y, e)) in enumerate(zip(items, outs)):
        y1, e1 = g(x, c, d)
        assert y.shape == e.shape == (c.shape[2] * g.hop,) and torch.isfinite(y).all() and torch.isfinite(e).all(), what
        ey, ee = nerr(y, y1.view(-1)), nerr(e, e1.view(-1))
        print(f"{what}: item of {c.shape[2]} frames vs its own B = 1 call: wave {ey:.2e} exc {ee:.2e} (< {tol:g})")
        assert ey < tol and ee < tol, f"{what}: item of {c.shape[2]} frames vs its own B = 1 call"
        if w is not None:
            y_ref, e_ref = SO.sifigan_forward(w, *host[i], cfg)
            assert torch.isfinite(y_ref).all() and torch.isfinite(e_ref).all()
            ey, ee = nerr(y, y_ref.view(-1)), nerr(e, e_ref.view(-1))
            print(f"{what}: item of {c.shape[2]} frames vs the restatement: wave {ey:.2e} exc {ee:.2e} (< {tol:g})")
            assert ey < tol and ee < tol, f"{what}: item of {c.shape[2]} frames vs the restatement"


@pytest.mark.parametrize("small,lens", [(True, (11, 4, 1, 7)), (False, (24, 9, 1))], ids=["small", "default"])
def test_generator_ragged_equals_b1_runs_and_the_restatement(dev, model_tol, small, lens):
    cfg = SMALL if small else sifigan.DEFAULT_PARAMS
    g, w = _model(cfg, seed=0 if small else 2)
    g = g.to(dev)
    host, items = items_of(cfg, lens, dev, seed=3)
    outs = g.inference_ragged(items)
    pl = g.plan_ragged(len(lens), max(lens))
    yb, eb = g(*nan_padded(cfg, items), lengths=lens)
    assert g.plan_ragged(len(lens), max(lens)) is pl
    check_items(g, items, outs, model_tol, "inference_ragged", w, cfg, host)
    assert yb.shape == eb.shape == (len(lens), 1, max(lens) * g.hop)
    for n, (y, e), yrow, erow in zip(lens, outs, yb, eb):
        assert torch.equal(yrow[0, :n * g.hop], y) and torch.equal(erow[0, :n * g.hop], e)
        assert bool((yrow[0, n * g.hop:] == 0).all()) and bool((erow[0, n * g.hop:] == 0).all())
    assert bool((pl.wave == 0)[0, lens[0] * g.hop:].all()) and bool((pl.exc == 0)[0, lens[0] * g.hop:].all())  # to T_cap


def test_short_batch_after_a_long_one_reuses_the_plan_and_ignores_stale_rows(dev, model_tol):
    """the case a missing mask hides: rows past an item's end hold the PREVIOUS batch's data, not zeros.  Same bucket,
    so the same plan object -- and, with graphs on, the same captured graph replayed over new lengths"""
    g, w = _model(SMALL)
    g = g.to(dev)
    _, long_ = items_of(SMALL, (60, 50, 64, 33), dev, seed=21)
    _, short = items_of(SMALL, (11, 4, 1, 7), dev, seed=22)
    g.inference_ragged(long_)
    pl = g.plan_ragged(4, 64)
    outs = g.inference_ragged(short)
    assert g.plan_ragged(4, 11) is pl and pl.T == 64
    check_items(g, short, outs, model_tol, "eager")
    ops.set_graphs(True)
    try:
        g._invalidate()
        g.inference_ragged(long_)            # eager warm-up of a new plan
        first = g.inference_ragged(long_)    # captured
        pl = g.plan_ragged(4, 64)
        replay = g.inference_ragged(short)   # replayed over new lengths and the long batch's leftovers
        assert g.plan_ragged(4, 11) is pl
    finally:
        ops.set_graphs(False)
    for (ya, ea), (yb, eb) in zip(replay, outs):
        assert torch.equal(ya, yb) and torch.equal(ea, eb)
    check_items(g, long_, first, model_tol, "captured")


def test_bucket_edges_length_validation_and_the_dense_plan(dev, model_tol):
    g, w = _model(SMALL)
    g = g.to(dev)
    _, probe = items_of(SMALL, (13,), dev, seed=31)
    y0, e0 = g(*probe[0])  # the dense plan, before any ragged call
    plans = []
    for top, cap in ((64, 64), (65, 128)):
        _, items = items_of(SMALL, (top, 7), dev, seed=top)
        outs = g.inference_ragged(items)
        plans.append(g.plan_ragged(2, top))
        assert plans[-1].T == cap
        check_items(g, items, outs, model_tol, f"batch maximum {top}")
    assert plans[0] is not plans[1]
    y1, e1 = g(*probe[0])
    assert torch.equal(bits(y1), bits(y0)) and torch.equal(bits(e1), bits(e0)), "the dense forward changed"
    assert g.plan_ragged(2, 64) is plans[0], "a miss in the dense plan() cleared the ragged plans"
    g._invalidate()
    _, two = items_of(SMALL, (5, 11), dev)
    x, c, d = nan_padded(SMALL, two)
    for bad in ((5,), (5, 11, 3), (0, 11), (5, 12)):
        with pytest.raises(ValueError):
            g(x, c, d, lengths=bad)
    assert not g._ragged_plans and not g._plans, "validation comes before any plan is built or launched"


# ---------------------------------------------------------------------------------------------------- the CLI
def _pcm(path):
    with wavmod.open(str(path)) as f:
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int32)


def _stage9_argv(tmp_path):
    """a synthetic checkpoint and stats, as tests/test_world.py builds its own; returns run -> argv"""
    from joblib import dump
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(11)
    scaler = {"mcep": StandardScaler().fit(rng.standard_normal((60, 40)) * 2 - 1),
              "bap": StandardScaler().fit(rng.standard_normal((60, 3)) * 10 - 20)}
    dump(scaler, tmp_path / "stats.joblib")
    sd = fill_state_dict(_shapes.as_meta(sifigan.sifigan_shapes(**sifigan.DEFAULT_PARAMS)), seed=5)
    torch.save({"model": {"generator": sd}}, tmp_path / "model.pkl")
    return lambda run: ["generator=sifigan", f"in_dir={tmp_path / run}", f"stats={tmp_path / 'stats.joblib'}",
                        f"checkpoint_path={tmp_path / 'model.pkl'}", "seed=31"]


def _write_song(d, name, seconds, seed, contour="own"):
    """NAME.wav (PCM_16) and its 10 ms lf0 contour as the decode CLI writes it; contour: own | silent | too_high"""
    from serenade_amd.utils.io import write_wav_pcm16
    from tests.test_world import FS, song
    x, f0 = song(seconds, seed)
    write_wav_pcm16(str(d / f"{name}.wav"), 0.9 * x / np.abs(x).max(), FS)
    lf0 = f0[::2].astype(np.float32)
    np.savez(d / f"{name}.npz", lf0={"own": lf0, "silent": 0 * lf0, "too_high": 0 * lf0 + 7000.0}[contour])


def _same_outputs(tmp_path, want):
    """both runs wrote exactly `want`, PCM_16 samples within ceil(1e-4 * 32768) + 1 LSB (PostJob writes files and hands
    no float waveform back)"""
    names = sorted(n for n in os.listdir(tmp_path / "loop" / "test") if n.endswith("_sifigan.wav"))
    assert names == [f"{n}_sifigan.wav" for n in want]
    assert names == sorted(n for n in os.listdir(tmp_path / "batched" / "test") if n.endswith("_sifigan.wav"))
    lsb = math.ceil(1e-4 * 32768) + 1
    for n in names:
        pa, pb = _pcm(tmp_path / "loop" / "test" / n), _pcm(tmp_path / "batched" / "test" / n)
        assert pa.shape == pb.shape and pa.size > 0 and np.abs(pa).max() > 16
        print(f"{n}: {pa.size} samples, max |difference| {np.abs(pa - pb).max()} LSB (<= {lsb})")
        assert np.abs(pa - pb).max() <= lsb, n


def test_cli_batch_utterances_writes_what_the_loop_writes(dev, tmp_path):
    """four wavs of distinct lengths (one without a voiced frame) and one without a contour through the default loop
    and through batch_utterances=3, the default noise_amp and the same seed: the same files, the same samples"""
    from serenade_amd.bin import ssc_postprocessing as PP
    from serenade_amd.utils.io import write_wav_pcm16
    from tests.test_world import FS, song
    argv = _stage9_argv(tmp_path)
    for run in ("loop", "batched"):
        d = tmp_path / run / "test"
        d.mkdir(parents=True)
        for name, seconds, seed in (("a_song", 0.30, 7), ("b_silent", 0.22, 8), ("c_song", 0.41, 9), ("d_song", 0.26, 10)):
            _write_song(d, name, seconds, seed, "silent" if name == "b_silent" else "own")
        write_wav_pcm16(str(d / "b_no_contour.wav"), song(0.30, 7)[0] * 0.1, FS)
    serenade_amd.set_precision("fp32")
    frames = PP.main(argv("loop"))
    frames_b = PP.main(argv("batched") + ["batch_utterances=3"])
    assert frames == frames_b > 0
    _same_outputs(tmp_path, ("a_song", "c_song", "d_song"))


def test_cli_bad_files_are_skipped_alone_in_a_group(dev, tmp_path, caplog):
    """batch_utterances=5 over seven files.  The first group holds a contour file that cannot be read and a wav that
    cannot be used (two channels) between three good files: those two are skipped alone and the three go through one
    ragged call.  The second group holds a contour the analysis refuses: the group falls back to the one-by-one loop,
    which skips that file alone.  The same files and samples as the default loop, which skips the same three."""
    from serenade_amd.bin import ssc_postprocessing as PP
    from tests.test_world import FS
    argv = _stage9_argv(tmp_path)
    for run in ("loop", "batched"):
        d = tmp_path / run / "test"
        d.mkdir(parents=True)
        for name, seconds, seed, contour in (("a_song", 0.30, 7, "own"), ("b_bad_contour_file", 0.24, 8, "own"),
                                             ("c_stereo", 0.24, 9, "own"), ("d_song", 0.26, 10, "own"),
                                             ("e_song", 0.35, 11, "own"), ("f_refused", 0.24, 12, "too_high"),
                                             ("g_song", 0.28, 13, "own")):
            _write_song(d, name, seconds, seed, contour)
        (d / "b_bad_contour_file.npz").write_bytes(b"not an archive of arrays " * 4)
        with wavmod.open(str(d / "c_stereo.wav"), "wb") as f:
            f.setnchannels(2)
            f.setsampwidth(2)
            f.setframerate(FS)
            f.writeframes(np.zeros(2 * 4800, dtype="<i2").tobytes())
    serenade_amd.set_precision("fp32")
    frames = PP.main(argv("loop"))
    caplog.clear()
    with caplog.at_level(logging.ERROR):
        frames_b = PP.main(argv("batched") + ["batch_utterances=5"])
    errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
    print("\n".join(errors))
    assert len(errors) == 4 and "b_bad_contour_file.wav" in errors[0] and "c_stereo.wav" in errors[1]
    assert errors[0].startswith("skipped") and errors[1].startswith("skipped")
    assert "not analysed together" in errors[2] and errors[3].startswith("skipped") and "f_refused.wav" in errors[3]
    assert frames == frames_b > 0
    _same_outputs(tmp_path, ("a_song", "d_song", "e_song", "g_song"))
