"""The WORLD analysis kernels (csrc/world.hip) on the MI355X against the float64 oracle at edge shapes: every F0 branch
of CheapTrick and D4C (default F0 at and next to the floor, the largest window that fits, the 40 / 47 Hz floors, windows
of a handful of samples), the three transform sizes of CheapTrick and both of D4C (fs = 12000 is the 1024-point
d4c_kernel), signals shorter than one window, the padding of a ragged batch, the contour and excitation kernels past
one 256-frame chunk, and the small kernels through the C entry points with leading dimensions of their own.

The cases, references and bounds are tests/_world_cases.py's; tests/test_world_cases_host.py shows on the CPU that the
cases are well conditioned and off the Love-Train threshold, so that the bounds here judge the kernels."""
import numpy as np
import pytest
import torch

from oracle import world_oracle as W
from serenade_amd import ops, world
from tests import _world_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cuda(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(device=DEV, dtype=dtype)


def _host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ A. CheapTrick
@pytest.mark.parametrize("case", C.CT_CASES, ids=repr)
def test_cheaptrick_and_sp2mc(case):
    sp_ref, mc_ref = C.ct_ref(case)
    sp = world.cheaptrick(_cuda(case.x), _cuda(case.f0), _cuda(case.t), case.fs, fft_size=case.fft_size)
    assert sp.shape == sp_ref.shape and sp.dtype == torch.float64
    err = float(np.abs(np.log(_host(sp) / sp_ref)).max())
    mc = _host(world.sp2mc(sp, C.ORDER, world.ALPHA[case.fs]))
    err_mc = float(np.abs(mc - mc_ref).max())
    print(f"{case}: log envelope {err:.2e}, mel-cepstrum {err_mc:.2e}")
    assert err < C.TOL, (case, err)
    assert err_mc < C.TOL, (case, err_mc)


# ------------------------------------------------------------------------------------------------ B. D4C
@pytest.mark.parametrize("case", C.D4C_CASES, ids=repr)
def test_d4c(case):
    ref, _ = C.d4c_ref(case)
    got = _host(world.d4c_band_aperiodicity(_cuda(case.x), _cuda(case.f0), _cuda(case.t), case.fs))
    assert got.shape == ref.shape
    # properties, on every frame: finite, a frame is unvoiced as a whole or not at all, voiced bands lie in [-60, 0] dB
    assert np.isfinite(got).all()
    unv = got == C.UNVOICED
    assert (unv.all(axis=1) | ~unv.any(axis=1)).all()
    voiced, voiced_ref = C.voiced_rows(got), C.voiced_rows(ref)
    assert (got[voiced] <= 0.0).all() and (got[voiced] >= -60.0).all()
    # the decision: equal to the oracle's on every frame off the threshold (all of them, but for the short signals)
    decided, compared = C.d4c_decided(case), C.d4c_compared(case)
    assert np.array_equal(voiced[decided], voiced_ref[decided]), (case, np.nonzero(voiced != voiced_ref)[0])
    both = compared & voiced & voiced_ref
    err = float(np.abs(got[both] - ref[both]).max(initial=0.0))
    print(f"{case}: {int(voiced.sum())} of {len(got)} frames voiced, {int(both.sum())} compared: {err:.2e} dB")
    assert err < C.TOL, (case, err)
    if case.kind == "pulses":
        assert both.all()
    elif case.kind == "unvoiced":
        assert unv.all()  # bit for bit the unvoiced constant


# ------------------------------------------------------------------------------------------------ C. ragged padding
def _poison(shapes):
    """leave NaN in the blocks the allocator will hand out next: a few MB, and blocks of the very sizes asked for"""
    junk = [torch.full((1 << 20,), float("nan"), dtype=torch.float64, device=DEV)]
    junk += [torch.full(s, float("nan"), dtype=torch.float64, device=DEV) for s in shapes for _ in range(2)]
    torch.cuda.synchronize()
    del junk


def test_ragged_batch_padding_is_zero():
    b = C.ragged_batch()
    waves, n, lf0, F = b["waves"], b["lengths"], list(b["lf0"]), b["frames"]
    buf = np.zeros((3, max(n)), dtype=np.float32)
    for i, w in enumerate(waves):
        buf[i, :n[i]] = w
    an = world.Analyzer(scaler={"mcep": C.Scaler(b["mean"][:40], b["scale"][:40]),
                                "bap": C.Scaler(b["mean"][40:], b["scale"][40:])})
    noise = _cuda(b["noise"], torch.float32)
    us = (5, 20, 60, 120)
    _poison([(3, max(F), 513), (3, max(F), 40), (3, max(F), 3)])
    in_signal, c, dfs, feats = an(_cuda(buf, torch.float32), n, lf0, noise=noise)
    assert c.shape == (3, 43, max(F)) and in_signal.shape == (3, 1, max(F) * C.HOP) and feats["n_frames"] == F
    for i in range(3):
        ref = C.ragged_ref(i)
        Fi = F[i]
        # the valid part against the oracle, at the bounds of tests/test_world.py's ragged batch
        got_c = _host(c[i, :, :Fi].T)
        got_bap = _host(feats["bap"][i, :Fi])
        flips = (got_bap == C.UNVOICED).all(1) != (ref["bap"] == C.UNVOICED).all(1)
        assert not flips.any(), (i, np.nonzero(flips)[0])  # every frame is off the threshold (host test)
        assert np.abs(got_bap - ref["bap"]).max() < 1e-6
        assert np.abs(_host(feats["mcep"][i, :Fi]) - ref["mcep"]).max() < 1e-6
        assert np.abs(got_c[:, :40] - ref["c"][:, :40]).max() < 1e-5      # float32 output
        assert np.abs(got_c[:, 40:] - ref["c"][:, 40:]).max() < 1e-4
        assert np.array_equal(_host(feats["f0"][i, :Fi]), ref["f0"])
        assert np.array_equal(_host(feats["cf0"][i, :Fi]), ref["cf0"])
        assert np.array_equal(_host(feats["uv"][i, :Fi]), ref["uv"])
        assert ref["ok"] and int(feats["ok"][i]) == 1
        for d, dref, u in zip(dfs, ref["dfs"], us):
            assert np.array_equal(_host(d[i, 0, :Fi * u]), dref.astype(np.float32))
        sref = C.excitation_ref(ref["cf0"], b["noise"][i:i + 1, :, :Fi * C.HOP])
        assert np.abs(_host(in_signal[i, 0, :Fi * C.HOP]) - sref).max() < C.SINE_TOL
        # the item alone is the item in the batch, bit for bit
        s1, c1, d1, f1 = an(_cuda(buf[i:i + 1, :n[i]], torch.float32), n[i:i + 1], lf0[i:i + 1],
                            noise=noise[i:i + 1, :, :Fi * C.HOP].contiguous())
        assert torch.equal(c1[0], c[i, :, :Fi]) and torch.equal(s1[0, 0], in_signal[i, 0, :Fi * C.HOP])
        for k in ("mcep", "bap", "f0", "cf0", "uv"):
            assert torch.equal(f1[k][0], feats[k][i, :Fi]), (i, k)
        for a, d, u in zip(d1, dfs, us):
            assert torch.equal(a[0, 0], d[i, 0, :Fi * u])
    # past an item's frames everything is exactly zero (NaN is not)
    bad = []
    for i in range(3):
        Fi = F[i]
        tails = {"c": c[i, :, Fi:], "mcep": feats["mcep"][i, Fi:], "bap": feats["bap"][i, Fi:], "f0": feats["f0"][i, Fi:],
                 "cf0": feats["cf0"][i, Fi:], "uv": feats["uv"][i, Fi:], "in_signal": in_signal[i, 0, Fi * C.HOP:]}
        tails.update({f"dfs[{k}]": d[i, 0, Fi * u:] for k, (d, u) in enumerate(zip(dfs, us))})
        bad += [(i, k) for k, v in tails.items() if not bool((v == 0).all())]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ D. contours
def test_match_length_bit_for_bit():
    n_out = [no for _, no in C.MATCH_PAIRS]
    got = _host(world.match_length(list(C.match_inputs()), n_out, DEV))
    assert got.shape == (len(n_out), max(n_out))
    for i, (ref, pair) in enumerate(zip(C.match_refs(), C.MATCH_PAIRS)):
        assert np.array_equal(got[i, :n_out[i]], ref), pair
        assert not got[i, n_out[i]:].any(), pair
    same = [p[0] == p[1] for p in C.MATCH_PAIRS].index(True, 1)
    assert (got[same] < 0).any() and got[0, 0] < 0  # equal lengths: no resampling and no clamp


def test_cont_f0_bit_for_bit_across_chunks():
    items, refs = C.cont_items(), C.cont_refs()
    F = max(C.CONT_LENGTHS)
    f0 = np.zeros((len(items), F))
    for i, (_, f) in enumerate(items):
        f0[i, :len(f)] = f
    nf = torch.tensor([len(f) for _, f in items], dtype=torch.int32, device=DEV)
    uv, cf0, ok = (_host(v) for v in world._cont_f0_raw(_cuda(f0), nf))
    for i, ((label, f), (uv_ref, cf0_ref, ok_ref)) in enumerate(zip(items, refs)):
        n = len(f)
        assert bool(ok[i]) == ok_ref, label
        assert np.array_equal(uv[i, :n], uv_ref) and uv.dtype == np.float32, label
        assert np.array_equal(cf0[i, :n], cf0_ref), (label, np.nonzero(cf0[i, :n] != cf0_ref)[0][:5])
        assert not cf0[i, n:].any() and not uv[i, n:].any(), label
        if not ok_ref:
            assert np.array_equal(cf0[i, :n], f), label


# ------------------------------------------------------------------------------------------------ E. excitation
@pytest.mark.parametrize("sine_f0_type", ["cf0", "f0"])
def test_excitation_past_one_chunk(sine_f0_type):
    e = C.excitation_batch()
    an = world.Analyzer(sine_f0_type=sine_f0_type)
    feats = dict(f0=_cuda(e["f0"]), cf0=_cuda(e["cf0"]),
                 nf=torch.tensor(C.EXC_FRAMES, dtype=torch.int32, device=DEV))
    sine, dfs = an.excitation(feats, noise=_cuda(e["noise"], torch.float32))
    F = max(C.EXC_FRAMES)
    assert sine.shape == (len(C.EXC_FRAMES), 1, F * C.HOP) and sine.dtype == torch.float32
    for b, n in enumerate(C.EXC_FRAMES):
        ref = C.excitation_ref(e[sine_f0_type][b, :n], e["noise"][b:b + 1, :, :n * C.HOP])
        got = _host(sine[b, 0])
        err = float(np.abs(got[:n * C.HOP] - ref).max())
        print(f"excitation from {sine_f0_type}, {n} frames: {err:.2e}")
        assert err < C.SINE_TOL, (n, err)
        assert not got[n * C.HOP:].any()
        for d, dense, u in zip(dfs, an.dense_factors, an.upsample):
            dref = np.repeat(W.dilated_factor(e["cf0"][b, :n, None], C.FS, dense), u).astype(np.float32)
            assert np.array_equal(_host(d[b, 0, :n * u]), dref), (n, dense)
            assert not _host(d[b, 0, n * u:]).any()


# ------------------------------------------------------------------------------------------------ F. small kernels
SENTINEL = -77.25


@pytest.mark.parametrize("K", [257, 513, 1025])
def test_project_rows_and_leading_dimensions(K):
    """bound per element, derived: a dot product of K float64 terms summed in any order errs by at most
    gamma_K |m|^T |g(x)| < 4 K 2^-53 |m|^T |g(x)| (the 4 is slack for the unspecified order and for FMA or not); a log
    good to an ulp or two of a value of magnitude up to 1 adds 2^-52 |m|^T 1, and more of it is inside the first term"""
    rng = np.random.default_rng(K)
    cases = [(rows, n_out, take_log, K, n_out) for rows in (1, 7, 8, 9, 17) for n_out in (1, 40, 64) for take_log in (0, 1)]
    cases += [(17, 40, 1, K + 3, 45), (9, 64, 0, K + 3, 69)]  # ld_in > K, ld_out > n_out
    worst = 0.0
    for rows, n_out, take_log, ld_in, ld_out in cases:
        x = np.exp(rng.uniform(-30.0, 5.0, (rows, ld_in))) if take_log else rng.standard_normal((rows, ld_in))
        m = rng.standard_normal((K, n_out))
        out = torch.full((rows, ld_out), SENTINEL, dtype=torch.float64, device=DEV)
        ops.call("srn_world_project", _cuda(x), rows, K, ld_in, _cuda(m), n_out, take_log, out, ld_out)
        g = np.log(x[:, :K]) if take_log else x[:, :K]
        bound = 4 * K * 2.0 ** -53 * (np.abs(g) @ np.abs(m)) + take_log * 2.0 ** -52 * np.abs(m).sum(axis=0)
        got = _host(out)
        ratio = float((np.abs(got[:, :n_out] - g @ m) / bound).max())
        worst = max(worst, ratio)
        assert ratio < 1.0, (rows, n_out, take_log, ld_in, ratio)
        assert (got[:, n_out:] == SENTINEL).all(), (rows, n_out, ld_out)
    print(f"projection K = {K}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("scaled", [False, True])
def test_pack_features_bit_for_bit(rows, scaled):
    rng = np.random.default_rng(rows)
    na, nb, ld = 40, 3, 48
    a, b = rng.standard_normal((rows, na)) * 3.0, rng.uniform(-60.0, 0.0, (rows, nb))
    mean, scale = rng.standard_normal(na + nb), rng.uniform(0.5, 2.0, na + nb)
    out = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=DEV)
    ops.call("srn_world_pack_features", _cuda(a), na, _cuda(b), nb, _cuda(mean) if scaled else None,
             _cuda(scale) if scaled else None, out, rows, ld)
    v = np.concatenate([a, b], axis=1)
    ref = np.float32((v - mean) / scale) if scaled else np.float32(v)
    got = _host(out)
    assert np.array_equal(got[:, :na + nb], ref)
    assert (got[:, na + nb:] == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("n", [1, 255, 257])
def test_wave_to_f64_bit_for_bit(n):
    special = [1.5, -1.5, 1.0, -1.0, 0.0, 0.99999, -0.99999, 1e-5, 1e-40, -1e-40, 0.5 / 32767, 1.5 / 32767]
    w = np.concatenate([special, np.random.default_rng(n).uniform(-1.2, 1.2, 257 - len(special))]).astype(np.float32)[:n]
    assert n == 1 or (0 < abs(w[8]) < np.finfo(np.float32).tiny)  # a float32 denormal
    for pcm16 in (1, 0):
        out = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
        ops.call("srn_wave_to_f64", _cuda(w, torch.float32), out, n, pcm16)
        got = _host(out)
        ref = W.pcm16_roundtrip(w) if pcm16 else w.astype(np.float64)
        assert np.array_equal(got[:n], ref) and got[n] == SENTINEL, (n, pcm16)
        assert not pcm16 or (got[:n].max() <= 32767 / 32768.0 and got[:n].min() >= -1.0)
