"""The ragged log-mel / loudness front-end (features.logmelfilterbank / loudness_extract with `lengths=`) on the CPU:
the host logic -- padding per item, the plans, the shared constant tables, the argument checks -- through the C-ABI
emulator (tests/_emulator.py plus CPU statements of the three ragged entry points below), at the shapes and to the
bound of the GPU run (tests/test_hip_features_ragged.py; cases in tests/_features_ragged_cases.py).  That the fp32
path stays within 2e-4 of the float64 oracle on these inputs is shown here too.  The kernels themselves are checked on
the GPU."""
import numpy as np
import pytest
import torch

from serenade_amd import features
from tests import _emulator as E
from tests import _features_ragged_cases as C
from tests.test_transcriber_emulated import _tview, emul_transcriber

CPU = torch.device("cpu")


def emul_features(name, a):
    if name == "srn_pad_ragged_zero":
        x, x_bs, lens, out, B, n, pad, ld = a
        xv, ov = _tview(x, B, 1, n, x_bs)[:, 0], _tview(out, B, 1, ld, ld)[:, 0]
        for b in range(B):
            L = min(int(lens[b]), n)
            ov[b] = 0
            ov[b, pad:pad + L] = xv[b, :L]
    elif name == "srn_logmel_ragged":
        spec, mel_t, frames, out, B, T, nb, ld, n_mels, eps, mode = a
        sv, ov = _tview(spec, B, T, ld, T * ld), _tview(out, B, T, n_mels, T * n_mels)
        log = {10: torch.log10, 2: torch.log2, 0: torch.log}[mode]
        for b in range(B):
            L = min(int(frames[b]), T)
            mag = torch.sqrt(sv[b, :L, :nb] ** 2 + sv[b, :L, nb:2 * nb] ** 2)
            ov[b] = 0
            ov[b, :L] = log(torch.clamp(mag @ mel_t, min=eps))
    elif name == "srn_loudness_ragged":
        spec, aw, frames, ws, out, B, T, nb, ld, amin, top_db, add_eps = a
        sv, ov = _tview(spec, B, T, ld, T * ld), _tview(out, B, T, 1, T)[..., 0]
        for b in range(B):
            L = min(int(frames[b]), T)
            if L <= 0:  # no frame of its own: no maximum to take
                ov[b] = 0
                continue
            p = sv[b, :L, :nb] ** 2 + sv[b, :L, nb:2 * nb] ** 2
            db = 10 * torch.log10(torch.clamp(p, min=amin))
            db = torch.maximum(db, db.max() - top_db) + aw
            ov[b] = 0
            ov[b, :L] = torch.log(torch.pow(10.0, 0.05 * db).mean(dim=-1) + add_eps)
    else:
        return emul_transcriber(name, a)  # srn_pad_ragged; everything else is tests/_emulator.py's


@pytest.fixture
def emulated():
    with E.installed():  # restores CallOp.__call__ on exit
        features.ops.CallOp.__call__ = lambda self_, stream=None: emul_features(self_.name, self_.targs)
        features._PLANS.clear()
        yield
    features._PLANS.clear()


@pytest.fixture
def edge_1e4(emulated):
    return C.run_edge(CPU, 1e4)


def test_edge_lengths_meet_the_oracle_per_item(edge_1e4):
    C.check_against_oracle(edge_1e4)


def test_nothing_past_an_item_is_read(edge_1e4):
    C.check_fill_independent(edge_1e4, C.run_edge(CPU, float("nan")))


def test_items_do_not_see_each_other(emulated):
    C.check_items_do_not_see_each_other(CPU)


def test_all_lengths_full_is_the_dense_call(emulated):
    C.check_anchored_to_dense(CPU)


@pytest.mark.parametrize("geom", list(C.GEOMETRIES), ids=lambda g: "fft{}-hop{}-win{}-mels{}".format(*g))
def test_geometry_logmel_meets_the_oracle(emulated, geom):
    """dense and ragged at a geometry that gives the STFT plan another shape; the emulator keeps to a quarter of the
    bound, which is four times what it measured"""
    fft, hop, win, _ = geom
    n = C.geometry_lengths(fft, hop)[0]
    assert C.plan_shape(features._Stft(CPU, 1, n, fft, hop, win)) == C.GEOMETRIES[geom]
    C.check_geometry("mel", geom, C.geometry_mel_errors(geom, CPU), share=0.25, own=False)


@pytest.mark.parametrize("mode", C.PAD_MODES)
@pytest.mark.parametrize("hop", list(C.LOUD_HOPS))
def test_geometry_loudness_meets_the_oracle(emulated, hop, mode):
    n = C.geometry_lengths(C.LOUD_FFT, hop)[0]
    assert C.plan_shape(features._Stft(CPU, 1, n, C.LOUD_FFT, hop, C.LOUD_FFT, mode)) == C.LOUD_HOPS[hop]
    C.check_geometry("loud", (hop, mode), C.geometry_loud_errors(hop, mode, CPU), share=0.25)


def test_geometries_reach_the_plan_branches_they_are_listed_for(emulated):
    """so that a change of features._Stft cannot empty the list without anyone noticing"""
    from tests._rowop_cases import _round_up
    shapes = set(C.GEOMETRIES.values()) | set(C.LOUD_HOPS.values())
    assert {c for c, _, _ in shapes} == {4, 8, 16}
    assert {(c, cw) for c, cw, _ in shapes} == {(4, 4), (8, 8), (16, 32)}      # cw = c: the generic contraction kernel
    assert {g for _, _, g in shapes} >= {1, 2, 4, 8}                             # one group; more than two chained
    assert C.GEOMETRIES[(1024, 256, 1024, 80)] == C.plan_shape(features._Stft(CPU, 1, 2321, 1024, 256, 1024))  # defaults
    assert C.GEOMETRIES[(64, 16, 64, 130)][2] == 1 and 64 // 32 == 2            # a single group of 2 taps
    assert C.GEOMETRIES[(512, 128, 400, 128)][2] == 1 and 512 // 32 == features._lib.SRN_MAX_TAPS
    assert any(m > 128 for _, _, _, m in C.GEOMETRIES) and any(m > 1 + f // 2 for f, _, _, m in C.GEOMETRIES)
    assert any((f - w) % 2 for f, _, w, _ in C.GEOMETRIES)                      # an odd window difference
    assert C.empty_filters((512, 100, 401, 160)) > 0 and C.empty_filters((1024, 256, 1024, 80)) == 0
    for what, (base, bound) in C.GEOM_TOL.items():
        assert abs(bound - _round_up(4 * base)) <= 1e-9 * bound, what
    assert C.GEOM_TOL["mel"][1] <= C.TOL and C.GEOM_TOL["loud"][1] <= C.TOL
    for geom, (base, bound) in C.GEOM_OWN.items():  # derived the same way, from the sum in the contraction's order
        assert f"{C.kernel_order_baseline(geom):.3e}" == f"{base:.3e}" and abs(bound - _round_up(4 * base)) <= 1e-9 * bound
        assert geom in C.GEOMETRIES
    n_ill, where = 0, set()
    for geom in C.GEOMETRIES:
        ns = C.geometry_lengths(geom[0], geom[1])
        for n, seed in ((ns[0], 30), (ns[0], 31), (ns[1], 32), (ns[2], 33)):
            k = int((C.mel_conditioning(C.wave(n, seed), geom) > C.ILL_COND).sum())
            n_ill += k
            where |= {(geom, n)} if k else set()
    assert n_ill == 2 and where == {((512, 100, 401, 160), 911)}  # the own bound covers two elements, no more


def test_without_lengths_the_result_is_a_bare_tensor(emulated):
    x, _ = C.batch([C.wave(1100, 0), C.wave(1100, 1)], 0.0, CPU)
    mel = features.logmelfilterbank(x, C.SR, **C.MEL_KW)
    loud = features.loudness_extract(x, C.SR, C.HOP)
    assert isinstance(mel, torch.Tensor) and mel.shape == (2, 5, C.MELS)
    assert isinstance(loud, torch.Tensor) and loud.shape == (2, 5)
    one = features.logmelfilterbank(x[0], C.SR, **C.MEL_KW)
    assert isinstance(one, torch.Tensor) and one.shape == (5, C.MELS)
    # the plan keys of the dense path are what they were: (what, device, B, n, ...) and nothing appended
    assert all(k[-1] != "ragged" and k[2:4] in ((2, 1100), (1, 1100)) for k in features._PLANS)


def test_length_errors_name_the_item(emulated):
    x, _ = C.batch([C.wave(1300, 0), C.wave(1300, 1)], 0.0, CPU)
    with pytest.raises(ValueError, match=r"item 1 has 256 samples"):  # too short for the reflect pad of 256
        features.logmelfilterbank(x, C.SR, lengths=[1300, 256], **C.MEL_KW)
    with pytest.raises(ValueError, match=r"item 0 has 1024 samples"):  # and for the loudness one of 1024
        features.loudness_extract(x, C.SR, C.HOP, pad_mode="reflect", lengths=[1024, 1300])
    loud, frames = features.loudness_extract(x, C.SR, C.HOP, lengths=[1024, 1])  # zero padding takes any item
    assert frames == [5, 1]
    for fn in (lambda l: features.logmelfilterbank(x, C.SR, lengths=l, **C.MEL_KW),
               lambda l: features.loudness_extract(x, C.SR, C.HOP, lengths=l),
               lambda l: features.loudness_extract(x, C.SR, C.HOP, pad_mode="reflect", lengths=l)):
        for bad in ([1300, 0], [1301, 1300], [1300], torch.tensor([1300, -5])):
            with pytest.raises(ValueError):
                fn(bad)


def test_constant_tables_are_built_once_per_process(emulated, monkeypatch):
    calls = {"_dft_basis": 0, "_slaney_mel": 0, "_a_weight_db": 0}
    for name in calls:
        def counted(*a, _f=getattr(features, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(features, name, counted)
    monkeypatch.setattr(features, "_TABLES", {})
    for n in (1100, 1500):  # two plans of different n per front-end, dense and ragged
        x, lens = C.batch([C.wave(n, 0), C.wave(n - 40, 1)], 0.0, CPU)
        features.logmelfilterbank(x, C.SR, **C.MEL_KW)
        features.logmelfilterbank(x, C.SR, lengths=lens, **C.MEL_KW)
        features.loudness_extract(x, C.SR, C.HOP)
        features.loudness_extract(x, C.SR, C.HOP, lengths=lens)
        features.loudness_extract(x, C.SR, C.HOP, pad_mode="reflect", lengths=lens)
    assert len(features._PLANS) == 10 - 2  # (the LRU holds 8)
    # n_fft 512 and 2048; one filterbank; one curve
    assert calls == {"_dft_basis": 2, "_slaney_mel": 1, "_a_weight_db": 1}
    assert len(features._TABLES) == 4
    bases = {id(p[0].basis) for p in features._PLANS.values()}
    assert len(bases) == 2  # every plan of an n_fft holds the one copy


def test_tables_hold_the_values_of_their_builders(emulated, monkeypatch):
    monkeypatch.setattr(features, "_TABLES", {})
    t = features._mel_table(CPU, C.SR, C.FFT, C.MELS, C.FMIN, C.FMAX)
    want = features._slaney_mel(C.SR, C.FFT, C.MELS, C.FMIN, C.FMAX).T.astype(np.float32)
    assert t.is_contiguous() and np.array_equal(t.numpy(), want)
    assert features._mel_table(CPU, C.SR, C.FFT, C.MELS, C.FMIN, C.FMAX) is t
    assert features._mel_table(CPU, C.SR, C.FFT, C.MELS, C.FMIN, 8000) is not t
