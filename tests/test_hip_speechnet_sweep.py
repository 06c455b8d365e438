"""The transcriber's and ContentVec's own kernels (serenade_amd/csrc/transcriber.hip, contentvec.hip) on the MI355X
against float64 at edge shapes: srn_mel_db with negative maxima, idle lanes, two loop trips and dirty scratch; srn_trans_conv0
and srn_trans_pool down to 1 x 1 x 1 and past their grids; srn_bilstm_recur with idle threads, empty k-slices, strides
of its own, saturated gates and items of length 1 and 0; srn_cvec_conv0 + srn_channel_norm_gelu at the limits of k and
stride, in place, and past the norm's grid; srn_posconv_gelu_res at the LDS limit, without lengths, with odd K and with
whole tiles past an item; and every refusal of the seven entries.

The cases, references and bounds are tests/_speechnet_cases.py's; tests/test_speechnet_cases_host.py shows on the CPU
that plain float32 statements of the entries meet the bounds with room, so that the bounds here judge the kernels."""
import ctypes

import pytest
import torch

from serenade_amd import _lib, ops
from tests import _speechnet_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(name, args):
    """one entry point in place on CPU tensors: every tensor's whole buffer goes up (once: views of one buffer stay
    views of one buffer, so guards and aliases are the device's too), the call runs, every buffer comes back"""
    bufs = {}

    def dev(t):
        base = t if t._base is None else t._base
        assert base.is_contiguous() and t.is_contiguous()
        if id(base) not in bufs:
            bufs[id(base)] = (base, base.to(DEV))
        return bufs[id(base)][1].view(-1)[t.storage_offset():t.storage_offset() + t.numel()]

    ops.CallOp(name, [dev(a) if isinstance(a, torch.Tensor) else a for a in args])()
    torch.cuda.synchronize()
    for base, d in bufs.values():
        base.copy_(d)


def _hold(case, res):
    for what, (err, bound) in res.items():
        print(f"{case} {what}: {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (case, what, err, bound)


@pytest.mark.parametrize("case", C.MEL_CASES, ids=repr)
def test_mel_db(case):
    _hold(case, C.check_mel(case, run))


@pytest.mark.parametrize("case", C.CONV0_CASES, ids=repr)
def test_trans_conv0(case):
    _hold(case, C.check_conv0(case, run))


@pytest.mark.parametrize("case", C.POOL_CASES, ids=repr)
def test_trans_pool(case):
    _hold(case, C.check_pool(case, run))


@pytest.mark.parametrize("case", C.LSTM_CASES, ids=repr)
def test_bilstm_recur(case):
    _hold(case, C.check_lstm(case, run))


@pytest.mark.parametrize("case", C.CVEC_CASES, ids=repr)
def test_cvec_conv0_and_channel_norm(case):
    _hold(case, C.check_cvec(case, run))


@pytest.mark.parametrize("case", C.POS_CASES, ids=repr)
def test_posconv_gelu_res(case):
    _hold(case, C.check_pos(case, run))


def test_bad_arguments_are_refused_before_any_launch():
    """every null pointer and every size rule the SRN_CHECK_ARGs of the seven entries state, one violation per call
    from a base call that is valid: non-zero return, the entry's name in srn_last_error, nothing launched.  Before
    each call another entry (srn_pad_ragged) is refused, so a message left by the previous call cannot pass for this
    one's."""
    h = _lib.lib()
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    zeros = torch.zeros(4096, device=DEV)
    dbl = torch.zeros(64, device=DEV, dtype=torch.float64)
    ones = torch.ones(4, device=DEV, dtype=torch.int32)
    out = torch.full((4096,), 7.0, device=DEV)
    f, f1, d, i, o, o1 = ptr(zeros), ptr(zeros, 4), ptr(dbl), ptr(ones), ptr(out), ptr(out, 4)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # name: (argument names, a valid call, [{argument: bad value}])
    cases = {
        "srn_mel_db": (
            "spec ld_spec n_bins mel_t lens gmax out ld_out B T n_mels amin top_db",
            (f, 8, 3, f, i, i, o, 4, 2, 2, 4, 1e-10, 80.0),
            [dict(spec=None), dict(mel_t=None), dict(lens=None), dict(gmax=None), dict(out=None), dict(B=0), dict(T=0),
             dict(n_bins=0), dict(n_bins=8193, ld_spec=16386), dict(ld_spec=5), dict(n_mels=0), dict(ld_out=3),
             dict(amin=0.0), dict(top_db=-1.0)]),
        "srn_trans_conv0": (
            "x x_bs ld_x lens w bias out B T F C dilation",
            (f, 16, 4, i, f, f, o, 2, 4, 3, 4, 1),
            [dict(x=None), dict(lens=None), dict(w=None), dict(bias=None), dict(out=None), dict(B=0), dict(T=0),
             dict(F=0), dict(C=0), dict(ld_x=2), dict(x_bs=15), dict(dilation=3), dict(dilation=0)]),
        "srn_trans_pool": (
            "in_ lens out B T F_in C C_valid flatten ld_out",
            (f, i, o, 2, 4, 4, 4, 4, 0, 0),
            [dict(in_=None), dict(lens=None), dict(out=None), dict(in_=o), dict(B=0), dict(T=0), dict(F_in=1),
             dict(C=0), dict(C_valid=0), dict(C_valid=5), dict(flatten=2, ld_out=8), dict(flatten=1, ld_out=7)]),
        "srn_bilstm_recur": (
            "g g_bs ld_g lens w_hh_t out out_bs ld_out B T H",
            (f, 512, 256, i, f, o, 128, 64, 1, 2, 32),
            [dict(g=None), dict(lens=None), dict(w_hh_t=None), dict(out=None), dict(H=24, ld_out=48),
             dict(H=36, g_bs=576, ld_g=288, out_bs=144, ld_out=72), dict(H=520, g_bs=8320, ld_g=4160, out_bs=2080, ld_out=1040),
             dict(w_hh_t=f1), dict(ld_g=248), dict(g_bs=511), dict(ld_out=63), dict(out_bs=127), dict(B=0), dict(T=0)]),
        "srn_cvec_conv0": (
            "wave wave_bs n lens w out partials B T0 C k stride",
            (f, 64, 64, i, f, o, d, 2, 4, 8, 10, 5),
            [dict(wave=None), dict(lens=None), dict(w=None), dict(out=None), dict(partials=None), dict(B=0), dict(T0=0),
             dict(C=0), dict(n=0), dict(k=0), dict(k=17), dict(stride=0), dict(stride=65), dict(wave_bs=63)]),
        "srn_channel_norm_gelu": (
            "x partials n_chunks lens gamma beta stats y B T C eps",
            (f, d, 1, i, f, f, f, o, 2, 4, 8, 1e-5),
            [dict(x=None), dict(partials=None), dict(lens=None), dict(gamma=None), dict(beta=None), dict(stats=None),
             dict(y=None), dict(B=0), dict(T=0, n_chunks=0), dict(C=0), dict(C=6), dict(n_chunks=2), dict(x=f1),
             dict(gamma=f1), dict(beta=f1), dict(stats=f1), dict(y=o1)]),
        "srn_posconv_gelu_res": (
            "x lens w bias y B T C groups k pad",
            (f, i, f, f, o, 1, 4, 16, 4, 3, 1),
            [dict(x=None), dict(w=None), dict(bias=None), dict(y=None), dict(x=o), dict(B=0), dict(T=0), dict(groups=0),
             dict(C=18), dict(C=24), dict(C=272), dict(k=0, pad=0), dict(k=129, pad=64), dict(pad=3), dict(pad=-1)]),
    }
    n_calls = 0
    for name, (names, base, bads) in cases.items():
        names = names.split()
        assert len(names) == len(base)
        for bad in bads:
            assert set(bad) <= set(names), (name, bad)
            args = [bad.get(k, v) for k, v in zip(names, base)] + [st]
            assert h.srn_pad_ragged(None, 8, i, o, 2, 8, 2, 16, st) != 0 and b"pad_ragged" in h.srn_last_error()
            assert getattr(h, name)(*args) != 0, (name, bad)
            assert name[4:].encode() in h.srn_last_error(), (name, bad, h.srn_last_error())
            n_calls += 1
    assert n_calls == 99
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched: the output is untouched
