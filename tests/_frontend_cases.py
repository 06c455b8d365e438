"""Case generators and float64 references for the feature front-end's own kernels (serenade_amd/csrc/features.hip:
srn_pad_signal, srn_logmel, srn_loudness and their ragged twins srn_pad_ragged_zero, srn_logmel_ragged,
srn_loudness_ragged) and the GST inference tail (serenade_amd/csrc/gst.hip: srn_gru_recur_last,
srn_style_token_attention_kv).

Shared by tests/test_frontend_cases_host.py (CPU: the C-ABI emulator against these references, the branch each case is
named for, the refusals on the cross-compiled library) and tests/test_zzz_hip_frontend_sweep.py (MI355X: the HIP kernels
against the same references).  No GPU is touched here.  Buf / Out / Case / materialize / check_outputs are
tests/_rowop_cases.py's: every written buffer sits between guard bands, every element the contract leaves alone starts
as the sentinel, and every input element the contract says is not read holds NaN (spec columns [2 n_bins, ld), spec
rows at or past frames[b], x[b][j] for j >= lens[b], the x_bs - n gap between items).  The references are float64
torch / numpy statements of the operation from the same fp32 inputs, written here and not taken from
tests/_emulator.py or tests/test_features_ragged_emulated.py (those are the fp32 baselines they are compared with).

Pass criterion, per element:
  srn_logmel*      |got - ref| * ln(base) <= tol_op    every term of the mel sum is non-negative, so the error of the
                                                       log is the relative error of the sum
  srn_loudness*    |got - ref| <= tol_op               natural log of a mean of non-negative terms
  the three pads   bit for bit
  the GST pair     |got - ref| <= tol_op (|ref| + RMS of the reference row), as srn_gru_train_fwd / srn_token_attn_fwd
(check_outputs measures |g - r| / (|r| + s); the first two pass s = unit - |r|, see _unit.)

tol_op is not chosen: it is 4 x the worst error, under the same formula and over the same sweep, of the fp32 CPU
restatement (the emulator), rounded up to two digits, with a floor of 8 * 2^-24.  `python -m tests._frontend_cases`
prints the measured column again; test_frontend_cases_host.py asserts that the emulator stays within tol_op / 4.

  op                             fp32 baseline   tol_op     remark
  srn_logmel                     6.929e-07       2.8e-06    the rounding of an fp32 log near -10 (log10), -23 (ln), -33 (log2)
  srn_logmel_ragged              7.737e-07       3.1e-06    the same
  srn_loudness                   1.258e-06       5.1e-06    a level of 100 dB has a float32 spacing of 7.6e-6 dB: 8.8e-7 of the amplitude
  srn_loudness_ragged            6.567e-07       2.7e-06    the same
  srn_gru_recur_last             5.034e-07       2.1e-06
  srn_style_token_attention_kv   1.024e-06       4.1e-06
  srn_pad_signal, srn_pad_ragged_zero: bit for bit (reference: numpy.pad)
"""
import math

import numpy as np
import torch

from oracle import features_oracle as FO
from tests import _rowop_cases as R
from tests._rowop_cases import FLOOR, Buf, Case, Out, _Rng, check_outputs, f32, materialize, rms  # noqa: F401

NAN = float("nan")

# op -> (measured fp32 baseline, tol_op); filled from `python -m tests._frontend_cases`
TOL = {
    'srn_logmel': (6.929e-07, 2.8e-06),
    'srn_logmel_ragged': (7.737e-07, 3.1e-06),
    'srn_loudness': (1.258e-06, 5.1e-06),
    'srn_loudness_ragged': (6.567e-07, 2.7e-06),
    'srn_gru_recur_last': (5.034e-07, 2.1e-06),
    'srn_style_token_attention_kv': (1.024e-06, 4.1e-06),
}
EXACT_OPS = ("srn_pad_signal", "srn_pad_ragged_zero")
RAGGED_OPS = ("srn_pad_ragged_zero", "srn_logmel_ragged", "srn_loudness_ragged")  # CPU statements: emul_features


def tol_for(op):
    return 0.0 if op in EXACT_OPS else TOL[op][1]


def _unit(ref, unit):
    """the s of check_outputs' |g - r| <= tol (|r| + s) under which the criterion reads |g - r| <= tol * unit"""
    return unit - ref.abs()


def _none(error):
    """Out.written of a refused call: nothing"""
    return torch.zeros((), dtype=torch.bool) if error else None


# ------------------------------------------------------------------------------------------------ sweep registry
SWEEPS, _LISTS = {}, {}


def sweep(op):
    def deco(fn):
        SWEEPS[op] = fn
        return fn
    return deco


def _list(op):
    if op not in _LISTS:
        lst = list(SWEEPS[op]())
        assert len({c for c, _ in lst}) == len(lst), f"{op}: duplicate case ids"
        _LISTS[op] = dict(lst)
    return _LISTS[op]


def case_ids(op):
    return list(_list(op))


def make(op, cid):
    return _list(op)[cid]()


def all_ids(error=None):
    """[(op, case id)] over every sweep; error True / False: only the cases that must / must not be refused"""
    out = []
    for op in SWEEPS:
        for cid in case_ids(op):
            if error is None or error == cid.startswith("reject-"):
                out.append((op, cid))
    return out


def run_emulated(case, args):
    """the call through the fp32 CPU statements of the C ABI"""
    if case.op in RAGGED_OPS:
        from tests.test_features_ragged_emulated import emul_features
        emul_features(case.op, list(args))
    else:
        from tests import _emulator
        _emulator.emul_call(case.op, list(args))


def refused(case, error, edits):
    """the same call with some arguments replaced ({position: value}): it must fail with `error` and write nothing"""
    for i, v in edits.items():
        case.args[i] = v
    for o in case.outs:
        o.written = _none(True)
    case.error = error
    return case


# ------------------------------------------------------------------------------------------------ srn_logmel
EPS = 1e-10
LN_BASE = {0: 1.0, 2: math.log(2.0), 10: math.log(10.0)}
_LOG64 = {0: torch.log, 2: torch.log2, 10: torch.log10}
LOGMEL_WG = 128  # logmel_kernel's workgroup: the stride of its bin loop and of its mel loop


def _spec(r, rows, nb, ld):
    """(rows, ld): [re | im] of N(0, 1), NaN in the columns [2 nb, ld)"""
    s = torch.full((rows, ld), NAN)
    s[:, :2 * nb] = r.n(rows, 2 * nb)
    return s


def _mel_table(r, nb, nm, empty=None):
    """(nb, nm) non-negative, about half of it zero as a filterbank's is; column `empty` all zero"""
    mel = r.u(nb, nm) * (r.u(nb, nm) < 0.5).float()
    mel[0] += 0.25
    if empty is not None:
        mel[:, empty] = 0.0
    return mel.contiguous()


def _logmel64(spec, mel_t, nb, mode):
    sd = spec.double()
    mag = torch.sqrt(sd[..., :nb] ** 2 + sd[..., nb:2 * nb] ** 2)
    return _LOG64[mode](torch.clamp(mag @ mel_t.double(), min=f32(EPS)))


def _same_in_row(row):
    """extra check: an all-zero spectrum row comes out as one value, log(eps), in every mel column"""
    def fn(g):
        return 0.0 if bool((g[row] == g[row, 0]).all()) else float("inf")
    return fn


LOGMEL_SHAPES = (  # (n_bins, n_mels, ld - 2 n_bins, frames, log_mode, zero row, empty filter)
    (1, 1, 0, 1, 0, None, None), (5, 80, 3, 3, 2, None, 40), (127, 127, 0, 3, 10, None, None),
    (128, 128, 3, 1, 0, None, None), (129, 129, 0, 3, 2, 1, None), (257, 300, 3, 3, 10, 2, 200),
    (257, 1, 0, 1, 10, None, None), (1, 300, 3, 3, 2, None, None), (129, 80, 3, 1, 10, None, None),
    (5, 129, 0, 3, 0, 0, 128), (128, 127, 0, 1, 2, None, None), (127, 128, 3, 3, 0, None, None),
    (8192, 2, 0, 1, 10, None, None))  # the last: the launcher's limit, 32 KiB of LDS


@sweep("srn_logmel")
def _sw_logmel():
    for p in LOGMEL_SHAPES:
        nb, nm, padc, fr, mode, zr, em = p
        cid = f"nb{nb}-nm{nm}-ld{2 * nb + padc}-fr{fr}-log{mode}" + ("" if zr is None else f"-zerorow{zr}") + \
              ("" if em is None else f"-empty{em}")
        yield cid, (lambda p=p: _mk_logmel(*p))
    base = (5, 4, 3, 2, 10, None, None)
    yield "reject-nb8193", lambda: refused(_mk_logmel(8193, 2, 0, 1, 10, None, None), "logmel: bad args", {})
    yield "reject-ld-short", lambda: refused(_mk_logmel(5, 4, 0, 2, 10, None, None), "logmel: bad args", {5: 9})
    yield "reject-log3", lambda: refused(_mk_logmel(*base), "logmel: bad args", {8: 3})
    yield "reject-frames0", lambda: refused(_mk_logmel(*base), "logmel: bad args", {3: 0})


def _mk_logmel(nb, nm, padc, frames, mode, zero_row, empty):
    r = _Rng(f"logmel{nb}-{nm}-{padc}-{frames}-{mode}")
    ld = 2 * nb + padc
    spec, mel = _spec(r, frames, nb, ld), _mel_table(r, nb, nm, empty)
    if zero_row is not None:
        spec[zero_row, :2 * nb] = 0.0
    ref = _logmel64(spec, mel, nb, mode)
    out = Buf(frames * nm)
    o = Out("out", out, ref, _unit(ref, 1.0 / LN_BASE[mode]), extra=None if zero_row is None else _same_in_row(zero_row))
    c = Case("srn_logmel", [spec, mel, out, frames, nb, ld, nm, EPS, mode], [o])
    c.meta = dict(nb=nb, nm=nm, ld=ld, frames=frames, mode=mode, zero_row=zero_row, empty=empty, ref=ref)
    return c


LOGMEL_RAGGED = (  # (B, T, n_bins, n_mels, ld - 2 n_bins, log_mode, frames[b])
    (1, 1, 5, 3, 0, 10, (1,)), (1, 1, 5, 3, 3, 0, (0,)), (1, 1, 129, 130, 0, 2, (6,)),
    (3, 4, 129, 130, 3, 10, (3, 4, 9)), (3, 4, 5, 80, 0, 2, (0, 1, 4)),
    (5, 6, 257, 80, 3, 0, (0, 1, 5, 6, 11)), (5, 6, 127, 129, 0, 10, (11, 6, 0, 5, 1)))


@sweep("srn_logmel_ragged")
def _sw_logmel_ragged():
    for p in LOGMEL_RAGGED:
        B, T, nb, nm, padc, mode, fr = p
        yield f"B{B}-T{T}-nb{nb}-nm{nm}-ld{2 * nb + padc}-log{mode}-frames{'_'.join(map(str, fr))}", \
            (lambda p=p: _mk_logmel_ragged(*p))
    yield "reject-B65536", lambda: refused(_mk_logmel_ragged(1, 1, 5, 3, 0, 10, (1,)), "logmel_ragged: bad args",
                                           {4: 65536})


def _mk_logmel_ragged(B, T, nb, nm, padc, mode, frames):
    r = _Rng(f"logmelr{B}-{T}-{nb}-{nm}-{padc}-{mode}")
    ld = 2 * nb + padc
    spec, mel = _spec(r, B * T, nb, ld).reshape(B, T, ld), _mel_table(r, nb, nm)
    live = torch.arange(T)[None, :] < torch.tensor(frames).clamp(max=T)[:, None]  # (B, T)
    spec[~live] = NAN  # rows at or past frames[b] are not read
    ref = torch.zeros(B, T, nm, dtype=torch.float64)
    ref[live] = _logmel64(spec[live], mel, nb, mode)
    out = Buf(B * T * nm)
    o = Out("out", out, ref, _unit(ref, 1.0 / LN_BASE[mode]), zero=~live[:, :, None])
    c = Case("srn_logmel_ragged", [spec, mel, torch.tensor(frames, dtype=torch.int32), out, B, T, nb, ld, nm, EPS, mode],
             [o])
    c.meta = dict(B=B, T=T, nb=nb, nm=nm, ld=ld, mode=mode, live=[min(f, T) for f in frames])
    return c


def logmel_dense_twin(case, b):
    """the dense srn_logmel call on item b's own rows of a ragged case: (args, position of the output among them)"""
    m = case.meta
    L = m["live"][b]
    out = torch.zeros(L, m["nm"])
    return [case.args[0][b, :L].contiguous(), case.args[1], out, L, m["nb"], m["ld"], m["nm"], EPS, m["mode"]], 2


# ------------------------------------------------------------------------------------------------ srn_loudness
AMIN, TOP_DB, ADD_EPS, SR = 1e-10, 80.0, 1e-5, 24000
POWER_MAX_GRID = 512  # power_max_kernel's block clamp: frames past it take its grid-stride loop
LOUD_WG = 256
KINDS = ("lastmax", "zero", "spike", "tiny", "rand")


def a_weight(nb):
    """the A-weighting of nb bins up to SR / 2; bin 0 (0 Hz) is its -80 dB clamp"""
    return torch.from_numpy(FO.a_weighting(np.linspace(0.0, SR / 2.0, nb))).float()


def _loud_item(r, kind, rows, nb):
    """(rows, 2 nb) [re | im] of one item:
    lastmax  levels uniform in [-70, 0] dB, the loudest bin (40 dB) in the last frame's last bin: floor -40 dB
    zero     exact zeros: every bin at amin, the floor from amin
    spike    one bin at 60 dB, every other at or below -40 dB: all of them at the top_db floor of -20 dB
    tiny     powers within a factor 10 either side of amin
    rand     N(0, 1): everything above both clamps"""
    if kind == "rand":
        return r.n(rows, 2 * nb)
    if kind == "zero":
        return torch.zeros(rows, 2 * nb)
    u, ph = r.u(rows, nb), r.u(rows, nb) * (2 * math.pi)
    if kind == "lastmax":
        amp = 10.0 ** ((-70.0 + 70.0 * u) / 20.0)
        amp[-1, -1] = 100.0
    elif kind == "spike":
        amp = 1e-2 * (0.2 + 0.8 * u)
        amp[rows // 2, nb // 2] = 1e3
    else:
        amp = 1e-5 * 10.0 ** ((-10.0 + 20.0 * u) / 20.0)
    return torch.cat([amp * torch.cos(ph), amp * torch.sin(ph)], dim=-1)


def _loud64(item, aw, nb):
    """item (rows > 0, >= 2 nb) fp32 -> (loudness (rows,), regime shares (above, at amin, at the floor))"""
    sd = item.double()
    p = sd[:, :nb] ** 2 + sd[:, nb:2 * nb] ** 2
    db = 10.0 * torch.log10(torch.clamp(p, min=f32(AMIN)))
    floor = db.max() - f32(TOP_DB)
    amp = torch.pow(10.0, 0.05 * (torch.maximum(db, floor) + aw.double()))
    at_floor = db < floor
    at_amin = (p <= f32(AMIN)) & ~at_floor
    n = float(p.numel())
    shares = (float((~at_floor & ~at_amin).sum()) / n, float(at_amin.sum()) / n, float(at_floor.sum()) / n)
    return torch.log(amp.mean(-1) + f32(ADD_EPS)), shares


def _gmax_ws(B):
    return Buf(B, torch.full((B,), -1, dtype=torch.int32), dtype=torch.int32)  # 0xFFFFFFFF: the launcher zeroes it


LOUD_SHAPES = (  # (B, frames, n_bins, ld - 2 n_bins, rotation of KINDS)
    (1, 1, 1, 0, 0), (3, 2, 63, 3, 0), (1, 513, 255, 0, 0), (3, 600, 256, 1, 2), (3, 2, 257, 0, 1),
    (1, 600, 1025, 3, 2), (3, 513, 1, 3, 0), (1, 2, 256, 3, 1), (3, 1, 1025, 0, 3), (1, 600, 63, 0, 3), (1, 2, 255, 1, 4))


@sweep("srn_loudness")
def _sw_loudness():
    for p in LOUD_SHAPES:
        B, fr, nb, padc, k = p
        kinds = [KINDS[(k + b) % len(KINDS)] for b in range(B)]
        yield f"B{B}-fr{fr}-nb{nb}-ld{2 * nb + padc}-{'_'.join(kinds)}", (lambda p=p: _mk_loudness(*p))
    yield "reject-ld-short", lambda: refused(_mk_loudness(1, 2, 5, 0, 0), "loudness: bad args", {7: 9})
    yield "reject-frames0", lambda: refused(_mk_loudness(1, 2, 5, 0, 0), "loudness: bad args", {5: 0})
    yield "reject-B65536", lambda: refused(_mk_loudness(1, 2, 5, 0, 0), "loudness: B 65536", {4: 65536})


def _mk_loudness(B, frames, nb, padc, k):
    r = _Rng(f"loud{B}-{frames}-{nb}-{padc}-{k}")
    ld = 2 * nb + padc
    kinds = [KINDS[(k + b) % len(KINDS)] for b in range(B)]
    aw = a_weight(nb)
    spec = torch.full((B, frames, ld), NAN)
    ref, shares = torch.zeros(B, frames, dtype=torch.float64), []
    for b, kind in enumerate(kinds):
        spec[b, :, :2 * nb] = _loud_item(r, kind, frames, nb)
        ref[b], sh = _loud64(spec[b], aw, nb)
        shares.append(sh)
    ws, out = _gmax_ws(B), Buf(B * frames)
    c = Case("srn_loudness", [spec, aw, ws, out, B, frames, nb, ld, AMIN, TOP_DB, ADD_EPS],
             [Out("gmax", ws, scratch=True), Out("out", out, ref, _unit(ref, 1.0))])
    c.meta = dict(B=B, frames=frames, nb=nb, ld=ld, kinds=kinds, shares=shares, aw=aw)
    return c


LOUD_RAGGED = (  # (B, T, n_bins, ld - 2 n_bins, frames[b], the quiet item whose dead rows are loud | None)
    (1, 1, 1, 0, (1,), None), (1, 1, 257, 3, (6,), None), (1, 1, 63, 0, (0,), None),
    (3, 5, 63, 3, (1, 5, 10), 0), (3, 5, 1025, 0, (5, 0, 1), 2),
    (4, 600, 255, 0, (0, 1, 600, 605), 1), (4, 600, 256, 3, (600, 605, 1, 0), 2))


@sweep("srn_loudness_ragged")
def _sw_loudness_ragged():
    for p in LOUD_RAGGED:
        B, T, nb, padc, fr, q = p
        yield f"B{B}-T{T}-nb{nb}-ld{2 * nb + padc}-frames{'_'.join(map(str, fr))}-quiet{q}", \
            (lambda p=p: _mk_loudness_ragged(*p))
    ok = (1, 1, 5, 0, (1,), None)
    yield "reject-B65536", lambda: refused(_mk_loudness_ragged(*ok), "loudness_ragged: bad args", {5: 65536})
    yield "reject-ld-short", lambda: refused(_mk_loudness_ragged(*ok), "loudness_ragged: bad args", {8: 9})


def _mk_loudness_ragged(B, T, nb, padc, frames, quiet):
    r = _Rng(f"loudr{B}-{T}-{nb}-{padc}")
    ld = 2 * nb + padc
    aw = a_weight(nb)
    spec = torch.full((B, T, ld), NAN)  # rows at or past frames[b] are not read
    ref = torch.zeros(B, T, dtype=torch.float64)
    live = [min(f, T) for f in frames]
    for b, L in enumerate(live):
        if b == quiet:  # its own rows clip at their own floor; the rows behind them are 80 dB, finite, and not its own
            spec[b, L:, :2 * nb] = 1e4 * r.n(T - L, 2 * nb)
        if L:
            spec[b, :L, :2 * nb] = _loud_item(r, "lastmax" if b == quiet else KINDS[(b + T) % len(KINDS)], L, nb)
            ref[b, :L] = _loud64(spec[b, :L], aw, nb)[0]
    dead = torch.arange(T)[None, :] >= torch.tensor(live)[:, None]
    ws, out = _gmax_ws(B), Buf(B * T)
    c = Case("srn_loudness_ragged",
             [spec, aw, torch.tensor(frames, dtype=torch.int32), ws, out, B, T, nb, ld, AMIN, TOP_DB, ADD_EPS],
             [Out("gmax", ws, scratch=True), Out("out", out, ref, _unit(ref, 1.0), zero=dead)])
    c.meta = dict(B=B, T=T, nb=nb, ld=ld, live=live, quiet=quiet)
    return c


def loudness_dense_twin(case, b):
    """the dense B = 1 srn_loudness call on item b's own rows of a ragged case: (args, position of the output)"""
    m = case.meta
    L = m["live"][b]
    out = torch.zeros(L)
    ws = torch.full((1,), -1, dtype=torch.int32)
    return [case.args[0][b, :L].contiguous(), case.args[1], ws, out, 1, L, m["nb"], m["ld"], AMIN, TOP_DB, ADD_EPS], 3


# ------------------------------------------------------------------------------------------------ the pad kernels
PAD_WG, PAD_GRID = 256, 4096  # the pad kernels' workgroup and block clamp: ld past their product takes the stride loop
PAD_N = (2, 3, 255, 256, 257, 1000)
BIG_LD = PAD_WG * PAD_GRID + 300


def _pad_shapes():
    """(mode, n, pad, ld - (n + 2 pad), B): every n x pad in {0, 1, n - 1}, the reflect limit pad = n - 1 in both modes,
    pad = n + 5 in zero mode, ld and B alternating; one case past the block clamp"""
    k = 0
    for n in PAD_N:
        for pad in sorted({0, 1, n - 1}):
            for mode in ((0, 1) if pad == n - 1 else ((k % 2),)):
                yield mode, n, pad, (0, 37)[k % 2], (1, 3)[(k // 2) % 2]
                k += 1
        yield 1, n, n + 5, (37, 0)[k % 2], (3, 1)[(k // 2) % 2]
        k += 1
    yield 0, 1_000_000, 24_000, BIG_LD - 1_048_000, 1


@sweep("srn_pad_signal")
def _sw_pad_signal():
    for p in _pad_shapes():
        yield "mode{}-n{}-pad{}-tail{}-B{}".format(*p), (lambda p=p: _mk_pad_signal(*p))
    yield "reject-reflect-pad-n", lambda: refused(_mk_pad_signal(0, 5, 4, 2, 1), "reflect padding of 5", {4: 5})
    yield "reject-n1", lambda: refused(_mk_pad_signal(1, 2, 1, 3, 1), "pad_signal: bad args", {3: 1})
    yield "reject-ld-short", lambda: refused(_mk_pad_signal(1, 5, 2, 0, 1), "pad_signal: bad args", {5: 8})
    yield "reject-B65536", lambda: refused(_mk_pad_signal(1, 5, 2, 0, 1), "pad_signal: B 65536", {2: 65536})


def _mk_pad_signal(mode, n, pad, tail, B):
    r = _Rng(f"pad{mode}-{n}-{pad}-{tail}-{B}")
    ld = n + 2 * pad + tail
    x = r.n(B, n)
    ref = np.zeros((B, ld), dtype=np.float32)
    ref[:, :n + 2 * pad] = np.pad(x.numpy(), ((0, 0), (pad, pad)), mode="constant" if mode else "reflect")
    out = Buf(B * ld)
    z = (torch.arange(ld) >= n + 2 * pad)[None, :]
    return Case("srn_pad_signal", [x, out, B, n, pad, ld, mode], [Out("out", out, torch.from_numpy(ref), zero=z, exact=True)])


RAGGED_LENS = lambda n: (0, 1, n, n + 7)  # noqa: E731  the last is clamped to n


@sweep("srn_pad_ragged_zero")
def _sw_pad_ragged_zero():
    k = 0
    for n in PAD_N:
        for pad in sorted({0, 1, n - 1}) + [n + 5]:
            p = (n, pad, (0, 37)[k % 2], (0, 9)[(k // 2) % 2], (4, 1)[(k // 4) % 2], k)
            yield "n{}-pad{}-tail{}-gap{}-B{}-rot{}".format(*p), (lambda p=p: _mk_pad_ragged_zero(*p))
            k += 1
    big = (1_000_000, 24_000, BIG_LD - 1_048_000, 9, 1, 2)
    yield "n{}-pad{}-tail{}-gap{}-B{}-rot{}".format(*big), (lambda: _mk_pad_ragged_zero(*big))
    ok = (5, 2, 0, 9, 1, 2)
    yield "reject-x_bs-short", lambda: refused(_mk_pad_ragged_zero(*ok), "pad_ragged_zero: bad sizes", {1: 4})
    yield "reject-ld-short", lambda: refused(_mk_pad_ragged_zero(*ok), "pad_ragged_zero: bad sizes", {7: 8})
    yield "reject-B65536", lambda: refused(_mk_pad_ragged_zero(*ok), "pad_ragged_zero: bad sizes", {4: 65536})


def _mk_pad_ragged_zero(n, pad, tail, gap, B, rot):
    r = _Rng(f"padr{n}-{pad}-{tail}-{gap}-{B}")
    ld, x_bs = n + 2 * pad + tail, n + gap
    lens = [RAGGED_LENS(n)[(rot + b) % 4] for b in range(B)]
    x = torch.full((B, x_bs), NAN)  # past an item's length and between items: not read
    ref = np.zeros((B, ld), dtype=np.float32)
    for b, ln in enumerate(lens):
        L = min(ln, n)
        x[b, :L] = r.n(L)
        ref[b] = np.pad(x[b, :L].numpy(), (pad, ld - pad - L), mode="constant")
    out = Buf(B * ld)
    c = Case("srn_pad_ragged_zero", [x, x_bs, torch.tensor(lens, dtype=torch.int32), out, B, n, pad, ld],
             [Out("out", out, torch.from_numpy(ref), exact=True)])
    c.meta = dict(lens=lens)
    return c


# ------------------------------------------------------------------------------------------------ the GST tail
GRU_H = (1, 4, 21, 22, 128, 341)  # 3 H = 63 | 66 straddle one wave; 3 H = 1023: the limit
GRU_SHAPES = ((1, 1, 1), (3, 2, 4), (1, 64, 21), (3, 1, 22), (1, 2, 128), (3, 64, 341), (3, 64, 4), (1, 1, 341),
              (3, 2, 21), (1, 64, 22))  # (B, T, H)


@sweep("srn_gru_recur_last")
def _sw_gru():
    for a in GRU_SHAPES:
        yield "B{}-T{}-H{}".format(*a), (lambda a=a: _mk_gru(*a))
    yield "reject-H342", lambda: _mk_gru(1, 2, 342, error="gru_recur_last: bad args")


def _mk_gru(B, T, H, error=None):
    _, gi, w_hh, b_hh = R._gru_inputs(B, T, H)
    with torch.no_grad():
        last = R._gru_forward64(gi.double(), w_hh.double(), b_hh.double())[0][:, -1]
        if not error:
            assert float((last - R._nn_gru64(gi.double(), w_hh.double(), b_hh.double())[:, -1]).abs().max()) < 1e-12
    h = Buf(B * H)
    c = Case("srn_gru_recur_last", [gi, w_hh.t().contiguous(), b_hh, h, B, T, H],
             [Out("h", h, last, rms(last, -1), written=_none(error))], error=error)
    c.meta = dict(B=B, T=T, H=H)
    return c


ATTN_WG = 256      # style_token_attention_kv_kernel's workgroup: one thread per head in the softmax
ATTN_LDS = 65536
ATTN_SHAPES = (  # (B, Dq, n_tok, F, n_head)
    (1, 1, 1, 4, 1), (3, 128, 10, 256, 4), (1, 257, 50, 260, 4), (3, 300, 257, 4, 4), (1, 128, 257, 256, 1),
    (3, 257, 10, 260, 4), (1, 300, 50, 256, 256), (3, 1, 1, 260, 1))
ATTN_LDS_LIMIT = (2, 272, 3900, 256, 4)  # (2 F + n_head n_tok + Dq) * 4 = 64 KiB exactly


def attn_lds_bytes(Dq, n_tok, Fd, nh):
    return (2 * Fd + nh * n_tok + Dq) * 4


@sweep("srn_style_token_attention_kv")
def _sw_attn():
    for a in ATTN_SHAPES:
        yield "B{}-Dq{}-tok{}-F{}-h{}".format(*a), (lambda a=a: _mk_attn(*a))
    yield "lds-limit-B{}-Dq{}-tok{}-F{}-h{}".format(*ATTN_LDS_LIMIT), lambda: _mk_attn(*ATTN_LDS_LIMIT)
    B, Dq, tok, Fd, nh = ATTN_LDS_LIMIT
    yield "reject-lds", lambda: _mk_attn(B, Dq + 1, tok, Fd, nh, error="too large for LDS")
    yield "reject-h258-F516", lambda: _mk_attn(1, 8, 2, 516, 258, error="n_head 258 is above the limit of 256")
    yield "reject-F6-h4", lambda: _mk_attn(1, 8, 2, 6, 4, error="style_token_attention_kv: bad sizes")


def _mk_attn(B, Dq, n_tok, Fd, nh, error=None):
    r = _Rng(f"stkv{B}-{Dq}-{n_tok}-{Fd}-{nh}")
    ref_in = r.n(B, Dq)
    wq_t, bq = r.n(Dq, Fd) / math.sqrt(Dq), 0.1 * r.n(Fd)
    k, v = r.n(n_tok, Fd), r.n(n_tok, Fd)
    wo_t, bo = r.n(Fd, Fd) / math.sqrt(Fd), 0.1 * r.n(Fd)
    if Fd % nh == 0:
        q = ref_in.double() @ wq_t.double() + bq.double()
        ctx = R._attn64(q, k.double(), v.double(), nh)[1]
        ref = ctx @ wo_t.double() + bo.double()
    else:
        ref = torch.zeros(B, Fd, dtype=torch.float64)
    out = Buf(B * Fd)
    c = Case("srn_style_token_attention_kv", [ref_in, wq_t, bq, k, v, wo_t, bo, out, B, Dq, n_tok, Fd, nh],
             [Out("out", out, ref, rms(ref, -1), written=_none(error))], error=error)
    c.meta = dict(B=B, Dq=Dq, n_tok=n_tok, F=Fd, nh=nh)
    return c


# ------------------------------------------------------------------------------------------------ measuring the table
def baseline_error(op, cid):
    case = make(op, cid)
    args, bufs = materialize(case)
    run_emulated(case, args)
    return check_outputs(case, bufs)[0]


def _main():
    import sys
    for op in sys.argv[1:] or list(SWEEPS):
        if op in EXACT_OPS:
            continue
        worst = max(baseline_error(op, cid) for cid in case_ids(op) if not cid.startswith("reject-"))
        print(f"    {op!r}: ({worst:.3e}, {R._round_up(max(4 * worst, FLOOR)):.1e}),", flush=True)


if __name__ == "__main__":
    _main()
