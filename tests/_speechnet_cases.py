"""TEST-ONLY: the edge cases of the transcriber's and ContentVec's own kernels (serenade_amd/csrc/transcriber.hip and
contentvec.hip: srn_mel_db, srn_trans_conv0, srn_trans_pool, srn_bilstm_recur, srn_cvec_conv0, srn_channel_norm_gelu,
srn_posconv_gelu_res), shared by the CPU test that shows the cases fit to judge a kernel
(tests/test_speechnet_cases_host.py) and the run on the GPU (tests/test_hip_speechnet_sweep.py): same inputs, same
float64 references, same bounds.

Every `check_*` takes a case and `run(name, args)`, which executes one entry point in place on CPU tensors: the host
test hands in the plain float32 CPU statements of the entries, the GPU test uploads, launches and copies back.  A check
asserts everything that is exact (zero padding, NaN guards, bit-for-bit results) and returns {label: (error, bound)};
the GPU test holds error <= bound, the host test a tenth of it (beyond one float32 spacing), so that summation order
cannot read as error.

References are float64 restatements of each entry's contract (include/serenade_hip.h), computed from the
float32-rounded inputs on the unpadded item x[b, :len_b].  Bounds are relative to max|ref| of the item:
  srn_trans_pool                bit for bit (data movement and max)
  srn_trans_conv0               1e-6   (tests/test_hip_transcriber.py's bound)
  srn_cvec_conv0 outputs        1e-6   (tests/test_hip_contentvec.py's bound)
  srn_cvec_conv0 partials       1e-12 of the item's largest sum (or sum of squares): the reference is the fp64 sum of the
                                kernel's OWN fp32 outputs, <= 64 terms, so the two differ by at most 64 * 2^-53 sum|v|,
                                and the largest of C sums is never a thousandth of sum|v|
  srn_channel_norm_gelu         2e-5   (the existing bound) against fp64 GroupNorm + GELU of the kernel's own conv output
  srn_posconv_gelu_res          1e-5   (the existing bound)
  srn_bilstm_recur              2e-5   (the existing bound)
  srn_mel_db                    absolute, 4.343 (n_bins + 4) 2^-24 + 3e-5 dB: all terms are non-negative, so the fp32
                                fma chain is within (n_bins + 3) 2^-24 relative; 10 log10 turns relative e into 4.343 e;
                                3e-5 covers log10f and the final product at |dB| <= 100
Buffers are NaN outside what an entry may write (leading-dimension columns, offsets, GUARD elements on either side) and
must still be NaN afterwards; inputs are NaN wherever the contract says they are not read.

Not here: srn_pad_ragged is swept by the ragged feature tests (tests/test_hip_features_ragged.py and
tests/_features_ragged_cases.py) and is not repeated.  Both of its callers refuse an item no longer than the pad, so
L <= pad stays out of scope (there the kernel clamps where numpy's reflect would reflect twice).  With lengths
[50, 41, 0] a batch of three of srn_mel_db has no room for an all-zero item, so that item comes with the second call
on the same buffers (lengths [41, 0, 50]).  The H of srn_bilstm_recur must be a multiple of 8 in [32, 512]; the
channels per group of srn_posconv_gelu_res a multiple of 4 up to 64: what lies outside is a refusal (the GPU test's
last test).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from serenade_amd.contentvec import ContentVec
from serenade_amd.transcriber import lstm_w_hh_t

NAN = float("nan")
GUARD = 8  # elements of NaN before and after every output buffer (a multiple of 4: 16-byte alignment survives)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(n, dtype=torch.float32, fill=NAN):
    """(whole buffer, the n elements an entry may write), GUARD elements of `fill` on either side"""
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype)
    return full, full[GUARD:GUARD + n]


def guards_intact(full):
    return bool(torch.isnan(full[:GUARD]).all() and torch.isnan(full[-GUARD:]).all())


def bits_equal(a, b):
    """bit for bit, NaN included"""
    a, b = a.contiguous(), b.contiguous()
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and bool((a.view(it) == b.view(it)).all())


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32)


def abs_err(got, ref):
    """max |got - ref| over EVERY element.  A NaN or an infinity on either side is a failure here and now: it would
    vanish in a running maximum (max(0.0, nan) is 0.0), and it is what padding that reached a valid row, or a valid
    element left unwritten in a NaN-filled buffer, looks like"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(ref).all()), "the reference is not finite"
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{int(bad.sum())} of {got.numel()} compared elements are NaN or infinite"
    return (got - ref).abs().max().item() if ref.numel() else 0.0


def rel_err(got, ref):
    """abs_err / max |ref| (the error itself where the reference is all zero)"""
    err = abs_err(got, ref)
    scale = ref.double().abs().max().item() if ref.numel() else 0.0
    return err / scale if scale > 0 else err


def worse(*v):
    """the running maximum of error figures; never silently past a NaN"""
    assert all(x == x for x in v), v
    return max(v)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


# ------------------------------------------------------------------------------------------------ A. srn_mel_db
MEL_SHAPES = ((1, 4), (65, 16), (257, 70), (513, 300))  # n_mels < 64: idle lanes in wave_max; > 256: two loop trips
MEL_CASES = tuple((nb, nm, T) for nb, nm in MEL_SHAPES for T in (50, 1))
AMIN = float(np.float32(1e-10))  # as it arrives behind the C ABI's float
TOP_DB = 80.0
AMIN_DB = (10.0 * torch.log10(torch.tensor(AMIN, dtype=torch.float64))).item()  # -100 dB, as the reference forms it
MEL_OLD_BOUND = 1e-3  # tests/test_hip_transcriber.py's; the derived bound may never exceed it


def mel_bound(nb):
    b = 4.343 * (nb + 4) * 2.0 ** -24 + 3e-5
    assert b <= MEL_OLD_BOUND
    return b


@functools.lru_cache(maxsize=None)
def mel_inputs(nb, nm, T):
    """two calls for the same buffers.  A: a loud item (positive maximum), one scaled by 1e-3 (negative maximum, its
    quiet frames at amin), one of length 0.  B: an all-zero item (everything -100 dB, nothing clamped upward), one of
    length 0, another loud one.  Frame gains fall over six decades; rows past a length and the columns past 2 n_bins
    are NaN."""
    g = _gen(1000 + nb)
    mel = torch.rand(nb, nm, generator=g)
    gains = torch.logspace(0, -6, T, dtype=torch.float64)[:, None]
    draw = lambda: (torch.randn(T, 2 * nb, generator=g, dtype=torch.float64) * gains).float()
    short = min(41, T)
    calls = ((("loud", draw()), ("quiet", (draw().double() * 1e-3).float()), ("none", None)), [T, short, 0]), \
            ((("zero", torch.zeros(T, 2 * nb)), ("none", None), ("loud", draw())), [short, 0, T])
    return mel, calls


def _mel_db64(spec, mel):
    s = spec.double()
    nb = mel.shape[0]
    return 10.0 * torch.log10(torch.clamp((s[:, :nb] ** 2 + s[:, nb:] ** 2) @ mel.double(), min=AMIN))


def mel_ref(nb, nm, T, call):
    """[(dB before the top_db clamp, reference) or None per item] of call 0 / 1"""
    mel, calls = mel_inputs(nb, nm, T)
    items, lens = calls[call]
    out = []
    for (kind, s), L in zip(items, lens):
        if L == 0:
            out.append(None)
            continue
        db = _mel_db64(s[:L], mel)
        out.append((db, torch.max(db, db.max() - TOP_DB)))
    return out


def mel_regimes(nb, nm, T):
    """shares of the valid elements (the all-zero item aside) above both clamps, at amin, at the top_db floor; and
    whether any such item is clamped in every element"""
    n = above = at_amin = at_floor = 0
    all_clamped = False
    for call in (0, 1):
        for (kind, _), r in zip(mel_inputs(nb, nm, T)[1][call][0], mel_ref(nb, nm, T, call)):
            if r is None or kind == "zero":
                continue
            db, ref = r
            fl = db < db.max() - TOP_DB
            am = (db == AMIN_DB) & ~fl
            n += db.numel()
            at_floor += int(fl.sum())
            at_amin += int(am.sum())
            above += int((~fl & ~am).sum())
            all_clamped |= bool((fl | am).all())
    return above / n, at_amin / n, at_floor / n, all_clamped


def check_mel(case, run):
    nb, nm, T = case
    mel, calls = mel_inputs(nb, nm, T)
    B, ld_spec, ld_out = 3, 2 * nb + 3, nm + 5

    def fill(spec, lens_t, call):
        items, lens = calls[call]
        sv = spec.view(B, T, ld_spec)
        sv.fill_(NAN)
        for b, ((_, s), L) in enumerate(zip(items, lens)):
            if L:
                sv[b, :L, :2 * nb] = s[:L]
        lens_t.copy_(i32(lens))

    def launch(spec, lens_t, gmax, out):
        run("srn_mel_db", (spec, ld_spec, nb, mel, lens_t, gmax, out, ld_out, B, T, nm, AMIN, TOP_DB))

    spec, lens_t = torch.empty(B * T * ld_spec), torch.zeros(B, dtype=torch.int32)
    full, out = guarded(B * T * ld_out)
    gmax = torch.full((B,), -1, dtype=torch.int32)  # 0xFFFFFFFF: a replayed plan leaves the last maximum there
    worst = 0.0
    for call in (0, 1):  # the second call finds the first one's maxima and results in its buffers
        fill(spec, lens_t, call)
        launch(spec, lens_t, gmax, out)
        o = out.view(B, T, ld_out)
        assert guards_intact(full) and bool(torch.isnan(o[..., nm:]).all()), (case, call)
        refs = mel_ref(nb, nm, T, call)
        for b, (r, L) in enumerate(zip(refs, calls[call][1])):
            assert bool((o[b, L:, :nm] == 0).all()), (case, call, b)
            if r is not None:
                worst = worse(worst, abs_err(o[b, :L, :nm], r[1]))
        if call == 0 and T > 1:  # a batch-wide clamp would floor the quiet item 60 dB higher: told apart here
            batch_max = max(r[0].max() for r in refs if r is not None)
            db, ref = refs[1]
            wrong = torch.max(db, batch_max - TOP_DB)
            assert (wrong - ref).abs().max().item() > 10.0
            assert (o[1, :calls[0][1][1], :nm].double() - wrong).abs().max().item() > 10.0
        if call == 1:
            assert refs[0][1].max().item() == AMIN_DB == refs[0][1].min().item()  # all -100 dB
    f2, fresh = guarded(B * T * ld_out)
    launch(spec, lens_t, torch.zeros(B, dtype=torch.int32), fresh)
    assert bits_equal(full, f2), (case, "the call on dirty buffers differs from a fresh one")
    return {"dB": (worst, mel_bound(nb))}


# ------------------------------------------------------------------------------------------------ B. srn_trans_conv0
CONV0_CASES = tuple((dil, T, Fq, C) for dil in (1, 2) for T, Fq, C in ((1, 1, 1), (2, 3, 4), (97, 39, 12), (70, 126, 128)))
CONV0_GRID = 4096 * 256  # the launch's thread cap per item: (70, 126, 128) has 1.15 M outputs


def conv0_lens(T):
    return [T, 1, 0]


@functools.lru_cache(maxsize=None)
def conv0_inputs(dil, T, Fq, C):
    g = _gen(2014 + 10 * T + dil)  # a seed at which ReLU leaves every item of (1, 1, 1) something to compare
    ld_x, lens = Fq + 3, conv0_lens(T)
    x_bs = T * ld_x + 7
    x = torch.full((3, x_bs), NAN)
    for b, L in enumerate(lens):
        x[b, :T * ld_x].view(T, ld_x)[:L, :Fq] = torch.randn(L, Fq, generator=g)
    return x, torch.randn(C, 9, generator=g), torch.randn(C, generator=g) + 0.5


@functools.lru_cache(maxsize=None)
def conv0_ref(dil, T, Fq, C):
    x, w, bias = conv0_inputs(dil, T, Fq, C)
    refs = []
    for b, L in enumerate(conv0_lens(T)):
        xi = x[b, :T * (Fq + 3)].view(T, Fq + 3)[:L, :Fq].double()[None, None]
        refs.append(F.relu(F.conv2d(xi, w.double().view(C, 1, 3, 3), bias.double(), padding=(dil, 1),
                                    dilation=(dil, 1)))[0].permute(1, 2, 0) if L else None)  # (L, F, C)
    return refs


def check_conv0(case, run):
    dil, T, Fq, C = case
    x, w, bias = conv0_inputs(*case)
    lens = conv0_lens(T)
    full, out = guarded(3 * T * (Fq + 2) * C)
    run("srn_trans_conv0", (x, x.shape[1], Fq + 3, i32(lens), w, bias, out, 3, T, Fq, C, dil))
    o = out.view(3, T, Fq + 2, C)
    assert guards_intact(full), case
    worst = 0.0
    for b, (L, ref) in enumerate(zip(lens, conv0_ref(*case))):
        assert bool((o[b, :, 0] == 0).all() and (o[b, :, Fq + 1] == 0).all() and (o[b, L:] == 0).all()), (case, b)
        if L:
            worst = worse(worst, rel_err(o[b, :L, 1:Fq + 1], ref))
    return {"conv0": (worst, 1e-6)}


# ------------------------------------------------------------------------------------------------ C. srn_trans_pool
POOL_T, POOL_LENS = 67, [67, 40, 0]
POOL_CASES = tuple((0, Fin, C, C, 0) for Fin in (2, 3, 39, 126) for C in (4, 12)) \
    + tuple((1, Fin, C, Cv, extra) for Fin in (2, 3, 39, 126) for C, Cv in ((4, 3), (12, 12), (128, 100)) for extra in (0, 8)) \
    + ((0, 126, 256, 256, 0),)  # 67 * 65 * 256 = 1 114 880 outputs per item: the grid-stride loop
POOL_GRID = 4096 * 256


def pool_width(flatten, Fin, C, Cv, extra):
    """output floats per frame"""
    Fo = Fin // 2
    return (Cv * Fo + 3) // 4 * 4 + extra if flatten else (Fo + 2) * C


@functools.lru_cache(maxsize=None)
def pool_inputs(Fin, C):
    """signed values with a negative mean (a maximum seeded with 0 is wrong on most elements); NaN in both border
    columns, in the last column of an odd F_in (MaxPool drops it) and in the rows past each length"""
    x = torch.randn(3, POOL_T, Fin + 2, C, generator=_gen(3000 + Fin + C)) - 1.0
    x[:, :, 0] = NAN
    x[:, :, Fin + 1] = NAN
    if Fin % 2:
        x[:, :, Fin] = NAN
    for b, L in enumerate(POOL_LENS):
        x[b, L:] = NAN
    return x


def pool_ref(flatten, Fin, C, Cv, extra):
    x, Fo = pool_inputs(Fin, C), Fin // 2
    p = torch.maximum(x[:, :, 1:2 * Fo + 1:2], x[:, :, 2:2 * Fo + 2:2])  # (B, T, Fo, C)
    if flatten:
        ref = torch.zeros(3, POOL_T, pool_width(flatten, Fin, C, Cv, extra))
        ref[:, :, :Cv * Fo] = p[..., :Cv].permute(0, 1, 3, 2).reshape(3, POOL_T, Cv * Fo)
    else:
        ref = torch.zeros(3, POOL_T, Fo + 2, C)
        ref[:, :, 1:Fo + 1] = p
    for b, L in enumerate(POOL_LENS):
        ref[b, L:] = 0
    return ref


def check_pool(case, run):
    flatten, Fin, C, Cv, extra = case
    ref = pool_ref(*case)
    full, out = guarded(ref.numel())
    run("srn_trans_pool", (pool_inputs(Fin, C), i32(POOL_LENS), out, 3, POOL_T, Fin, C, Cv, flatten,
                           pool_width(*case) if flatten else 0))
    assert guards_intact(full), case
    got = out.view(ref.shape)
    wrong = int((got.view(torch.int32) != ref.view(torch.int32)).sum())
    assert wrong == 0, (case, wrong, "elements differ from the reference's bits")
    return {"pool": (0.0, 0.0)}


# ------------------------------------------------------------------------------------------------ D. srn_bilstm_recur
LSTM_H = (48, 72, 200, 344)
LSTM_T, LSTM_LENS = 67, [67, 40, 1, 0, 67]  # the last item is the first with gate columns pinned at +-200
LSTM_CASES = tuple((H, drive) for H in LSTM_H for drive in (1, 8))


def lstm_slices(H, KS):
    """the kernel's slice rule: (live threads, launched threads, k-slices that own no k)"""
    kc = (H + KS - 1) // KS
    empty = sum(1 for s in range(KS) if min(s * kc, H) == H)
    return KS * H, (KS * H + 63) // 64 * 64, empty


@functools.lru_cache(maxsize=None)
def lstm_inputs(H, drive):
    """weights and inputs as tests/test_hip_transcriber.py's recurrence test draws them (everything 1 / sqrt(H)), the
    projection times `drive`; g is NaN past each length, in the columns past 8 H and between the items"""
    g = _gen(4000 + H)
    T, I, B = LSTM_T, 24, len(LSTM_LENS)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) / math.sqrt(H)
    w_ih, w_hh, bias = rn(8 * H, I).float(), rn(2, 4 * H, H).float(), (rn(8 * H) + rn(8 * H)).float()
    x = torch.randn(B - 1, T, I, generator=g, dtype=torch.float64)
    gin = ((x @ w_ih.double().T + bias.double()) * drive).float()
    pinned = gin[0].clone()
    col = torch.arange(8 * H)
    pinned[:, col % 7 == 0] = 200.0   # expf(-x) underflows, and expf(200) overflows in the sigmoid of -200
    pinned[:, col % 7 == 3] = -200.0
    gin = torch.cat([gin, pinned[None]])
    ld_g = 8 * H + 8
    g_bs = T * ld_g + 16
    gb = torch.full((B, g_bs), NAN)
    for b, L in enumerate(LSTM_LENS):
        gb[b, :T * ld_g].view(T, ld_g)[:L, :8 * H] = gin[b, :L]
    return gb, w_hh, lstm_w_hh_t(w_hh[0], w_hh[1])


@functools.lru_cache(maxsize=None)
def lstm_ref(H, drive):
    """nn.LSTM (gates i, f, g, o; zero initial state), both directions, in float64: [(L, 2 H) per item]"""
    gb, w_hh, _ = lstm_inputs(H, drive)
    T, ld_g = LSTM_T, 8 * H + 8
    W = w_hh.double()
    refs = []
    for b, L in enumerate(LSTM_LENS):
        gv = gb[b, :T * ld_g].view(T, ld_g).double()
        o = torch.zeros(L, 2 * H, dtype=torch.float64)
        for d in range(2):
            h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
            for t in (range(L - 1, -1, -1) if d else range(L)):
                i, f, gg, og = (gv[t, d * 4 * H:(d + 1) * 4 * H] + W[d] @ h).view(4, H)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
                h = torch.sigmoid(og) * torch.tanh(c)
                o[t, d * H:(d + 1) * H] = h
        refs.append(o)
    return refs


def check_lstm(case, run):
    H, drive = case
    gb, _, w_t = lstm_inputs(H, drive)
    T, B = LSTM_T, len(LSTM_LENS)
    ld_g, ld_out = 8 * H + 8, 2 * H + 8

    def launch(g, lens, n):
        full, out = guarded(n * T * ld_out)
        run("srn_bilstm_recur", (g, gb.shape[1], ld_g, i32(lens), w_t, out[4:], T * ld_out, ld_out, n, T, H))
        o = out.view(n, T, ld_out)
        assert guards_intact(full) and bool(torch.isnan(o[..., :4]).all() and torch.isnan(o[..., 4 + 2 * H:]).all()), case
        return o[..., 4:4 + 2 * H]

    o = launch(gb, LSTM_LENS, B)
    worst = 0.0
    for b, (L, ref) in enumerate(zip(LSTM_LENS, lstm_ref(H, drive))):
        assert bool((o[b, L:] == 0).all()), (case, b)
        assert bool(torch.isfinite(o[b]).all()), (case, b)
        if L:
            worst = worse(worst, rel_err(o[b, :L], ref))
        one = launch(gb[b], [L], 1)  # the item on its own
        assert bits_equal(one[0], o[b]), (case, b, "the item in the batch differs from its own B = 1 call")
    return {"h": (worst, 2e-5)}


# ------------------------------------------------------------------------------------------------ E. ContentVec layer 0
CVEC_SHAPES = ((1, 64, 8), (16, 1, 260), (10, 5, 12), (10, 5, 512))  # (k, stride, C)
CVEC_LENS = {1: [1, 1, 0], 64: [64, 30, 0], 65: [65, 30, 0], 139: [139, 60, 0], 4200: [4200, 2000, 0]}
CVEC_CASES = tuple((k, s, C, T0, "rand") for k, s, C in CVEC_SHAPES for T0 in (1, 64, 65, 139)) \
    + ((10, 5, 12, 139, "dc"),       # offsets 2.0 and 1.25 under weights that sum to 3: mean / std up to about 60
       (10, 5, 512, 4200, "rand"))   # T C / 4 = 537 600 quads: the norm's grid-stride loop (the only path of real audio)
CVEC_SHORT_N = (10, 5, 12, 139, "rand")  # n three samples short of the last frame: they read as zero
CVEC_EPS = 1e-5
C0_FRAMES = 64
NORM_GRID_QUADS = 2048 * 256


@functools.lru_cache(maxsize=None)
def cvec_inputs(k, s, C, T0, kind):
    g = _gen(5000 + 100 * k + s + C + T0 + (kind == "dc"))
    lens = CVEC_LENS[T0]
    need = (T0 - 1) * s + k
    n = need - 3 if (k, s, C, T0, kind) == CVEC_SHORT_N else need
    wave = torch.full((3, n + 5), NAN)  # wave_bs > n; NaN past each item's own samples
    for b, L in enumerate(lens):
        own = min(n, (L - 1) * s + k) if L else 0
        v = torch.randn(own, generator=g)
        wave[b, :own] = (2.0 - 0.75 * b) + 0.1 * v if kind == "dc" else v
    w = 0.3 + 0.05 * torch.randn(C, k, generator=g) if kind == "dc" else 0.3 * torch.randn(C, k, generator=g)
    w[1] = 0.0  # a constant channel: variance 0
    return wave, n, w, 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


@functools.lru_cache(maxsize=None)
def cvec_conv_ref(k, s, C, T0, kind):
    wave, n, w, _, _ = cvec_inputs(k, s, C, T0, kind)
    refs = []
    for b, L in enumerate(CVEC_LENS[T0]):
        if not L:
            refs.append(None)
            continue
        x = torch.zeros((L - 1) * s + k, dtype=torch.float64)
        own = min(n, len(x))
        x[:own] = wave[b, :own].double()
        refs.append(F.conv1d(x.view(1, 1, -1), w.double().view(C, 1, k), stride=s)[0].t())  # (L, C)
    return refs


def check_cvec(case, run):
    k, s, C, T0, kind = case
    wave, n, w, gamma, beta = cvec_inputs(*case)
    lens, B = CVEC_LENS[T0], 3
    lens_t = i32(lens)
    chunks = (T0 + C0_FRAMES - 1) // C0_FRAMES
    fo, out = guarded(B * T0 * C)
    fp, parts = guarded(B * chunks * C * 2, torch.float64)
    run("srn_cvec_conv0", (wave, wave.shape[1], n, lens_t, w, out, parts, B, T0, C, k, s))
    assert guards_intact(fo) and guards_intact(fp), case
    o, p = out.view(B, T0, C), parts.view(B, chunks, C, 2)
    res = {"conv": 0.0, "partials": 0.0, "norm": 0.0, "stats": 0.0}
    # ---- the norm: out of place into NaN, then in place on a copy of the conv output
    fs, stats = guarded(B * C * 2)
    fy, y = guarded(B * T0 * C)
    norm = lambda x_, st_, y_: run("srn_channel_norm_gelu", (x_, parts, chunks, lens_t, gamma, beta, st_, y_, B, T0, C,
                                                             CVEC_EPS))
    norm(out, stats, y)
    fs2, stats2 = guarded(B * C * 2)
    fy2, y2 = guarded(B * T0 * C)
    y2.copy_(out)
    norm(y2, stats2, y2)
    assert guards_intact(fs) and guards_intact(fy) and guards_intact(fo), case
    assert bits_equal(fy, fy2) and bits_equal(fs, fs2), (case, "in place differs from out of place")
    yv, sv = y.view(B, T0, C), stats.view(B, C, 2)
    eps = float(np.float32(CVEC_EPS))
    rstd0 = float(np.float32(1.0 / np.sqrt(np.float64(eps))))
    for b, (L, ref) in enumerate(zip(lens, cvec_conv_ref(*case))):
        assert bool((o[b, L:] == 0).all() and (yv[b, L:] == 0).all()), (case, b)
        v = torch.zeros(chunks * C0_FRAMES, C, dtype=torch.float64)
        v[:L] = o[b, :L].double()  # the kernel's OWN outputs: partials, statistics and the norm are judged alone
        pref = torch.stack([v.view(chunks, C0_FRAMES, C).sum(1), (v * v).view(chunks, C0_FRAMES, C).sum(1)], -1)
        for q in (0, 1):
            res["partials"] = worse(res["partials"], rel_err(p[b, ..., q], pref[..., q]))
        assert bool((p[b, :, 1] == 0).all()), (case, b)  # the all-zero weights
        if not L:
            assert bool((sv[b, :, 0] == 0).all() and (sv[b, :, 1] == rstd0).all()), (case, b)
            continue
        res["conv"] = worse(res["conv"], rel_err(o[b, :L], ref))
        mean = v[:L].mean(0)
        var = ((v[:L] - mean) ** 2).mean(0)
        rstd = 1.0 / torch.sqrt(var + eps)
        yref = gelu64((v[:L] - mean) * rstd * gamma.double() + beta.double())
        res["norm"] = worse(res["norm"], rel_err(yv[b, :L], yref))
        # statistics: fp32 roundings of fp64 values, relative to the channel's own figure (the mean: to its largest)
        res["stats"] = worse(res["stats"], abs_err(sv[b, :, 0], mean) / mean.abs().max().item(),
                           ((sv[b, :, 1].double() - rstd).abs() / rstd).max().item())
        assert sv[b, 1, 0].item() == 0.0 and sv[b, 1, 1].item() == rstd0, (case, b, "rstd of the constant channel")
        assert (yv[b, :L, 1].double() - gelu64(beta[1].double())).abs().max().item() <= 2e-5 * yref.abs().max().item()
    return {"conv": (res["conv"], 1e-6), "partials": (res["partials"], 1e-12), "norm": (res["norm"], 2e-5),
            "stats": (res["stats"], 2.0 ** -22)}


# ------------------------------------------------------------------------------------------------ F. positional conv
POS_SHAPES = ((4, 1, 0), (16, 7, 3), (36, 7, 0), (36, 7, 6), (60, 16, 8), (64, 128, 64))  # (channels per group, K, pad)
POS_GROUPS = 4
POS_LENS = {1: [1, 1], 128: [128, 64], 129: [129, 65], 300: [300, 150, 20, 0]}  # 300: whole 128-row tiles past items 1, 2
POS_CASES = tuple((Cg, K, pad, T) for Cg, K, pad in POS_SHAPES for T in POS_LENS)
PC_BM = 128


def pos_lds_bytes(Cg, K):
    return (PC_BM + K - 1) * (Cg + 1) * 4


@functools.lru_cache(maxsize=None)
def pos_inputs(Cg, K, pad, T):
    """weight-normed weights through the model's own packing (ContentVec.fold_pos_weight + pack_pos_weight), gains of
    sqrt(D / K) so that the conv has about the variance of x"""
    g = _gen(6000 + 10 * Cg + K + pad + T)
    D, B = Cg * POS_GROUPS, len(POS_LENS[T])
    wg = math.sqrt(D / K) * (1 + 0.1 * torch.randn(1, 1, K, generator=g))
    pw = ContentVec.fold_pos_weight(wg, torch.randn(D, Cg, K, generator=g))
    return torch.randn(B, T, D, generator=g), pw, ContentVec.pack_pos_weight(pw, POS_GROUPS), 0.1 * torch.randn(D, generator=g)


@functools.lru_cache(maxsize=None)
def pos_ref(Cg, K, pad, T, masked):
    """x + GELU(grouped conv + bias) of x[b, :L] alone, zero padding of `pad` rows in front and K - 1 - pad behind (for
    an even K with pad = K / 2 that is Conv1d(padding = K / 2) with its last frame dropped, HubertSamePadLayer)"""
    x, pw, _, bias = pos_inputs(Cg, K, pad, T)
    refs = []
    for b, L in enumerate(POS_LENS[T] if masked else [T] * x.shape[0]):
        if not L:
            refs.append(None)
            continue
        xv = x[b, :L].double().t().unsqueeze(0)
        c = F.conv1d(F.pad(xv, (pad, K - 1 - pad)), pw.double(), bias.double(), groups=POS_GROUPS)[0].t()
        refs.append(x[b, :L].double() + gelu64(c))
    return refs


def check_pos(case, run):
    Cg, K, pad, T = case
    x, _, wp, bias = pos_inputs(*case)
    lens = POS_LENS[T]
    B, D = len(lens), Cg * POS_GROUPS

    def launch(xin, lens_t):
        full, y = guarded(B * T * D)
        run("srn_posconv_gelu_res", (xin, lens_t, wp, bias, y, B, T, D, POS_GROUPS, K, pad))
        assert guards_intact(full), case
        return y.view(B, T, D)

    worst = 0.0
    y = launch(x, i32(lens))  # finite x everywhere: every row is finite, valid rows follow x[b, :L] alone
    assert bool(torch.isfinite(y).all()), case
    xn = x.clone()
    for b, L in enumerate(lens):
        xn[b, L:] = NAN
    yn = launch(xn, i32(lens))  # NaN past each length: no valid row may see it
    for b, (L, ref) in enumerate(zip(lens, pos_ref(Cg, K, pad, T, True))):
        assert bits_equal(yn[b, :L], y[b, :L]), (case, b, "rows past the length reached a valid row")
        if L:
            worst = worse(worst, rel_err(y[b, :L], ref))
    if T == 129:  # lens == nullptr: every row is valid
        yf = launch(x, None)
        assert bool(torch.isfinite(yf).all()), case
        for b, ref in enumerate(pos_ref(Cg, K, pad, T, False)):
            worst = worse(worst, rel_err(yf[b], ref))
    return {"posconv": (worst, 1e-5)}
