"""Thin Python wrappers over the C ABI (include/serenade_hip.h).

Tensors are torch CUDA fp32 tensors used as device memory only; every wrapper passes raw
pointers, sizes and the current HIP stream.  All activations are channels-last (B, T, C).
Nothing here computes on the host and nothing falls back to torch ops or to ``oracle/``.

An op holds a reference to every tensor whose address it was built from (the ``kw`` of the struct-parameter ops,
``CallOp.targs``, ``MultiCopyOp.srcs / dst``, ``TransposeMultiOp.entries``), so a plan's buffers live exactly as long as
its op list does: plans keep no separate list of their buffers.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import (ACT_LEAKY, ACT_MISH, ACT_NONE, ACT_SILU, POST_DIV, POST_LEAKY, POST_NONE, POST_RELU,  # noqa: F401
                   POST_TANH,
                   RES_ADD, RES_AXPY, RES_NONE, SrnConvParams, SrnExcitationParams, SrnResUnitParams, SrnWorldParams,
                   check)


DEFAULT_PRECISION = _lib.PREC_FP32  # contraction arithmetic of ops built without an explicit precision
ATTENTION_PRECISION = None  # Q K^T / P V of the estimator's self-attention; None: DEFAULT_PRECISION


def attention_precision():
    return DEFAULT_PRECISION if ATTENTION_PRECISION is None else ATTENTION_PRECISION
# Split-K for launches whose tile grid cannot fill the chip (B = 1 / short utterances; conv_splitk.hip): every ConvOp
# is handed the per-device workspace below and the library decides per call.  SERENADE_AMD_SPLITK=0 turns it off.
SPLITK = os.environ.get("SERENADE_AMD_SPLITK", "1") != "0"
SPLITK_WS_BYTES = 32 << 20  # upper bound of the library's need (<= 192 tiles of 64 x 64, <= 8 slices, fp32)
_SPLITK_WS = {}
PROFILE = None  # set to a list by bench.py to collect (start event, end event, op) per conv_gemm launch


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(x):
    """tensor | (tensor, element_offset) | None -> raw device address (int) or None.  The offset of the pair form
    counts 4-byte elements (fp32 / int32 buffers); the float64 front-ends pass tensors or views, never pairs."""
    if x is None:
        return None
    if isinstance(x, tuple):
        t, off = x
        return t.data_ptr() + 4 * int(off)
    return x.data_ptr()


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32, "expected a CUDA fp32 tensor"
    return t


class _StructOp:
    """A prebuilt call of an entry point that takes one filled parameter struct and the stream: `p` the struct
    (parameters frozen, pointers borrowed from live tensors), `kw` the keywords it was filled from -- kept for
    introspection (tests emulate the C-ABI contract from it) and to pin the tensors -- and `name` the entry point."""

    __slots__ = ("p", "kw", "name", "_fn")
    _profiled = False  # True: bench.py's PROFILE collects (start event, end event, op) around every launch

    def __init__(self, name, kw):
        self.name, self.kw, self._fn = name, kw, getattr(_lib.lib(), name)
        self.p = self._fill(**kw)

    def __call__(self, stream=None):
        timed = self._profiled and PROFILE is not None and stream is None
        if timed:  # bench.py: HIP events on the launch stream around the launch
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
        check(self._fn(ctypes.byref(self.p), stream if stream is not None else _stream()), self.name)
        if timed:
            e.record()
            PROFILE.append((s, e, self))


class ConvOp(_StructOp):
    """A prebuilt srn_conv_gemm call."""

    __slots__ = ("_wplanes",)
    _profiled = True

    def __init__(self, **kw):
        super().__init__("srn_conv_gemm", kw)

    def _fill(self, *, in0, w, out, n_batch, T_in, T_out, C_in, N, ld_in0, ldw, ld_out, taps=(0,), n_head=1,
                 in0_bs=0, in0_hs=0, in1=None, C_in0=0, in1_bs=0, ld_in1=0, C_w=0, w_bs=0, w_hs=0, w_nmajor=False,
                 bias=None, len_in=None, len_out=None, in_stride=1, reflect=False, pro_act=ACT_NONE, pro_slope=0.0,
                 alpha=1.0, beta=0.0, geglu=False, res=None, res_mode=RES_NONE, res_bs=0, res_hs=0, ld_res=0, res2=None,
                 res2_bs=0, ld_res2=0, post=POST_NONE, post_div=1.0, out_bs=0, out_hs=0, out_t_stride=1, out_t_off=0,
                 gn_partials=None, N_out=0, tile=0, precision=None, route=_lib.ROUTE_AUTO, out_tr=None, out_tr_bs=0,
                 ld_out_tr=0, out_tr_col0=0, no_halo=None):
        p = SrnConvParams()
        p.n_batch, p.n_head, p.T_in, p.T_out = int(n_batch), int(n_head), int(T_in), int(T_out)
        p.C_in, p.C_in0, p.C_w, p.N, p.N_out = int(C_in), int(C_in0), int(C_w), int(N), int(N_out)
        taps = [int(t) for t in taps]
        assert 1 <= len(taps) <= _lib.SRN_MAX_TAPS
        p.n_taps = len(taps)
        for i, t in enumerate(taps):
            p.tap_off[i] = t
        p.in_stride, p.pad_reflect, p.w_nmajor = int(in_stride), int(reflect), int(bool(w_nmajor))  # reflect: 0 / 1 / 2
        p.pro_act, p.pro_slope, p.alpha, p.beta = int(pro_act), float(pro_slope), float(alpha), float(beta)
        p.geglu, p.res_mode, p.post, p.post_div = int(bool(geglu)), int(res_mode), int(post), float(post_div)
        p.out_t_stride, p.out_t_off, p.tile = int(out_t_stride), int(out_t_off), int(tile)
        p.in0, p.in0_bs, p.in0_hs, p.ld_in0 = _ptr(in0), int(in0_bs), int(in0_hs), int(ld_in0)
        p.in1, p.in1_bs, p.ld_in1 = _ptr(in1), int(in1_bs), int(ld_in1)
        p.w, p.w_bs, p.w_hs, p.ldw = _ptr(w), int(w_bs), int(w_hs), int(ldw)
        p.bias, p.len_in, p.len_out = _ptr(bias), _ptr(len_in), _ptr(len_out)
        p.res, p.res_bs, p.res_hs, p.ld_res = _ptr(res), int(res_bs), int(res_hs), int(ld_res)
        p.res2, p.res2_bs, p.ld_res2 = _ptr(res2), int(res2_bs), int(ld_res2)
        p.out, p.out_bs, p.out_hs, p.ld_out = _ptr(out), int(out_bs), int(out_hs), int(ld_out)
        p.gn_partials = _ptr(gn_partials)
        p.out_tr, p.out_tr_bs, p.ld_out_tr, p.out_tr_col0 = _ptr(out_tr), int(out_tr_bs), int(ld_out_tr), int(out_tr_col0)
        p.precision = int(DEFAULT_PRECISION if precision is None else precision)
        # _lib.ROUTE_*: kernel selection (testing / A-B timing); no_halo is its former name, same values
        p.route = int(route if no_halo is None else no_halo)
        self._wplanes = None
        if p.precision in (_lib.PREC_BF16X3, _lib.PREC_BF16X6):
            # static weights are split once, at plan-build time, into the bf16 plane images conv_fast.hip streams
            # straight into LDS: (hi | lo) for bf16x3; (hi | mid) + a separate lo plane for bf16x6
            if isinstance(w, torch.Tensor) and w.is_cuda and p.w_bs == 0 and p.w_hs == 0 and not w_nmajor:
                self._wplanes = weight_planes(w, p.N, p.n_taps, p.C_in, p.ldw, three=p.precision == _lib.PREC_BF16X6)
                p.w_hi = self._wplanes[0].data_ptr()
                if p.precision == _lib.PREC_BF16X6:
                    p.w_lo = self._wplanes[2].data_ptr()
        if SPLITK and isinstance(out, (torch.Tensor, tuple)):
            o = out[0] if isinstance(out, tuple) else out
            if o.is_cuda and self._fn and _lib.lib().srn_conv_gemm_workspace_bytes(ctypes.byref(p)) > 0:
                ws = splitk_workspace(o.device)  # one per device: the ops of a plan run back to back on one stream
                p.ws, p.ws_bytes = ws.data_ptr(), ws.numel()
        return p


def splitk_workspace(device):
    """the split-K partial-sum slab of the stream that is current while an op is BUILT: ops of one plan run back to
    back on the stream they were built under, and two streams never share a slab (plans driven from different streams
    would overwrite each other's partial sums).  Built under a graph capture, the slab comes from the graph's pool
    and is keyed by the capture stream, so eager code cannot pick it up."""
    stream = torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0
    key = (str(device), stream)
    if key not in _SPLITK_WS:
        _SPLITK_WS[key] = torch.empty(SPLITK_WS_BYTES, dtype=torch.uint8, device=device)
    return _SPLITK_WS[key]


def _item_lens(lens, n_batch, what):
    """the `lens` of a ragged op: an int32 device tensor of (at least) n_batch per-item row counts, read when the op
    RUNS (a plan rewrites it in place between runs)"""
    if not (isinstance(lens, torch.Tensor) and lens.dtype == torch.int32 and lens.numel() >= int(n_batch)):
        raise TypeError(f"{what}: lens must be an int32 tensor of n_batch entries")
    return lens


class ResUnitOp(_StructOp):
    """A prebuilt srn_hifigan_resunit call: one fused HiFi-GAN residual unit (see include/serenade_hip.h).  With `lens`
    (_item_lens) it is a srn_hifigan_resunit_ragged call of the same struct: item b is computed as its own n_batch = 1,
    T = lens[b] dense call; rows at or past lens[b] are neither read nor written.  With `lead` (_item_lens) it is a
    srn_hifigan_resunit_causal call: both convs reach back only, `x` holds (k - 1) (dilation + 1) history rows in front
    of each item's T rows, and item b's utterance began clamp(lead[b], 0, history) rows before this call's first."""

    __slots__ = ("_wplanes",)
    _profiled = True  # timed with the other contraction launches

    def __init__(self, lens=None, lead=None, **kw):
        if lens is None and lead is None:
            super().__init__("srn_hifigan_resunit", kw)
            return
        if lead is not None:
            if lens is not None:
                raise TypeError("ResUnitOp: lens and lead exclude each other")
            super().__init__("srn_hifigan_resunit_causal", dict(kw, lead=_item_lens(lead, kw["n_batch"], "ResUnitOp")))
        else:
            super().__init__("srn_hifigan_resunit_ragged", dict(kw, lens=_item_lens(lens, kw["n_batch"], "ResUnitOp")))
        entry, data_p = self._fn, ctypes.c_void_p(_ptr(lens if lead is None else lead))
        self._fn = lambda p, stream: entry(p, data_p, stream)

    def _fill(self, *, x, w1, b1, w2, b2, out, n_batch, T, C, k, dilation, slope, res2=None, post_div=0.0,
              precision=None, route=0, x_bs=None, res2_bs=None, out_bs=None, lens=None, lead=None):
        p = SrnResUnitParams()
        p.n_batch, p.T, p.C, p.k, p.dilation, p.slope = int(n_batch), int(T), int(C), int(k), int(dilation), float(slope)
        item = int(T) * int(C)  # batch strides: contiguous items unless given
        hist = 0 if lead is None else (int(k) - 1) * (int(dilation) + 1) * int(C)  # the causal item's rows in front
        p.x, p.x_bs = _ptr(x), item + hist if x_bs is None else int(x_bs)
        p.w1, p.b1, p.w2, p.b2 = _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2)
        p.res2, p.res2_bs = _ptr(res2), item if res2_bs is None else int(res2_bs)
        p.post_div = float(post_div)
        p.out, p.out_bs = _ptr(out), item if out_bs is None else int(out_bs)
        p.precision = int(DEFAULT_PRECISION if precision is None else precision)
        p.route = int(route)  # _lib.RESUNIT_ROUTE_SHARED: resunit.hip's exact-fp32 form (testing / A-B timing)
        self._wplanes = None
        if p.precision == _lib.PREC_BF16X3 and w1.is_cuda and lead is None:  # the causal unit runs exact fp32
            self._wplanes = (weight_planes(w1, C, k, C, k * C), weight_planes(w2, C, k, C, k * C))
            p.w1_hi, p.w2_hi = self._wplanes[0][0].data_ptr(), self._wplanes[1][0].data_ptr()
        return p


class MultiCopyOp:
    """srn_multi_copy: many small device-to-device copies as one launch per 160 entries -- src tensor i (contiguous
    fp32) goes to dst.view(-1)[offs[i] : offs[i] + src.numel()].  The table travels in the kernel arguments, so the call
    can sit inside a captured hipGraph."""

    __slots__ = ("srcs", "offs", "dst", "_lists", "_fn")

    def __init__(self, srcs, offs, dst):
        self.srcs, self.offs, self.dst = list(srcs), [int(o) for o in offs], dst
        self._fn = _lib.lib().srn_multi_copy
        self._lists = []
        for i0 in range(0, len(self.srcs), _lib.SRN_COPY_LIST_MAX):
            lst = _lib.SrnCopyList()
            chunk = self.srcs[i0:i0 + _lib.SRN_COPY_LIST_MAX]
            lst.n = len(chunk)
            for j, t in enumerate(chunk):
                assert t.is_contiguous() and t.dtype == torch.float32
                lst.src[j], lst.off[j], lst.len[j] = t.data_ptr(), self.offs[i0 + j], t.numel()
            self._lists.append(lst)

    def __call__(self, stream=None):
        st = stream if stream is not None else _stream()
        for lst in self._lists:
            check(self._fn(ctypes.byref(lst), _ptr(self.dst), st), "srn_multi_copy")


class TransposeMultiOp:
    """srn_transpose_multi: a table of batched 2-D transposes as one launch per 40 entries.  entries: (src, dst, B, R,
    Cc, src_bs, ld_src, dst_bs, ld_dst) with dst[b][c][r] = src[b][r][c]; src / dst: tensor or (tensor, element offset)."""

    __slots__ = ("entries", "_lists", "_fn")

    def __init__(self, entries):
        self.entries = list(entries)
        self._fn = _lib.lib().srn_transpose_multi
        self._lists = []
        for i0 in range(0, len(self.entries), _lib.SRN_TR_LIST_MAX):
            lst = _lib.SrnTransposeList()
            chunk = self.entries[i0:i0 + _lib.SRN_TR_LIST_MAX]
            lst.n = len(chunk)
            for j, (src, dst, B, R, Cc, src_bs, ld_src, dst_bs, ld_dst) in enumerate(chunk):
                lst.src[j], lst.dst[j] = _ptr(src), _ptr(dst)
                lst.B[j], lst.R[j], lst.Cc[j] = B, R, Cc
                lst.src_bs[j], lst.ld_src[j], lst.dst_bs[j], lst.ld_dst[j] = src_bs, ld_src, dst_bs, ld_dst
            self._lists.append(lst)

    def __call__(self, stream=None):
        st = stream if stream is not None else _stream()
        for lst in self._lists:
            check(self._fn(ctypes.byref(lst), st), "srn_transpose_multi")


_TN_WS = {}


_TN_OUTGROWN = []


def tn_workspace(device, nbytes):
    """slices of a time-sliced srn_tn_gemm: per (device, stream) like the split-K slab, grown on demand.  An outgrown
    slab is kept alive, not freed: a captured graph (training.GraphedStep) may have its address baked in, and the ops
    that took it are transient.  Growth is by doubling at least, so the kept slabs sum to less than the live one."""
    stream = torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0
    key = (str(device), stream)
    old = _TN_WS.get(key)
    if old is None or old.numel() < nbytes:
        if old is not None:
            _TN_OUTGROWN.append(old)
        _TN_WS[key] = torch.empty(max(nbytes, 64 << 20, 2 * (old.numel() if old is not None else 0)),
                                  dtype=torch.uint8, device=device)
    return _TN_WS[key]


class TnGemmOp(_StructOp):
    """srn_tn_gemm (include/serenade_hip.h): out[z, m, j*N + n] = alpha * sum_{item,t} a[z,item,t,m] *
    b[z,item,t*stride + shifts[j], n].  a / b / out: tensor or (tensor, element offset).  len_b (int32, per item): rows
    of b at or past it read as zero; colsum (M,): alpha * the column sums of a (a conv's bias gradient), same launch."""

    __slots__ = ("_ws",)

    def __init__(self, **kw):
        super().__init__("srn_tn_gemm", kw)

    def _fill(self, *, a, b, out, n_items, T_a, T_b, M, N, lda, ldb, ldc, shifts=(0,), stride=1, n_batch=1,
              n_head=1, a_bs=0, a_hs=0, a_is=0, b_bs=0, b_hs=0, b_is=0, out_bs=0, out_hs=0, alpha=1.0, n_inner=1,
              a_is2=0, b_is2=0, len_b=None, colsum=None, route=0):
        p = _lib.SrnTnGemmParams()
        p.n_batch, p.n_head, p.n_items, p.T_a, p.T_b = n_batch, n_head, n_items, T_a, T_b
        p.stride, p.n_shifts, p.M, p.N = stride, len(shifts), M, N
        for i, v in enumerate(shifts):
            p.shift[i] = int(v)
        p.a, p.a_bs, p.a_hs, p.a_is, p.lda = _ptr(a), a_bs, a_hs, a_is, lda
        p.b, p.b_bs, p.b_hs, p.b_is, p.ldb = _ptr(b), b_bs, b_hs, b_is, ldb
        p.out, p.out_bs, p.out_hs, p.ldc, p.alpha = _ptr(out), out_bs, out_hs, ldc, float(alpha)
        p.n_inner, p.a_is2, p.b_is2 = n_inner, a_is2, b_is2
        if len_b is not None and len_b.dtype != torch.int32:
            raise TypeError("TnGemmOp: len_b must be int32")
        p.len_b, p.colsum = _ptr(len_b), _ptr(colsum)
        p.route = int(route)  # _lib.TN_ROUTE_GENERAL: the general kernel only (testing / A-B timing)
        self._ws = None
        o = out[0] if isinstance(out, tuple) else out
        need = int(_lib.lib().srn_tn_gemm_workspace_bytes(ctypes.byref(p))) if o.is_cuda else 0
        if need:
            self._ws = tn_workspace(o.device, need)
            p.ws, p.ws_bytes = self._ws.data_ptr(), self._ws.numel()
        return p


class WorldOp(_StructOp):
    """A prebuilt srn_world_cheaptrick / srn_world_d4c call (`entry`): float64 tensors x (B, N), f0 and t (B, F), their
    valid counts x_len / n_frames (B,) int32, the FFT's twiddle table; out0 / out1 (B, F, ld) or None.  CheapTrick reads
    q1 and f0_floor, D4C threshold and the band window."""

    __slots__ = ()

    def __init__(self, entry, **kw):
        super().__init__(entry, kw)

    def _fill(self, *, x, x_len, f0, t, n_frames, twiddle, fs, fft_size, unvoiced_db, q1=0.0, f0_floor=0.0,
              threshold=0.0, band_window=None, n_bands=0, out0=None, out1=None):
        p = SrnWorldParams()
        p.n_batch, p.max_frames, p.fs, p.fft_size = f0.size(0), f0.size(1), int(fs), int(fft_size)
        p.x, p.x_bs, p.x_len = _ptr(x), x.stride(0), _ptr(x_len)
        p.f0, p.t, p.f_bs, p.n_frames, p.twiddle = _ptr(f0), _ptr(t), f0.stride(0), _ptr(n_frames), _ptr(twiddle)
        p.q1, p.f0_floor, p.threshold, p.unvoiced_db = float(q1), float(f0_floor), float(threshold), float(unvoiced_db)
        if band_window is not None:
            p.band_window, p.band_window_len, p.n_bands = _ptr(band_window), band_window.numel(), int(n_bands)
        if out0 is not None:
            p.out0, p.out0_bs, p.ld_out0 = _ptr(out0), out0.stride(0), out0.size(-1)
        if out1 is not None:
            p.out1, p.out1_bs, p.ld_out1 = _ptr(out1), out1.stride(0), out1.size(-1)
        return p


class ExcitationOp(_StructOp):
    """A prebuilt srn_sifigan_excitation call: f0 / df_f0 (B, F) float64 contours of the sine and of the dilated
    factors, n_frames (B,) int32, phase_ws (B, F) float64 scratch, noise (B, F hop) fp32 or None, sine (B, 1, F hop) and
    one dfs[i] (B, 1, F df_upsample[i]) per dense factor, fp32."""

    __slots__ = ()

    def __init__(self, **kw):
        super().__init__("srn_sifigan_excitation", kw)

    def _fill(self, *, f0, df_f0, n_frames, phase_ws, noise, sine, dfs, fs, hop, sine_amp, noise_amp, df_upsample,
              dense_factors):
        p = SrnExcitationParams()
        p.n_batch, p.max_frames, p.fs, p.hop = f0.size(0), f0.size(1), int(fs), int(hop)
        p.f0, p.df_f0, p.f_bs, p.n_frames = _ptr(f0), _ptr(df_f0), f0.stride(0), _ptr(n_frames)
        p.phase_ws, p.noise, p.sine = _ptr(phase_ws), _ptr(noise), _ptr(sine)
        p.sine_amp, p.noise_amp, p.n_df = sine_amp, noise_amp, len(dfs)
        for i, d in enumerate(dfs):
            p.dfs[i], p.df_upsample[i], p.dense_factors[i] = _ptr(d), df_upsample[i], dense_factors[i]
        return p


_WPLANES = {}  # (data_ptr, version, shape, ...) -> (planes, weight) bf16 weight planes, split once per weight VALUE


def clear_caches():
    """Drop the weight-plane cache (long-running services that load many checkpoints).
    Ops already built keep their own references, so existing plans stay valid."""
    _WPLANES.clear()


def drop_weight_planes(tensors):
    """Forget the cached planes of the given weight tensors (a module re-packing its weights calls this, so planes
    of a previous checkpoint can never be contracted with the new one even when the storage address is reused)."""
    ptrs = {t.data_ptr() for t in tensors if isinstance(t, torch.Tensor)}
    for key in [k for k in _WPLANES if k[0] in ptrs]:
        del _WPLANES[key]


def weight_planes(w, N, n_taps, C_in, ldw, three=False):
    """fp32 packed weights [N][n_taps * C_in] -> bf16 planes [N][n_taps][roundup(C_in, 32) / 32][hi 32 | lo 32],
    hi = bf16(w), lo = bf16(w - hi) (round-to-nearest-even, the same split the kernels apply to activations).
    three=True (bf16x6): the exact three-way split w = hi + mid + lo; returns (planes [..][hi 32 | mid 32], w,
    lo plane [N][n_taps][chunks][32]).
    The cache key carries the tensor's in-place version counter: `load_state_dict` copies into the live parameter
    (same address, version + 1), which therefore misses the cache and is split again."""
    try:
        version = w._version
    except RuntimeError:  # tensors created under torch.inference_mode() carry no counter (and cannot be written)
        version = -1
    key = (w.data_ptr(), version, tuple(w.shape), N, n_taps, C_in, ldw, bool(three))
    if key not in _WPLANES:
        for stale in [k for k in _WPLANES if k[0] == key[0] and k[2:] == key[2:]]:
            del _WPLANES[stale]  # an older value of the same tensor
        cp = (C_in + 31) // 32 * 32
        src = w.reshape(-1)[: N * ldw].view(N, ldw)[:, : n_taps * C_in].reshape(N, n_taps, C_in)
        full = torch.zeros(N, n_taps, cp, device=w.device, dtype=torch.float32)
        full[:, :, :C_in] = src
        hi = full.to(torch.bfloat16)
        r1 = full - hi.to(torch.float32)
        lo = r1.to(torch.bfloat16)  # bf16x3: second plane; bf16x6: the MID plane
        # kernel layout: per row, per 32-channel chunk, [32 hi | 32 lo]  (one 128-B line per chunk)
        pl = torch.stack([hi.view(N, n_taps, cp // 32, 32), lo.view(N, n_taps, cp // 32, 32)], dim=3).contiguous()
        if three:
            third = (r1 - lo.to(torch.float32)).to(torch.bfloat16).view(N, n_taps, cp // 32, 32).contiguous()
            _WPLANES[key] = (pl, w, third)
        else:
            _WPLANES[key] = (pl, w)  # keep `w` alive so the data_ptr key stays unique
    return _WPLANES[key]


class CallOp:
    """A prebuilt call of any other C-ABI function (stream appended at run time)."""

    __slots__ = ("_fn", "_args", "targs", "name")

    def __init__(self, name, targs):
        self._fn = getattr(_lib.lib(), name)
        self.targs = tuple(targs)  # python-level arguments (tensors / scalars), pins the tensors
        self._args = tuple(_ptr(a) if (a is None or isinstance(a, (torch.Tensor, tuple))) else a for a in targs)
        self.name = name

    def __call__(self, stream=None):
        check(self._fn(*self._args, stream if stream is not None else _stream()), self.name)


def call(name, *args):
    """one-shot: build the CallOp and run it on the current stream"""
    CallOp(name, args)()


# ------------------------------------------------------------------ op builders (return CallOp)
def gn_mish_apply_op(x, partials, gamma, beta, time_bias, lens, y, B, T, C, groups=8, eps=1e-5, tb_bs=0,
                     valid_stats=False):
    return CallOp("srn_gn_mish_apply", (x, partials, gamma, beta, time_bias, tb_bs, lens, y, B, T, C, groups, eps,
                                        int(bool(valid_stats))))


def resblock_tail_op(c2, partials, gamma, beta, lens, r, scale, shift, ld_ss, y, B, T, C, groups=8, gn_eps=1e-5,
                     ln_eps=1e-5, valid_stats=False):
    return CallOp("srn_resblock_tail", (c2, partials, gamma, beta, lens, r, scale, shift, ld_ss, y, B, T, C, groups,
                                        gn_eps, ln_eps, int(bool(valid_stats))))


def resblock_tail_ln_op(c2, partials, gamma, beta, lens, r, scale, shift, ld_ss, y, ln_w, ln_b, y2, B, T, C, groups=8,
                        gn_eps=1e-5, ln_eps=1e-5, valid_stats=False, ln2_eps=1e-5):
    """resblock_tail_op + the LayerNorm that opens the transformer block behind it, in one launch"""
    return CallOp("srn_resblock_tail_ln", (c2, partials, gamma, beta, lens, r, scale, shift, ld_ss, y, B, T, C, groups,
                                           gn_eps, ln_eps, int(bool(valid_stats)), ln_w, ln_b, y2, ln2_eps))


def scatter_rows_op(src, src_bs, ld_src, dst, dst_bs, ld_dst, dc0, row_off, n_rows, B, T, C):
    return CallOp("srn_scatter_rows", (src, src_bs, ld_src, dst, dst_bs, ld_dst, dc0, row_off, n_rows, B, T, C))


def layernorm_op(x, gamma, beta, y, rows, C, eps=1e-5):
    return CallOp("srn_layernorm", (x, gamma, beta, y, rows, C, eps))


def softmax_rows_op(s, lens, Z, n_head, L, ld):
    return CallOp("srn_softmax_rows", (s, lens, Z, n_head, L, ld))


def sinusoidal_emb_op(t, out, n, dim, ld, scale=1000.0):
    return CallOp("srn_sinusoidal_emb", (t, out, n, dim, ld, scale))


def copy_channels_op(src, src_bs, ld_src, sc0, dst, dst_bs, ld_dst, dc0, B, T, C):
    return CallOp("srn_copy_channels", (src, src_bs, ld_src, sc0, dst, dst_bs, ld_dst, dc0, B, T, C))


def transpose_op(src, dst, B, R, Cc, src_bs, ld_src, dst_bs, ld_dst):
    """dst[b][c][r] = src[b][r][c]"""
    return CallOp("srn_transpose_ct", (src, dst, B, R, Cc, src_bs, ld_src, dst_bs, ld_dst))


def renorm_op(x, trg_scale, trg_mean, voc_mean, voc_scale, y, rows, C):
    return CallOp("srn_renorm", (x, trg_scale, trg_mean, voc_mean, voc_scale, y, rows, C))


def out_conv_tanh_op(x, w, bias, y, B, T, C, k, slope, lens=None):
    """lens (_item_lens): a ragged batch, lens[b] rows of item b; y is zero past each item's end"""
    if lens is None:
        return CallOp("srn_out_conv_tanh", (x, w, bias, y, B, T, C, k, slope))
    lens = _item_lens(lens, B, "out_conv_tanh_op")
    return CallOp("srn_out_conv_tanh_ragged", (x, w, bias, y, lens, B, T, C, k, slope))


def out_conv_tanh_causal_op(x, w, bias, y, B, T, C, k, slope):
    """x (B, (k - 1) + T, C): k - 1 history rows in front of each item's T rows (zeros at the start of an utterance)"""
    return CallOp("srn_out_conv_tanh_causal", (x, w, bias, y, B, T, C, k, slope))


def pd_gather_op(x, d, out, B, T, C, dilation, slope, lens=None):
    """lens (_item_lens): a ragged batch, lens[b] rows of item b; rows past an item's end are neither read nor
    written"""
    if lens is None:
        return CallOp("srn_pd_gather", (x, d, out, B, T, C, float(dilation), float(slope)))
    lens = _item_lens(lens, B, "pd_gather_op")
    return CallOp("srn_pd_gather_ragged", (x, d, lens, out, B, T, C, float(dilation), float(slope)))


def gru_recur_last_op(gi, w_hh_t, b_hh, h, B, T, H):
    return CallOp("srn_gru_recur_last", (gi, w_hh_t, b_hh, h, B, T, H))


def gru_recur_last_ragged_op(gi, w_hh_t, b_hh, h, n_steps, B, T_cap, H):
    """n_steps (_item_lens): item b's recurrence ends after n_steps[b] of its T_cap rows of gi"""
    n_steps = _item_lens(n_steps, B, "gru_recur_last_ragged_op")
    return CallOp("srn_gru_recur_last_ragged", (gi, w_hh_t, b_hh, h, n_steps, B, T_cap, H))


def zero_rows_ragged_op(x, bs, n_cols, n_rows, B, rows_cap):
    """n_rows (_item_lens): rows [n_rows[b], rows_cap) of item b of x (n_cols floats each, items bs floats apart)
    become zero"""
    n_rows = _item_lens(n_rows, B, "zero_rows_ragged_op")
    return CallOp("srn_zero_rows_ragged", (x, bs, n_cols, n_rows, B, rows_cap))


def replicate_first_row_op(x, bs, n_cols, lead, B):
    """lead (_item_lens): where lead[b] <= 0, row 0 of item b of x (rows of n_cols floats, items bs floats apart) becomes
    a copy of its row 1 -- ReplicationPad1d((1, 0)) of a stream that has not begun"""
    lead = _item_lens(lead, B, "replicate_first_row_op")
    return CallOp("srn_replicate_first_row", (x, bs, n_cols, lead, B))


def history_carry_ragged_ops(arena, entries, n, B):
    """n (_item_lens): for every entry (off, bs, H, T, C, scale) -- a [history | chunk] buffer inside `arena`, item b at
    float off + b * bs, H + T rows of C floats, `scale` rows per input frame -- and every item b, rows [0, H) become
    zero where n[b] < 0, stay where n[b] == 0, and take rows [m, m + H) with m = min(n[b], T // scale) * scale where
    n[b] > 0 (overlapping spans as a snapshot).  One launch per _lib.SRN_CARRY_MAX entries; the table travels in the
    kernel arguments, so the calls can sit inside a captured hipGraph."""
    n = _item_lens(n, B, "history_carry_ragged_ops")
    entries = [tuple(int(v) for v in e) for e in entries]
    out = []
    for i0 in range(0, len(entries), _lib.SRN_CARRY_MAX):
        table = _lib.SrnCarryTable()
        chunk = entries[i0:i0 + _lib.SRN_CARRY_MAX]
        table.n = len(chunk)
        for j, (off, bs, H, T, C, scale) in enumerate(chunk):
            e = table.e[j]
            e.off, e.bs, e.H, e.T, e.C, e.scale = off, bs, H, T, C, scale
        out.append(CallOp("srn_history_carry_ragged", (arena, table, n, B)))
    return out


def style_token_attention_kv_op(ref, wq_t, bq, k, v, wo_t, bo, out, B, Dq, n_tok, F, n_head):
    return CallOp("srn_style_token_attention_kv", (ref, wq_t, bq, k, v, wo_t, bo, out, B, Dq, n_tok, F, n_head))


# ------------------------------------------------------------------ weight packing (one-time, at load)
def pack_conv_weight(w, c_pad=None):
    """torch Conv1d weight (Co, Ci, k) -> [Co][k][Ci_pad] k-contiguous GEMM operand."""
    co, ci, k = w.shape
    cp = ci if c_pad is None else c_pad
    out = w.new_zeros(co, k, cp)
    out[:, :, :ci] = w.permute(0, 2, 1)
    return out.reshape(co, k * cp).contiguous()


def conv_taps(k, dilation=1, padding=None):
    """input-row offsets of a stride-1 Conv1d: tap j reads t + j*dilation - padding."""
    if padding is None:
        padding = (k - 1) // 2 * dilation
    return [j * dilation - padding for j in range(k)]


def convtranspose_phases(w, stride, padding):
    """torch ConvTranspose1d weight (Ci, Co, k) -> per output phase r (out index = m*stride + r):
    (taps = input-row offsets relative to m, packed weight [Co][n_taps*Ci]).
    out[o] = sum_i sum_k x[i] w[:, :, k] with o = i*stride - padding + k.
    Slices, stack and reshape only: autograd flows through it (the training step packs its up-sampling weights here)."""
    ci, co, k = w.shape
    phases = []
    for r in range(stride):
        taps, mats = [], []
        # k = r + padding + j*stride for integer j, 0 <= k < kernel;  i = m - j
        j = -((r + padding) // stride)
        while True:
            kk = r + padding + j * stride
            if kk >= k:
                break
            if kk >= 0:
                taps.append(-j)
                mats.append(w[:, :, kk].t())  # (Co, Ci)
            j += 1
        packed = torch.stack(mats, dim=1).reshape(co, len(taps) * ci).contiguous()
        phases.append((taps, packed))
    return phases


def convtranspose_phases_causal(w, stride):
    """convtranspose_phases for CausalConvTranspose1d (vocoder/layers/causal_conv.py:44-77): kernel 2 * stride, the
    input padded by one replicated row on the left, the first and last `stride` outputs cut.  Over a [1 history row |
    rows] buffer, whose row m + 1 is input row m, output m * stride + r is  W[:, :, r + stride]^T x[m - 1] +
    W[:, :, r]^T x[m]:  taps (0, 1) of the buffer for every phase."""
    ci, co, k = w.shape
    assert k == 2 * stride
    return [([0, 1], torch.stack([w[:, :, r + stride].t(), w[:, :, r].t()], dim=1).reshape(co, 2 * ci).contiguous())
            for r in range(stride)]


def pack_geglu(w, b):
    """GEGLU proj (2*inner, dim): rows [0, inner) = value, [inner, 2 inner) = gate  ->  rows interleaved in
    32-row (value | gate) groups so one 64-wide MFMA column span holds both halves of 32 outputs."""
    inner = w.shape[0] // 2
    assert inner % 32 == 0
    idx = torch.arange(inner, device=w.device).view(-1, 32)
    order = torch.cat([idx, idx + inner], dim=1).reshape(-1)
    return w[order].contiguous(), b[order].contiguous()


# ------------------------------------------------------------------ hipGraph replay of a fixed op list
GRAPHS = os.environ.get("SERENADE_AMD_GRAPHS", "0") == "1"


def set_graphs(enabled):
    """Replay plans (the per-utterance-batch op lists) as captured hipGraphs.  Pays off when launches, not kernels,
    bound the step: B=1 / short utterances (~1600 launches of 5-20 us each)."""
    global GRAPHS
    GRAPHS = bool(enabled)


class GraphRunner:
    """Runs `get_ops()` (a flat list of ConvOp / CallOp over static buffers) eagerly, or -- with GRAPHS on -- as one
    captured hipGraph.  The first call is always eager (every kernel sets its attributes and loads its code object
    outside capture); per-launch profiling (PROFILE) always runs eagerly.  `invalidate()` after any change of the op
    list or of a buffer address baked into it."""

    def __init__(self, get_ops):
        self._get_ops = get_ops
        self._graph = None
        self._warm = False

    def invalidate(self):
        self._graph = None
        self._warm = False

    def __call__(self):
        op_list = self._get_ops()
        if not GRAPHS or PROFILE is not None or not self._warm or not torch.cuda.is_available():
            for op in op_list:
                op()
            self._warm = True
            return
        if self._graph is None:
            g = torch.cuda.CUDAGraph()
            # callers run under torch.inference_mode() (flow_matching.py:39); capture bookkeeping (generator state
            # registration) must happen outside it.  Only C-ABI launches are recorded, no torch ops.
            with torch.inference_mode(False), torch.cuda.graph(g):
                for op in op_list:
                    op()
            self._graph = g
        self._graph.replay()
