"""The autograd nodes of the training step: forward and backward of every op are launches of the HIP library, built
by the builders of the inference plans (plan.conv_op, plan.attention_ops, ops.ConvOp / TnGemmOp / ops.call)."""
import math

import torch

from .. import _lib, ops
from .. import training as _root  # _root._require_cuda: the guard, bound once at the package root
from ..ops import ConvOp, TnGemmOp
from ..plan import attention_ops, conv_op, rup

_call = ops.call
_FP32 = _lib.PREC_FP32  # every contraction of the training step, whatever ops.DEFAULT_PRECISION says
NORM_BWD_ROWS = 8  # rows per chunk of partial sums in the LayerNorm / GroupNorm backward kernels (srn_rowln_chunks, srn_gn_chunks)

# =====================================================================================================================
#  conv / linear
# =====================================================================================================================

class _Conv(torch.autograd.Function):
    """y[b, t, :] = sum_j x[b, t * stride + taps[j], :] W_j^T + bias  (rows outside [0, T) read as zero).
    x (B, T, C) fp32 contiguous, C % 4 == 0; w packed (N, len(taps) * C), k-major; optional GroupNorm partial sums of
    the output (32 x 32 tiles, conv epilogue) as a second, non-differentiable result.
    lens (B,) int32 or None (stride 1 only): input rows t >= lens[b] count as zero -- the reference's `x * mask` in front
    of its convs (decoder.py:66-101) without the multiply: the forward reads them as zero (len_in), dX's rows past the
    length are stored as zero (len_out), and the weight gradient skips them (srn_tn_gemm's len_b)."""

    @staticmethod
    def forward(ctx, x, w, bias, taps, stride, T_out, want_gn, lens=None, wd=None):
        _root._require_cuda(x, "training.conv1d")
        B, T, C = x.shape
        N = w.shape[0]
        x, w = x.contiguous(), w.contiguous()
        y = torch.empty(B, T_out, N, device=x.device, dtype=torch.float32)
        part = None
        if want_gn:
            part = torch.empty(B, (T_out + 31) // 32, N // 32, 2, device=x.device, dtype=torch.float32)
        assert lens is None or stride == 1
        ctx.set_materialize_grads(False)  # no zero-filled gradient tensor for the non-differentiable partial sums
        conv_op(B, x, C, T, w, bias, y, N, T_out, taps, in_stride=stride, gn_partials=part, len_in=lens,
                precision=_FP32)()
        ctx.save_for_backward(x, w, wd)  # wd too: a re-laid buffer of the estimator, version-checked like w
        ctx.taps, ctx.stride, ctx.has_bias, ctx.lens = tuple(taps), stride, bias is not None, lens
        if want_gn:
            ctx.mark_non_differentiable(part)
            return y, part
        return y

    @staticmethod
    def backward(ctx, dy, *_):
        if dy is None:
            return (None,) * 9
        x, w, wd_saved = ctx.saved_tensors
        taps, stride, lens = ctx.taps, ctx.stride, ctx.lens
        B, T, C = x.shape
        _, T_out, N = dy.shape
        nt = len(taps)
        dy = dy.contiguous()
        dx = dw = db = None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[0]:
            # dgrad: dX[t] = sum_j dY[(t - taps[j]) / stride] W_j over the taps that divide -> a conv of dY with the
            # transposed weights Wd[c][j][n] = W[n][j][c]; with stride 2 one launch per output-row parity
            if wd_saved is not None:  # re-laid once for the whole step (Estimator._relay)
                wd = wd_saved.view(C, nt, N)
            else:
                wd = torch.empty(C, nt, N, device=dy.device, dtype=torch.float32)  # LDS tile transposes, one batch per tap
                _call("srn_transpose_ct", w, wd, nt, N, C, C, nt * C, N, nt * N)
            dx = torch.empty(B, T, C, device=dy.device, dtype=torch.float32)
            if stride == 1:
                conv_op(B, dy, N, T_out, wd.view(C, nt * N), None, dx, C, T, [-o for o in taps], len_out=lens,
                        precision=_FP32)()
            else:
                for ph in range(stride):
                    sel = [j for j, o in enumerate(taps) if (ph - o) % stride == 0]
                    rows = (T - ph + stride - 1) // stride
                    if rows <= 0:
                        continue
                    if not sel:
                        dx[:, ph::stride] = 0
                        continue
                    wsel = torch.stack([wd[:, j, :] for j in sel], dim=1).reshape(C, len(sel) * N)  # no host-side index tensor
                    conv_op(B, dy, N, T_out, wsel, None, dx, C, rows, [(ph - taps[j]) // stride for j in sel],
                            out_t_stride=stride, out_t_off=ph, out_bs=T * C, precision=_FP32)()
        if ctx.needs_input_grad[1]:
            # wgrad: dW_j = sum_{b,t} dY[b,t,:]^T x[b, t*stride + taps[j], :] -- a contraction over time on operands
            # that are time-major as they lie: srn_tn_gemm (rows outside the item read as zero; time sliced over
            # workgroups, slices added in order), straight into the packed (N, taps * C) layout; the bias gradient (the
            # column sums of dY) rides along in the same launch
            dw = torch.empty(N, nt * C, device=dy.device, dtype=torch.float32)
            if want_db and N % 4 == 0:
                db = torch.empty(N, device=dy.device, dtype=torch.float32)
            TnGemmOp(a=dy, b=x, out=dw, n_items=B, T_a=T_out, T_b=T, M=N, N=C, lda=N, ldb=C, ldc=nt * C, shifts=taps,
                     stride=stride, a_is=T_out * N, b_is=T * C, len_b=lens, colsum=db)()
        if want_db and db is None:
            db = _colsum(dy.reshape(-1, N))  # own kernel, not a torch reduction: see AdamW._grad_norm
        return dx, dw, db, None, None, None, None, None, None


def conv1d(x, w, bias, taps=(0,), stride=1, want_gn=False, T_out=None, lens=None, wd=None):
    """channels-last conv / linear over the HIP contraction kernel.  x (B, T, C) or (rows, C); w packed (N, k * C).
    T_out (stride 1 only): number of output rows when the input was padded by the caller (taps >= 0, "valid" conv).
    lens (B,) int32 (stride 1 only): conv of x with its rows past lens[b] zeroed (`x * mask`), see _Conv.
    wd: the weights already laid out for the input gradient, (C, taps * N) with wd[c, j * N + n] = w[n, j * C + c], when
    the caller keeps them (Estimator._relay); made on the fly otherwise."""
    two_d = x.dim() == 2
    if two_d:
        x = x.unsqueeze(0)
    T = x.shape[1]
    if T_out is not None:
        assert stride == 1 and max(taps) + T_out <= T
    elif stride == 1:
        T_out = T
    else:  # torch Conv1d with padding (k - 1) / 2: taps -p .. p
        p = -min(taps)
        T_out = (T + 2 * p - (len(taps) - 1) - 1) // stride + 1
    out = _Conv.apply(x, w, bias, tuple(int(t) for t in taps), int(stride), int(T_out), bool(want_gn), lens, wd)
    if two_d:
        return out.squeeze(0)
    return out


def _colsum(x):
    """column sums over the rows of a contiguous (R, N) matrix -> (N,), or per item of (B, R, N) -> (B, N)
    (srn_colsum: two small launches, fixed summation order)"""
    two_d = x.dim() == 2
    B, R, N = (1, *x.shape) if two_d else x.shape
    part = torch.empty(B, (R + 31) // 32, N, device=x.device, dtype=torch.float32)  # srn_colsum_chunks(R)
    out = torch.empty(B, N, device=x.device, dtype=torch.float32)
    _call("srn_colsum", x, part, out, B, R, N, N)
    return out[0] if two_d else out


class _AddRowBias(torch.autograd.Function):
    """h (B, T, C) + b (B, C) broadcast over T.  Its backward's column sums are srn_colsum launches instead of the
    reduction autograd would insert for the broadcast: see AdamW._grad_norm."""

    @staticmethod
    def forward(ctx, h, b):
        return h + b.unsqueeze(1)

    @staticmethod
    def backward(ctx, dy):
        B, T, C = dy.shape
        dy = dy.contiguous()
        return dy, _colsum(dy)


class _PackConv(torch.autograd.Function):
    """(N, C, k) -> (N, k * C_pad): per output channel a (C, k) -> (k, C) LDS tile transpose (srn_transpose_ct), zero pad
    columns; backward the transpose back.  (torch's strided copy of the same permute ran at < 1 TB/s and there are
    three of them per weight per step: pack, its gradient, and the dgrad operand.)"""

    @staticmethod
    def forward(ctx, w, c_pad):
        n, c, k = w.shape
        ctx.dims = (n, c, k, c_pad)
        w = w.contiguous()
        out = (torch.zeros if c_pad > c else torch.empty)(n, k * c_pad, device=w.device, dtype=torch.float32)
        _call("srn_transpose_ct", w, out, n, c, k, c * k, k, k * c_pad, c_pad)
        return out

    @staticmethod
    def backward(ctx, dp):
        n, c, k, c_pad = ctx.dims
        dw = torch.empty(n, c, k, device=dp.device, dtype=torch.float32)
        _call("srn_transpose_ct", dp.contiguous(), dw, n, k, c, k * c_pad, c_pad, c * k, k)
        return dw, None


class _PackAll(torch.autograd.Function):
    """Every conv weight of the estimator (N, C, k) -> (N, k * C_pad) in ONE launch, into buffers the estimator keeps
    (Estimator._relay), together with W^T of every conv / linear for the input gradients; backward: the packed gradients
    back to (N, C, k), one launch again.  Issued one by one these were ~140 launches of a few microseconds per step."""

    @staticmethod
    def forward(ctx, est, *weights):
        for op in est._relay_ops:
            op()
        # the launches above rewrote the persistent buffers through raw pointers: tell autograd, so that a backward of an
        # EARLIER forward (which saved aliases of them) raises instead of mixing its activations with these weights
        for t in (*est._pk.values(), *est._wd.values()):
            torch.autograd.graph.increment_version(t)
        ctx.est = est
        return tuple(est._pk[name].detach() for name in est._pack_names)  # fresh aliases: apply() marks its outputs

    @staticmethod
    def backward(ctx, *dps):
        est = ctx.est
        outs, entries = [], []
        for name, dp in zip(est._pack_names, dps):
            n, c, k = est.params[name].shape
            if dp is None:
                outs.append(None)
                continue
            c_pad = est._pk[name].shape[1] // k
            dp = dp.contiguous()
            dw = torch.empty(n, c, k, device=dp.device, dtype=torch.float32)
            entries.append((dp, dw, n, k, c, k * c_pad, c_pad, c * k, k))
            outs.append(dw)
        if entries:
            ops.TransposeMultiOp(entries)()
        return (None, *outs)


class _WeightNormPack(torch.autograd.Function):
    """torch weight_norm (w = g v / ||v|| per output channel) of a conv weight (N, C, k) straight into the packed k-major
    rows (N, k * C) the conv kernels read, plus W^T for the input gradient (`.wd` of the ctx-less return: second output,
    non-differentiable): srn_weight_norm_fwd / _bwd, one launch per direction instead of ~14 torch launches and three
    transposes per conv."""

    @staticmethod
    def forward(ctx, v, g):
        n, c, k = v.shape
        v, g = v.contiguous(), g.contiguous()
        w = torch.empty(n, k * c, device=v.device, dtype=torch.float32)
        wd = torch.empty(c, k * n, device=v.device, dtype=torch.float32)
        inv = torch.empty(n, device=v.device, dtype=torch.float32)
        _call("srn_weight_norm_fwd", v, g, w, wd, inv, n, c, k)
        ctx.save_for_backward(v, g, inv)
        ctx.mark_non_differentiable(wd)
        ctx.set_materialize_grads(False)  # no zero-filled "gradient" of wd
        return w, wd

    @staticmethod
    def backward(ctx, dw, _):
        if dw is None:
            return None, None
        v, g, inv = ctx.saved_tensors
        n, c, k = v.shape
        dv = torch.empty_like(v)
        dg = torch.empty(n, device=v.device, dtype=torch.float32)
        _call("srn_weight_norm_bwd", dw.contiguous(), v, g, inv, dv, dg, n, c, k)
        return dv, dg.view(g.shape)


def pack_conv(w, c_pad=None):
    """torch Conv1d weight (N, C, k) -> (N, k * C_pad), differentiable."""
    n, c, k = w.shape
    c_pad = c if c_pad is None else max(int(c_pad), c)
    if k == 1 and c_pad == c:
        return w.reshape(n, c)  # a view
    return _PackConv.apply(w, c_pad)


# =====================================================================================================================
#  GroupNorm -> Mish -> mask   (Block1D, decoder.py:66-77)
# =====================================================================================================================
def _gn_stats(part, T, C, groups, eps):
    """(mean, rstd) (B, groups) fp32 from the conv epilogue's 32 x 32 tile sums; statistics over the padded length"""
    B = part.shape[0]
    mean = torch.empty(B, groups, device=part.device, dtype=torch.float32)
    rstd = torch.empty(B, groups, device=part.device, dtype=torch.float32)
    _call("srn_gn_stats", part, mean, rstd, B, T, C, groups, eps)
    return mean, rstd


class _GNMish(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, part, gamma, beta, lens, groups, eps):
        B, T, C = h.shape
        y = torch.empty_like(h)
        _call("srn_gn_mish_apply", h, part, gamma, beta, None, 0, lens, y, B, T, C, groups, eps, 0)
        mean, rstd = _gn_stats(part, T, C, groups, eps)
        ctx.save_for_backward(h, mean, rstd, gamma, beta, lens)
        ctx.groups = groups
        return y

    @staticmethod
    def backward(ctx, dy):
        h, mean, rstd, gamma, beta, lens = ctx.saved_tensors
        G = ctx.groups
        B, T, C = h.shape
        dy = dy.contiguous()
        nch = (T + NORM_BWD_ROWS - 1) // NORM_BWD_ROWS
        part = torch.empty(B, nch, 2, C, device=h.device, dtype=torch.float32)
        _call("srn_gn_mish_bwd_partial", h, dy, mean, rstd, gamma, beta, lens, part, B, T, C, G)
        col = torch.empty(B, 2, C, device=h.device, dtype=torch.float32)  # sum_t dg, sum_t dg * xhat
        gsum = torch.empty(B, G, 2, device=h.device, dtype=torch.float32)
        _call("srn_chunk_colsum", part, gamma, col, gsum, B, nch, C, G)
        dcol = col.sum(0)
        dbeta, dgamma = dcol[0], dcol[1]
        dh = torch.empty_like(h)
        _call("srn_gn_mish_bwd_apply", h, dy, mean, rstd, gamma, beta, gsum, lens, dh, B, T, C, G)
        return dh, None, dgamma, dbeta, None, None, None


def gn_mish(h, part, gamma, beta, lens, groups=8, eps=1e-5):
    """mish(GroupNorm(h)) on rows < lens[b], zero after; `part` = the producing conv's GroupNorm partial sums."""
    return _GNMish.apply(h.contiguous(), part, gamma.contiguous(), beta.contiguous(), lens, groups, eps)


# =====================================================================================================================
#  per-frame LayerNorm with a per-(batch, channel) multiplier / offset: nn.LayerNorm and SpeakerAdapter
# =====================================================================================================================
class _RowLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, m, a, eps):
        B, T, C = x.shape
        per_b = m.dim() == 2
        y = torch.empty_like(x)
        _call("srn_rowln_fwd", x, m, C if per_b else 0, a, C if per_b else 0, y, B, T, C, eps)
        ctx.save_for_backward(x, m)
        ctx.eps, ctx.per_b = eps, per_b
        return y

    @staticmethod
    def backward(ctx, dy):
        x, m = ctx.saved_tensors
        B, T, C = x.shape
        dy = dy.contiguous()
        nch = (T + NORM_BWD_ROWS - 1) // NORM_BWD_ROWS
        part = torch.empty(B, nch, 2, C, device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x)
        _call("srn_rowln_bwd", x, dy, m, C if ctx.per_b else 0, dx, part, B, T, C, ctx.eps)
        if ctx.per_b:
            col = torch.empty(B, 2, C, device=x.device, dtype=torch.float32)
            _call("srn_chunk_colsum", part, None, col, None, B, nch, C, 1)
            return dx, col[:, 0].contiguous(), col[:, 1].contiguous(), None
        col = torch.empty(2, C, device=x.device, dtype=torch.float32)  # shared weights: one sum over all items' chunks
        _call("srn_chunk_colsum", part, None, col, None, 1, B * nch, C, 1)
        return dx, col[0], col[1], None


def row_ln(x, m, a, eps=1e-5):
    """y = LayerNorm_C(x) * m + a; m, a (C,) (nn.LayerNorm) or (B, C) (SpeakerAdapter, decoder.py:34-45)."""
    return _RowLN.apply(x.contiguous(), m.contiguous(), a.contiguous(), eps)


# =====================================================================================================================
#  attention core: softmax(Q K^T / sqrt(d) + key mask) V on the fused (B, L, 3 * H * d) projection
# =====================================================================================================================
class _AttnCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, lens, H):
        B, L, three = qkv.shape
        inner = three // 3
        hd = inner // H
        Lp = rup(L, 32)
        dev = qkv.device
        alloc = torch.empty if Lp == L else torch.zeros  # pad columns must read as zero
        P = alloc(B, H, L, Lp, device=dev, dtype=torch.float32)  # kept for the backward: the score buffer is all pairs
        vt = alloc(B, inner, Lp, device=dev, dtype=torch.float32)  # V^T per head: (hd, Lp) k-major
        o = torch.empty(B, L, inner, device=dev, dtype=torch.float32)
        qk, softmax, pv = attention_ops(qkv, vt, P, o, lens, B, H, hd, L, _FP32)  # one chunk: P holds every pair
        qk()
        softmax()
        _call("srn_transpose_ct", (qkv, 2 * inner), vt, B, L, inner, L * three, three, inner * Lp, Lp)
        pv()
        ctx.save_for_backward(qkv, P)
        ctx.H = H
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, P = ctx.saved_tensors
        H = ctx.H
        B, L, three = qkv.shape
        inner = three // 3
        hd = inner // H
        Lp = P.shape[-1]
        dev = qkv.device
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        # dP = dO V^T (rows of dO against rows of V: the Q K^T launch with other operands), then dS in place
        alloc = torch.empty if Lp == L else torch.zeros
        dS = alloc(B, H, L, Lp, device=dev, dtype=torch.float32)
        ConvOp(in0=do, w=(qkv, 2 * inner), out=dS, n_batch=B, n_head=H, T_in=L, T_out=L, C_in=hd, N=L,
               in0_bs=L * inner, in0_hs=hd, ld_in0=inner, w_bs=L * three, w_hs=hd, ldw=three, out_bs=H * L * Lp,
               out_hs=L * Lp, ld_out=Lp, precision=_FP32)()
        _call("srn_softmax_bwd", P, dS, B * H * L, L, Lp, 1.0 / math.sqrt(hd))
        # dQ = dS K: contraction over keys, K^T per head as the k-major operand
        kt = alloc(B, inner, Lp, device=dev, dtype=torch.float32)
        _call("srn_transpose_ct", (qkv, inner), kt, B, L, inner, L * three, three, inner * Lp, Lp)
        ConvOp(in0=dS, w=kt, out=dqkv, n_batch=B, n_head=H, T_in=L, T_out=L, C_in=Lp, N=hd, in0_bs=H * L * Lp,
               in0_hs=L * Lp, ld_in0=Lp, w_bs=inner * Lp, w_hs=hd * Lp, ldw=Lp, out_bs=L * three, out_hs=hd,
               ld_out=three, precision=_FP32)()
        # dK = dS^T Q, dV = P^T dO: contractions over query rows, one problem per (batch, head): srn_tn_gemm reads dS / P
        # (keys contiguous) and Q / dO (channels contiguous) as they lie and writes the head's slice of dqkv
        for src, rhs, col in ((dS, (qkv, 0), inner), (P, do, 2 * inner)):
            TnGemmOp(a=src, b=rhs, out=(dqkv, col), n_items=1, T_a=L, T_b=L, M=L, N=hd, lda=Lp,
                     ldb=(three if isinstance(rhs, tuple) else inner), ldc=three, n_batch=B, n_head=H,
                     a_bs=H * L * Lp, a_hs=L * Lp, b_bs=L * (three if isinstance(rhs, tuple) else inner), b_hs=hd,
                     out_bs=L * three, out_hs=hd)()
        return dqkv, None, None


def attention_core(qkv, lens, n_head):
    return _AttnCore.apply(qkv.contiguous(), lens, n_head)


# =====================================================================================================================
#  GST pieces: Conv2d(k3, s2, p1), BatchNorm2d(training) + ReLU, GRU (last state), style-token attention
# =====================================================================================================================
class _Conv2dS2(torch.autograd.Function):
    """y (B, Ho, Wo, Co) = Conv2d(k 3, stride 2, pad 1, no bias) of channels-last x (B, H, W, Cp) with the reference's
    weight (Co, Ci, 3, 3), Ci <= Cp.  srn_im2col_s2 gathers the receptive fields once ((B Ho Wo) x 9 Cp rows, padded to
    a multiple of 32 columns), then forward, dX (+ srn_col2im_s2) and dW (srn_tn_gemm) are ONE contraction each over
    all output positions -- the per-(b, ho) form of the inference path wastes its 64-row tiles once Wo <= 20."""

    @staticmethod
    def forward(ctx, x, w):
        _root._require_cuda(x, "training.conv2d_s2")
        B, H, W, Cp = x.shape
        Co, Ci = w.shape[0], w.shape[1]
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dev = x.device
        K = rup(9 * Cp, 32)
        rows = B * Ho * Wo
        col = (torch.zeros if K > 9 * Cp else torch.empty)(rows, K, device=dev, dtype=torch.float32)
        _call("srn_im2col_s2", x, col, B, H, W, Cp, K)
        wk = torch.zeros(Co, K, device=dev, dtype=torch.float32)  # [co][(kh, kw, ci)]
        wk[:, :9 * Cp].view(Co, 3, 3, Cp)[..., :Ci] = w.permute(0, 2, 3, 1)
        y = torch.empty(B, Ho, Wo, Co, device=dev, dtype=torch.float32)
        conv_op(1, col, K, rows, wk, None, y, Co, rows, [0], precision=_FP32)()
        ctx.save_for_backward(col, wk)
        ctx.dims = (B, H, W, Cp, Co, Ci, Ho, Wo, K, rows)
        return y

    @staticmethod
    def backward(ctx, dy):
        col, wk = ctx.saved_tensors
        B, H, W, Cp, Co, Ci, Ho, Wo, K, rows = ctx.dims
        dev = dy.device
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wd = torch.empty(K, Co, device=dev, dtype=torch.float32)
            _call("srn_transpose_ct", wk, wd, 1, Co, K, 0, K, 0, Co)
            dcol = torch.empty(rows, K, device=dev, dtype=torch.float32)
            conv_op(1, dy, Co, rows, wd, None, dcol, K, rows, [0], precision=_FP32)()
            dx = torch.empty(B, H, W, Cp, device=dev, dtype=torch.float32)
            _call("srn_col2im_s2", dcol, dx, B, H, W, Cp, K)
        if ctx.needs_input_grad[1]:
            dwk = torch.empty(Co, K, device=dev, dtype=torch.float32)
            TnGemmOp(a=dy, b=col, out=dwk, n_items=1, T_a=rows, T_b=rows, M=Co, N=K, lda=Co, ldb=K, ldc=K)()
            dw = dwk[:, :9 * Cp].view(Co, 3, 3, Cp)[..., :Ci].permute(0, 3, 1, 2)  # -> (Co, Ci, kh, kw)
        return dx, dw


def conv2d_s2(x, w):
    return _Conv2dS2.apply(x.contiguous(), w)


class _BnRelu(torch.autograd.Function):
    """relu(BatchNorm(x)) over the rows of channels-last x (..., C) with batch statistics; running statistics (when
    given) move like nn.BatchNorm2d's (momentum 0.1)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, eps, momentum):
        _root._require_cuda(x, "training.bn_relu")
        C = x.shape[-1]
        rows = x.numel() // C
        x = x.contiguous()
        gamma, beta = gamma.contiguous(), beta.contiguous()
        dev = x.device
        part = torch.empty(_bn_chunks(rows) * 2 * C, device=dev, dtype=torch.float32)
        stats = torch.empty(2, C, device=dev, dtype=torch.float32)
        y = torch.empty_like(x)
        _call("srn_bn_relu_fwd", x, gamma, beta, run_mean, run_var, part, stats, y, rows, C, eps, momentum)
        ctx.save_for_backward(x, y, stats, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, stats, gamma = ctx.saved_tensors
        C = x.shape[-1]
        rows = x.numel() // C
        dev = dy.device
        part = torch.empty(_bn_chunks(rows) * 2 * C, device=dev, dtype=torch.float32)
        sums = torch.empty(2, C, device=dev, dtype=torch.float32)
        dx = torch.empty_like(x)
        _call("srn_bn_relu_bwd", x, y, dy.contiguous(), stats, gamma, part, sums, dx, rows, C)
        return dx, sums[1], sums[0], None, None, None, None


def _bn_chunks(rows):
    per = 16 if rows <= 256 * 16 else (rows + 255) // 256  # srn_bn_chunks
    return (rows + per - 1) // per


def bn_relu(x, gamma, beta, run_mean=None, run_var=None, eps=1e-5, momentum=0.1):
    return _BnRelu.apply(x, gamma, beta, run_mean, run_var, eps, momentum)


class _GruLast(torch.autograd.Function):
    """last hidden state of nn.GRU (one layer, zero initial state) given gi = x W_ih^T + b_ih (B, T, 3H)."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh):
        _root._require_cuda(gi, "training.gru_last")
        B, T, G = gi.shape
        H = G // 3
        dev = gi.device
        gi, w_hh = gi.contiguous(), w_hh.contiguous()
        w_hh_t = torch.empty(H, G, device=dev, dtype=torch.float32)
        _call("srn_transpose_ct", w_hh, w_hh_t, 1, G, H, 0, H, 0, G)
        hs = torch.empty(B, T + 1, H, device=dev, dtype=torch.float32)
        gates = torch.empty(B, T, 4 * H, device=dev, dtype=torch.float32)
        _call("srn_gru_train_fwd", gi, w_hh_t, b_hh.contiguous(), hs, gates, B, T, H)
        ctx.save_for_backward(w_hh, hs, gates)
        return hs[:, T].clone()

    @staticmethod
    def backward(ctx, dh):
        w_hh, hs, gates = ctx.saved_tensors
        B, T1, H = hs.shape
        T, G = T1 - 1, 3 * H
        dev = dh.device
        dgi = torch.empty(B, T, G, device=dev, dtype=torch.float32)
        dgh = torch.empty(B, T, G, device=dev, dtype=torch.float32)
        _call("srn_gru_train_bwd", dh.contiguous(), w_hh, hs, gates, dgi, dgh, B, T, H)
        dw = torch.empty(G, H, device=dev, dtype=torch.float32)
        TnGemmOp(a=dgh, b=hs, out=dw, n_items=B, T_a=T, T_b=T, M=G, N=H, lda=G, ldb=H, ldc=H, a_is=T * G,
                 b_is=(T + 1) * H)()
        return dgi, dw, _colsum(dgh.view(B * T, G))


def gru_last(gi, w_hh, b_hh):
    return _GruLast.apply(gi, w_hh, b_hh)


class _TokenAttn(torch.autograd.Function):
    """gst/attention.py:110-184 for one query per item: q (B, F), k / v (n_tok, F) -> context (B, F)."""

    @staticmethod
    def forward(ctx, q, k, v, n_head):
        _root._require_cuda(q, "training.token_attention")
        B, Fd = q.shape
        n_tok = k.shape[0]
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        p = torch.empty(B, n_head, n_tok, device=q.device, dtype=torch.float32)
        out = torch.empty(B, Fd, device=q.device, dtype=torch.float32)
        _call("srn_token_attn_fwd", q, k, v, p, out, B, n_tok, Fd, n_head)
        ctx.save_for_backward(q, k, v, p)
        ctx.n_head = n_head
        return out

    @staticmethod
    def backward(ctx, dctx):
        q, k, v, p = ctx.saved_tensors
        B, Fd = q.shape
        n_tok = k.shape[0]
        dev = q.device
        dq = torch.empty(B, Fd, device=dev, dtype=torch.float32)
        dkp = torch.empty(B, n_tok * Fd, device=dev, dtype=torch.float32)
        dvp = torch.empty(B, n_tok * Fd, device=dev, dtype=torch.float32)
        _call("srn_token_attn_bwd", dctx.contiguous(), q, k, v, p, dq, dkp, dvp, B, n_tok, Fd, ctx.n_head)
        return dq, _colsum(dkp).view(n_tok, Fd), _colsum(dvp).view(n_tok, Fd), None


def token_attention(q, k, v, n_head):
    return _TokenAttn.apply(q, k, v, n_head)


# =====================================================================================================================
#  GEGLU
# =====================================================================================================================
class _Geglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hg):
        rows, two = hg.numel() // hg.shape[-1], hg.shape[-1]
        a = torch.empty(*hg.shape[:-1], two // 2, device=hg.device, dtype=torch.float32)
        _call("srn_geglu_fwd", hg, a, rows, two // 2)
        ctx.save_for_backward(hg)
        return a

    @staticmethod
    def backward(ctx, da):
        (hg,) = ctx.saved_tensors
        rows, two = hg.numel() // hg.shape[-1], hg.shape[-1]
        dhg = torch.empty_like(hg)
        _call("srn_geglu_bwd", hg, da.contiguous(), dhg, rows, two // 2)
        return dhg


def geglu(hg):
    """(.., 2 inner) = [h | g] -> h * gelu_erf(g)   (transformer.py:120-146)"""
    return _Geglu.apply(hg.contiguous())


# =====================================================================================================================
#  the scalar reductions of the losses
# =====================================================================================================================
class _Dot(torch.autograd.Function):
    """sum(a * b) (b None: sum(a)) through srn_dot's fp64 partial sums.  Not a torch reduction: one of this size zeroes
    its semaphore buffer with hipMemsetAsync, and a captured memset node replays with a corrupted value on this stack
    (count_memset_nodes); the <= 1024 partials are added by a single-block torch sum, which has no such node."""

    @staticmethod
    def forward(ctx, a, b):
        a = a.contiguous().view(-1)
        b = None if b is None else b.contiguous().view(-1)
        if a.data_ptr() % 16:  # srn_dot reads 16-byte pieces: a sliced view may start anywhere
            a = a.clone()
        if b is not None and b.data_ptr() % 16:
            b = b.clone()
        part = torch.zeros(1024, device=a.device, dtype=torch.float64)
        _call("srn_dot", a, b, a.numel(), part)
        ctx.save_for_backward(a, b)
        return part.sum().to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        if b is None:
            return g.expand_as(a), None
        return g * b, g * a


def _dot(a, b=None):
    """sum(a * b); sum of all elements of a without b"""
    return _Dot.apply(a.reshape(-1), None if b is None else b.reshape(-1))
