"""The model of the training step: the flat parameter store, the flow-matching estimator and its loss, the whole
`Serenade.forward` -- host logic over the autograd nodes of `functions`."""
import math

import torch
import torch.nn.functional as F

from .. import ops
from .. import training as _root  # _root._require_cuda: the guard, bound once at the package root
from ..plan import rup
from .functions import (_AddRowBias, _PackAll, _WeightNormPack, _dot, attention_core, bn_relu, conv1d, conv2d_s2, geglu,
                        gn_mish, gru_last, pack_conv, row_ln, token_attention)


# =====================================================================================================================
#  the estimator
# =====================================================================================================================
def sinusoidal_pos_emb(t, dim, scale=1000.0):
    """decoder.py:54-63 (no parameters): t (B,) -> (B, dim)"""
    half = dim // 2
    e = math.log(10000) / (half - 1)
    f = torch.exp(torch.arange(half, device=t.device, dtype=torch.float32) * -e)
    arg = scale * t.reshape(-1, 1).to(torch.float32) * f.unsqueeze(0)
    return torch.cat((arg.sin(), arg.cos()), dim=-1)


def _row_counts(m):
    """boolean length mask (B, L) -> (B,) int32 valid rows per item: the `lens` the kernels mask by"""
    return m.sum(1).to(torch.int32)


class ParamStore:
    """Trainable tensors under their state_dict names, every one a view of ONE flat fp32 buffer (`flat`) with its
    gradient a view of `flat_grad` (autograd accumulates in place): what the all-reduce and the optimizer work on.
    Tensors in `skip` (BatchNorm running statistics) are not parameters and stay out."""

    def __init__(self, state_dict, device, skip=()):
        names = [k for k in state_dict if k not in skip]
        sizes = [state_dict[k].numel() for k in names]
        offs, o = [], 0
        for n in sizes:  # 4-float alignment of every view (16-B loads in the kernels)
            offs.append(o)
            o += rup(n, 4)
        self.device = device
        self.flat = torch.zeros(o, device=device, dtype=torch.float32)
        self.flat_grad = torch.zeros(o, device=device, dtype=torch.float32)
        self.params, self.spans = {}, {}
        for k, off, n in zip(names, offs, sizes):
            v = self.flat[off:off + n].view(state_dict[k].shape)
            v.copy_(state_dict[k].to(torch.float32))
            v.requires_grad_(True)
            v.grad = self.flat_grad[off:off + n].view(state_dict[k].shape)
            self.params[k] = v
            self.spans[k] = (off, n)

    def zero_grad(self):
        self.flat_grad.zero_()

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.params.items()}

    def backward_into_flat(self, loss):
        """`flat_grad` <- d loss / d parameters, OVERWRITING it (no zero_grad needed): torch.autograd.grad + one
        multi-tensor copy (srn_multi_copy), every op on the current stream.  Used by captured steps: the per-leaf AccumulateGrad nodes of
        `loss.backward()` run on the stream the leaf was created on, and the 262 in-place adds they issue from there
        raced with the capture stream's reuse of the gradient temporaries."""
        names = list(self.params)
        ps = [self.params[k] for k in names]
        grads = torch.autograd.grad(loss, ps, allow_unused=True)
        with torch.no_grad():
            have = [(g.contiguous(), self.spans[k][0]) for k, g in zip(names, grads) if g is not None]
            # one launch per 160 tensors (torch._foreach_copy_ issues one memcpy per tensor on this stack: 245 launches)
            ops.MultiCopyOp([g for g, _ in have], [o for _, o in have], self.flat_grad)()
            for p, g in zip(ps, grads):
                if g is None:
                    p.grad.zero_()


class Estimator:
    """`Decoder` (matcha_components/decoder.py:196-467) for training: parameters under the reference's names and
    shapes (`self.params`), each a view of the flat buffer `self.flat`; gradients are views of `self.flat_grad`.

    `forward(x, mask, mu, t, spks)` takes the reference's layouts -- x (B, out_ch, L), mask (B, 1, L), mu (B, cond, L),
    t (B,), spks (B, S) -- and returns (B, out_ch, L) with an autograd graph whose backward runs on the HIP kernels."""

    N_HEAD, GROUPS = 4, 8

    def __init__(self, state_dict, device, dropout=0.0, _store=None, _prefix=""):
        """state_dict: the estimator's tensors under the reference's names.  dropout: probability of the two Dropout
        layers of every transformer block (attention output, feed-forward; decoder.py:215 trains with 0.05) -- torch's
        generator, so not reproducible against the reference's draws; parity tests use 0."""
        if _store is None:
            _store = ParamStore(state_dict, device)
        self.store = _store
        self.flat, self.flat_grad, self.device = _store.flat, _store.flat_grad, _store.device
        n = len(_prefix)
        self.params = {k[n:]: v for k, v in _store.params.items() if k.startswith(_prefix)}
        self.spans = {k[n:]: v for k, v in _store.spans.items() if k.startswith(_prefix)}
        self.dropout = float(dropout)
        names = list(self.params)
        self.n_down = sum(1 for k in names if k.startswith("down_blocks.") and k.endswith(".0.mlp.1.weight"))
        self.n_mid = sum(1 for k in names if k.startswith("mid_blocks.") and k.endswith(".0.mlp.1.weight"))
        self.n_up = sum(1 for k in names if k.startswith("up_blocks.") and k.endswith(".0.mlp.1.weight"))
        self._plan_relay()

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.params.items()}

    def zero_grad(self):
        self.flat_grad.zero_()

    def _plan_relay(self):
        """What every step re-lays of the weights, planned once: conv weights (N, C, k) -> packed (N, k * C_pad)
        (`self._pk`, the differentiable outputs of _PackAll) and, for every conv / linear, W^T for the input gradient
        (`self._wd[name]`: (C_pad, k * N); q | k | v side by side for the fused projection).  Buffers are allocated here
        (pad columns stay zero) and the transposes are two prebuilt srn_transpose_multi tables: parameters first, then
        the transposes that read the packed buffers."""
        P, dev = self.params, self.device
        z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self._pk, self._wd, self._pack_names, self._relay_ops = {}, {}, [], []
        if "down_blocks.0.0.block1.block.0.weight" not in P:
            return  # not a decoder's state_dict (GradSync's unit tests hand a bare ParamStore): nothing to re-lay
        cin0 = P["down_blocks.0.0.block1.block.0.weight"].shape[1]
        first, second = [], []
        for name, w in P.items():
            if not name.endswith(".weight") or w.dim() not in (2, 3):
                continue
            if name.startswith("up_blocks.") and name.endswith("2.conv.weight"):
                continue  # ConvTranspose1d: re-laid per output phase by ops.convtranspose_phases
            if name.startswith("time_mlp.linear_1"):
                continue  # its input is padded on the fly (242 -> 244 columns)
            if any(t in name for t in (".to_q.", ".to_k.", ".to_v.")):
                continue  # the fused projection, below
            if w.dim() == 2 and w.shape[0] * w.shape[1] >= 64:
                n, c = w.shape
                if ".norm" in name:
                    continue
                self._wd[name] = z(c, n)
                first.append((w, self._wd[name], 1, n, c, 0, c, 0, n))
            elif w.dim() == 3:
                n, c, k = w.shape
                c_pad = rup(c, 32) if name.startswith("down_blocks.0.0.") and c == cin0 else c
                self._wd[name] = z(c_pad, k * n)
                if k == 1 and c_pad == c:  # pack_conv is a view
                    first.append((w, self._wd[name], 1, n, c, 0, c, 0, n))
                    continue
                self._pk[name] = z(n, k * c_pad)
                self._pack_names.append(name)
                first.append((w, self._pk[name], n, c, k, c * k, k, k * c_pad, c_pad))
                second.append((self._pk[name], self._wd[name], k, n, c_pad, c_pad, k * c_pad, n, k * n))
        for name in [k for k in P if k.endswith("attn1.to_q.weight")]:
            pre = name[:-len("to_q.weight")]
            ws = [P[pre + t + ".weight"] for t in ("to_q", "to_k", "to_v")]
            inner, c = ws[0].shape
            wd = z(c, 3 * inner)
            self._wd[pre + "qkv"] = wd
            for i, w in enumerate(ws):
                first.append((w, (wd, i * inner), 1, inner, c, 0, c, 0, 3 * inner))
        self._relay_ops = [ops.TransposeMultiOp(first), ops.TransposeMultiOp(second)]

    def _relay(self):
        """once per forward: packed conv weights (differentiable) + the input-gradient layouts (constants of the step)"""
        packed = _PackAll.apply(self, *[self.params[n] for n in self._pack_names])
        self._pkd = dict(zip(self._pack_names, packed))

    def _packed(self, name, c_pad=None):
        w = self._pkd.get(name)
        return w if w is not None else pack_conv(self.params[name], c_pad)

    def _drop(self, x):
        return F.dropout(x, self.dropout, True) if self.dropout > 0.0 else x

    # ---- blocks ------------------------------------------------------------------------------------------------
    def _lin(self, x, name, bias=True, c_pad=None):
        w = self.params[name + ".weight"]
        if c_pad is not None and c_pad > w.shape[1]:
            w = F.pad(w, (0, c_pad - w.shape[1]))
        wd = self._wd.get(name + ".weight") if c_pad is None else None
        return conv1d(x, w, self.params[name + ".bias"] if bias else None, wd=wd)

    def _block1d(self, p, x, lens, c_pad=None):
        """Block1D (decoder.py:66-77): conv k3 of the masked input -> GroupNorm(8) -> Mish -> mask"""
        w = self._packed(p + "block.0.weight", c_pad)
        h, part = conv1d(x, w, self.params[p + "block.0.bias"], ops.conv_taps(3), want_gn=True, lens=lens,
                         wd=self._wd.get(p + "block.0.weight"))
        return gn_mish(h, part, self.params[p + "block.1.weight"], self.params[p + "block.1.bias"], lens, self.GROUPS)

    def _resnet(self, p, x, lens, temb, spk, c_pad=None):
        """ResnetBlock1D (decoder.py:80-101) + SpeakerAdapter (decoder.py:23-45)"""
        h = self._block1d(p + "block1.", x, lens, c_pad)
        h = _AddRowBias.apply(h, self._lin(F.mish(temb), p + "mlp.1"))
        h = self._block1d(p + "block2.", h, lens)
        out = h + conv1d(x, self._packed(p + "res_conv.weight", c_pad), self.params[p + "res_conv.bias"], lens=lens,
                         wd=self._wd.get(p + "res_conv.weight"))
        scale = self._lin(spk, p + "speaker_projection.W_scale")
        shift = self._lin(spk, p + "speaker_projection.W_bias")
        return row_ln(out, scale, shift)

    def _tfm(self, p, x, lens):
        """BasicTransformerBlock effective path (transformer.py:286-352): LN -> self-attention -> +x -> LN -> GEGLU FF
        -> +x; dropout not applied (see module docstring)"""
        P = self.params
        n = row_ln(x, P[p + "norm1.weight"], P[p + "norm1.bias"])
        wqkv = torch.cat([P[p + "attn1.to_q.weight"], P[p + "attn1.to_k.weight"], P[p + "attn1.to_v.weight"]], dim=0)
        o = attention_core(conv1d(n, wqkv, None, wd=self._wd.get(p + "attn1.qkv")), lens, self.N_HEAD)
        x = self._drop(self._lin(o, p + "attn1.to_out.0")) + x
        n = row_ln(x, P[p + "norm3.weight"], P[p + "norm3.bias"])
        a = self._drop(geglu(self._lin(n, p + "ff.net.0.proj")))
        return self._lin(a, p + "ff.net.2") + x

    def forward(self, x, mask, mu, t, spks):
        _root._require_cuda(x, "Estimator.forward")
        P = self.params
        self._relay()
        B, _, L = x.shape
        maskb = mask.reshape(B, L) > 0
        if not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            # the reference's `x * mask` is done by row counts here (len_in / len_out / len_b of the kernels): that equals
            # the multiply only for a LENGTH mask -- anything else would silently change activations and gradients
            if not torch.equal(maskb, torch.arange(L, device=x.device)[None] < maskb.sum(1, keepdim=True)):
                raise ValueError("Estimator.forward: `mask` must be a length (prefix) mask, as make_non_pad_mask builds it")
        h = torch.cat([x, mu], dim=1).transpose(1, 2)  # (B, L, 242) channels-last
        cin = h.shape[-1]
        cp = rup(cin, 32)
        h = F.pad(h, (0, cp - cin)).contiguous()
        t = torch.as_tensor(t, device=x.device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(B)
        s = sinusoidal_pos_emb(t, cin)
        s = F.pad(s, (0, rup(cin, 4) - cin))
        temb = self._lin(F.silu(self._lin(s, "time_mlp.linear_1", c_pad=s.shape[1])), "time_mlp.linear_2")
        spk = spks.to(torch.float32)

        masks = [maskb]
        hiddens = []
        for i in range(self.n_down):
            p = f"down_blocks.{i}."
            m = masks[-1]
            lens = _row_counts(m)
            h = self._resnet(p + "0.", h, lens, temb, spk, c_pad=cp if i == 0 else None)
            h = self._tfm(p + "1.0.", h, lens)
            hiddens.append(h)
            if p + "2.conv.weight" in P:  # conv1d's `lens` is stride-1 only: the one mask multiply that is left
                h = conv1d(h * m.unsqueeze(-1).to(torch.float32), self._packed(p + "2.conv.weight"),
                           P[p + "2.conv.bias"], ops.conv_taps(3), stride=2, wd=self._wd.get(p + "2.conv.weight"))
            else:
                h = conv1d(h, self._packed(p + "2.weight"), P[p + "2.bias"], ops.conv_taps(3), lens=lens,
                           wd=self._wd.get(p + "2.weight"))
            masks.append(m[:, ::2])
        masks = masks[:-1]
        lens = _row_counts(masks[-1])
        for i in range(self.n_mid):
            p = f"mid_blocks.{i}."
            h = self._resnet(p + "0.", h, lens, temb, spk)
            h = self._tfm(p + "1.0.", h, lens)
        for i in range(self.n_up):
            p = f"up_blocks.{i}."
            lens = _row_counts(masks.pop())
            skip = hiddens.pop()
            h = torch.cat([h[:, :skip.shape[1]], skip], dim=-1)
            h = self._resnet(p + "0.", h, lens, temb, spk)
            h = self._tfm(p + "1.0.", h, lens)
            if p + "2.conv.weight" in P:
                # ConvTranspose1d(k 4, stride 2, padding 1): two output phases, each a 2-tap conv of the input
                ys = []
                for taps, wp in ops.convtranspose_phases(P[p + "2.conv.weight"], 2, 1):
                    ys.append(conv1d(h, wp, P[p + "2.conv.bias"], taps, lens=lens))
                h = torch.stack(ys, dim=2).reshape(B, -1, ys[0].shape[-1])
            else:
                h = conv1d(h, self._packed(p + "2.weight"), P[p + "2.bias"], ops.conv_taps(3), lens=lens,
                           wd=self._wd.get(p + "2.weight"))
        h = self._block1d("final_block.", h, lens)
        out = conv1d(h, self._packed("final_proj.weight"), P["final_proj.bias"], lens=lens,
                     wd=self._wd.get("final_proj.weight"))
        return (out * maskb.unsqueeze(-1).to(torch.float32)).transpose(1, 2)

    __call__ = forward


def cfm_loss(estimator, x1, mask, mu, spks, mask_l=None, draws=None, sigma_min=1e-4):
    """CFM.compute_loss (flow_matching.py:95-133) with autograd through `estimator`.  `draws` = {"t": (B,1,1),
    "z": like x1} fixes the random draws (parity tests); otherwise torch.rand / randn_like as in the reference."""
    b = mu.shape[0]
    if draws is None:
        t = torch.rand([b, 1, 1], device=mu.device, dtype=mu.dtype)
        z = torch.randn_like(x1)
    else:
        t, z = draws["t"].to(x1), draws["z"].to(x1)
    y = (1 - (1 - sigma_min) * t) * z + t * x1
    u = x1 - (1 - sigma_min) * z
    den = estimator(y, mask, mu, t.reshape(-1), spks)
    if mask_l is not None:
        den = den * mask_l
        u = u * mask_l
    d = (den - u).reshape(-1)
    loss = _dot(d, d)  # F.mse_loss(den, u, reduction="sum")
    denom = _dot(mask_l if mask_l is not None else mask.to(d.dtype))
    return loss / (denom * u.shape[1]), y


# =====================================================================================================================
#  the whole model: Serenade.forward (serenade.py:90-166) for training
# =====================================================================================================================
_REFLECT_IDX = {}


def _reflect_pad_rows(x, p):
    """nn.ReflectionPad1d(p) along time of a channels-last (B, T, C) tensor (a gather: autograd scatters back)"""
    T = x.shape[1]
    d = x.device  # built on the device: a captured step may not copy from the host
    key = (T, p, str(d))
    idx = _REFLECT_IDX.get(key)
    if idx is None:  # once per (length, pad): three aranges + a cat per call otherwise, five calls per step
        idx = _REFLECT_IDX[key] = torch.cat([torch.arange(p, 0, -1, device=d), torch.arange(T, device=d),
                                             torch.arange(T - 2, T - 2 - p, -1, device=d)])
    return x.index_select(1, idx)


class TrainSerenade:
    """`Serenade` (serenade/models/serenade.py:35-166) for training: all trainable tensors of the checkpoint in one
    `ParamStore`; `forward` returns {"gauss_mel", "prior_loss", "cfm_loss"} with an autograd graph.

      * estimator: `Estimator` above (HIP forward and backward);
      * content encoder `Conv1dResnet` (serenade.py:282-296,310-376): weight norm folded straight into the packed
        layouts by srn_weight_norm_fwd / _bwd (`_WeightNormPack`), reflection padding as a row gather, every conv through `conv1d` (HIP forward, dgrad and wgrad), LeakyReLU in torch;
      * GST style encoder (modules/gst/style_encoder.py): six 3x3 stride-2 Conv2d + train-mode BatchNorm2d + ReLU, a
        GRU over T_ref / 64 steps and the 50-token attention -- 0.8 GFLOP of the step's ~1.3 TFLOP -- run on the
        project's own kernels in both directions (`gst` below).
    BatchNorm running statistics are updated like nn.BatchNorm2d (momentum 0.1) in `self.buffers`."""

    def __init__(self, state_dict, device, dropout=0.05, mask_size=(0.1, 0.5), output_dim=80):
        skip = [k for k in state_dict if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
        self.store = ParamStore(state_dict, device, skip=skip)
        self.buffers = {k: state_dict[k].to(device).clone() for k in skip}
        self.flat, self.flat_grad, self.device = self.store.flat, self.store.flat_grad, device
        self.params, self.spans = self.store.params, self.store.spans
        self.estimator = Estimator(None, device, dropout=dropout, _store=self.store, _prefix="cfm_decoder.estimator.")
        self.mask_size, self.output_dim, self.training = tuple(mask_size), output_dim, True

    def zero_grad(self):
        self.store.zero_grad()

    def backward(self, loss, sync=None):
        """gradients of `loss` into the flat buffer, all-reduced if `sync` spans several ranks.  With a GradSync that
        overlaps: zero_grad() + `loss.backward()`, whose per-parameter hooks launch the bucketed all-reduce while
        backward is still running, + sync.finish().  Otherwise one `torch.autograd.grad` + one multi-tensor copy that
        OVERWRITES the buffer -- no zero fill, none of the 262 per-parameter accumulation kernels -- then sync.finish()."""
        if sync is not None and sync._hooks:
            self.zero_grad()
            loss.backward()
        else:
            self.store.backward_into_flat(loss)
        if sync is not None:
            sync.finish()

    def state_dict(self):
        sd = self.store.state_dict()
        sd.update({k: v.clone() for k, v in self.buffers.items()})
        return sd

    # ---- content encoder -----------------------------------------------------------------------------------------
    def _wn(self, name):
        """(packed weight, W^T for the input gradient or None) of an encoder conv: weight-normed ones through the fused
        kernel, plain ones through pack_conv"""
        P = self.params
        if name + ".weight" in P:
            return pack_conv(P[name + ".weight"]), None
        return _WeightNormPack.apply(P[name + ".weight_v"], P[name + ".weight_g"])

    def encoder(self, x):
        """(B, T, in_dim) -> (B, T, out_dim); like the reference, padded frames are not masked here"""
        P, T = self.params, x.shape[1]
        e = "encoder.model."
        w, wd = self._wn(e + "1")
        h = conv1d(_reflect_pad_rows(x.contiguous(), 3), w, P[e + "1.bias"], range(7), T_out=T, wd=wd)
        n = 0
        while f"{e}{2 + n}.shortcut.bias" in P:
            p, d = f"{e}{2 + n}", 2 ** n
            w, wd = self._wn(p + ".shortcut")
            sc = conv1d(h, w, P[p + ".shortcut.bias"], wd=wd)
            w, wd = self._wn(p + ".block.2")
            b = conv1d(_reflect_pad_rows(F.leaky_relu(h, 0.2), d), w, P[p + ".block.2.bias"], [0, d, 2 * d], T_out=T, wd=wd)
            w, wd = self._wn(p + ".block.4")
            b = conv1d(F.leaky_relu(b, 0.2), w, P[p + ".block.4.bias"], wd=wd)
            h = sc + b
            n += 1
        last = f"{e}{2 + n + 2}"
        w, wd = self._wn(last)
        return conv1d(_reflect_pad_rows(F.leaky_relu(h, 0.2), 3), w, P[last + ".bias"], range(7), T_out=T, wd=wd)

    # ---- GST -------------------------------------------------------------------------------------------------------
    def gst(self, speech, n_head=4):
        """StyleEncoder.forward (style_encoder.py:78-91,171-191,235-252), channels-last, own kernels in both directions:
        Conv2d(k3, s2, p1) as one stride-2 three-tap contraction along the mel axis per kernel row (srn_conv_gemm forward
        and dgrad, srn_tn_gemm wgrad), BatchNorm2d(training) + ReLU (srn_bn_relu_*), the GRU's input projection as a
        linear + srn_gru_train_* for the recurrence / BPTT, the token attention's four linears + srn_token_attn_*."""
        P, Bf = self.params, self.buffers
        r = "gst.ref_enc."
        B, T, F0 = speech.shape
        h = F.pad(speech.to(torch.float32).unsqueeze(-1), (0, 3))  # (B, H = T, W = 80, C = 1 padded to 4)
        i = 0
        while f"{r}convs.{3 * i}.weight" in P:
            c, b = f"{r}convs.{3 * i}", f"{r}convs.{3 * i + 1}"
            h = conv2d_s2(h, P[c + ".weight"])
            if self.training:
                h = bn_relu(h, P[b + ".weight"], P[b + ".bias"], Bf[b + ".running_mean"], Bf[b + ".running_var"])
                if b + ".num_batches_tracked" in Bf:
                    Bf[b + ".num_batches_tracked"] += 1
            else:
                # eval mode (the reference's _eval_epoch, trainers/base.py:171-190): BatchNorm2d on the running
                # statistics, folded into one scale / shift per channel (channels last), then ReLU
                scale = P[b + ".weight"] * torch.rsqrt(Bf[b + ".running_var"] + 1e-5)
                h = torch.relu(h * scale + (P[b + ".bias"] - Bf[b + ".running_mean"] * scale))
            i += 1
        bsz, tlen, wdim, cdim = h.shape
        xs = h.reshape(bsz, tlen, wdim * cdim)  # features ordered (w, c); the reference's view orders them (c, w)
        wih, whh = P[r + "gru.weight_ih_l0"], P[r + "gru.weight_hh_l0"]
        wih = wih.view(-1, cdim, wdim).permute(0, 2, 1).reshape(wih.shape[0], -1)
        gi = conv1d(xs, wih, P[r + "gru.bias_ih_l0"])
        hh = gru_last(gi, whh, P[r + "gru.bias_hh_l0"])
        m = "gst.stl.mha."
        toks = torch.tanh(P["gst.stl.gst_embs"])
        q = conv1d(hh, P[m + "linear_q.weight"], P[m + "linear_q.bias"])
        k = conv1d(F.pad(toks, (0, (-toks.shape[1]) % 4)), F.pad(P[m + "linear_k.weight"], (0, (-toks.shape[1]) % 4)),
                   P[m + "linear_k.bias"])
        v = conv1d(F.pad(toks, (0, (-toks.shape[1]) % 4)), F.pad(P[m + "linear_v.weight"], (0, (-toks.shape[1]) % 4)),
                   P[m + "linear_v.bias"])
        ctx = token_attention(q, k, v, n_head)
        return conv1d(ctx, P[m + "linear_out.weight"], P[m + "linear_out.bias"])

    def draw_segment(self, T):
        """(seg_start, seg_len) of the infill segment, drawn like serenade.py:117-119 (python `random`)"""
        import random
        msize = int(random.uniform(*self.mask_size) * T)
        return random.randint(0, T - msize), msize

    # ---- Serenade.forward ----------------------------------------------------------------------------------------
    def forward(self, x, lengths, logmel, midi, lft, draws=None):
        """serenade.py:90-166.  `draws` (tests) = {"uniform", "seg_start", "t", "z"} replaces the random draws."""
        import random
        _root._require_cuda(x, "TrainSerenade.forward")
        ret = {}
        enc = self.encoder(x.to(torch.float32))
        ret["gauss_mel"] = enc
        spk = self.gst(logmel)
        B, T = enc.shape[0], enc.shape[1]
        mask = (torch.arange(T, device=x.device)[None] < torch.as_tensor(lengths, device=x.device)[:, None])
        mask = mask.unsqueeze(1).to(torch.float32)
        if draws is not None and "seg" in draws:  # device tensor [seg_start, seg_len] (a captured step replays it)
            s0, msize = draws["seg"][0], draws["seg"][1]
        else:
            uni = random.uniform(*self.mask_size) if draws is None else float(draws["uniform"])
            msize = int(uni * T)
            s0 = random.randint(0, T - msize) if draws is None else int(draws["seg_start"])
        idx = torch.arange(T, device=x.device)
        inside = ((idx >= s0) & (idx < s0 + msize)).to(torch.float32).view(1, 1, T)
        mask_l = mask * inside
        mask_c = mask * (1.0 - inside)
        # sum(0.5 * ((logmel - enc)^2 + log 2 pi) * mask) over (B, out, T), written with dot products (see _Dot)
        diff = (logmel - enc).reshape(-1)
        n_valid = _dot(mask)
        prior = 0.5 * _dot(diff * mask.permute(0, 2, 1).expand(B, T, self.output_dim).reshape(-1), diff) \
            + 0.5 * math.log(2 * math.pi) * self.output_dim * n_valid
        ret["prior_loss"] = prior / (n_valid * self.output_dim)
        targets = logmel * mask_l.permute(0, 2, 1)
        cond = logmel * mask_c.permute(0, 2, 1)
        mu = torch.cat([enc, midi, lft, cond], dim=-1)
        tz = None if draws is None or "t" not in draws else {"t": draws["t"], "z": draws["z"]}
        ret["cfm_loss"], _ = cfm_loss(self.estimator, targets.permute(0, 2, 1), mask, mu.permute(0, 2, 1), spk, mask_l,
                                      draws=tz)
        return ret

    __call__ = forward
