"""HIP-backed mirror of ``serenade.models`` for the audio-infilling inference hot path.

Same class names, constructor kwargs, ``forward()/inference()`` signatures and ``state_dict``
layout as the reference, so ``getattr(models, config["model_type"])
(**config["model_params"])`` + ``load_state_dict(torch.load(ckpt)["model"])`` works unchanged:

    Serenade        serenade/models/serenade.py:35-221
    Conv1dResnet    serenade/models/serenade.py:224-356
    StyleEncoder    serenade/modules/gst/style_encoder.py:16-91
    CFM             serenade/models/matcha_components/flow_matching.py:9-93
    Decoder         serenade/models/matcha_components/decoder.py:208-467

The modules are weight containers plus *plans*: lists of prebuilt C-ABI calls (``ops.ConvOp`` /
``ops.CallOp``) over preallocated channels-last HBM buffers.  All arithmetic runs in
libserenade_hip.so; torch is used for device memory, streams and the one-time weight packing.
There is no CPU path: calling these modules with CPU tensors raises.
"""
import functools
import math

import torch
import torch.nn as nn

from . import _shapes, ops
from .ops import ACT_LEAKY, ACT_MISH, ACT_SILU, RES_ADD, RES_AXPY, ConvOp
from .plan import (StridedLengthTable, attention_ops, attention_scores, conv_op, dev_f32, item_lengths, linear_op,
                   lru_get, rup, tensors_of)
from .plan import require_cuda as _require_cuda
from .utils.masking import make_non_pad_mask

__all__ = ["Serenade", "Conv1dResnet", "StyleEncoder", "CFM", "Decoder", "serenade_state_shapes"]


def serenade_state_shapes(**params):
    return _shapes.as_meta(_shapes.serenade_shapes(**params))


class _Packed(nn.Module):
    """Base: parameter tree with the reference's names + lazily packed device weights."""

    def __init__(self, shapes):
        super().__init__()
        tree = _shapes.ParamTree(shapes)
        for name, child in tree.named_children():
            self.add_module(name, child)
        for name, p in tree._parameters.items():
            self.register_parameter(name, p)
        self._packed = None
        self._plans = {}

    def _invalidate(self):
        if self._packed is not None:
            ops.drop_weight_planes(tensors_of(self._packed))
        self._packed = None
        self._plans = {}
        for m in self.children():
            if isinstance(m, _Packed):
                m._invalidate()

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._invalidate()
        return r

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._invalidate()
        return r

    def _own_state(self):
        """state of this module only (no _Packed children), keys relative to it"""
        return {k: v.detach() for k, v in self.state_dict().items()}

    def _device(self):
        for p in self.parameters():
            return p.device
        return torch.device("cpu")


def _fold_wn(sd, name):
    """weight_norm fold (serenade.py:359-360): w = g * v / ||v||  over dims != 0."""
    if name + ".weight" in sd:
        return sd[name + ".weight"]
    g, v = sd[name + ".weight_g"], sd[name + ".weight_v"]
    norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
    return v * (g / norm)


# =====================================================================================
#  Decoder (the UNet estimator) and its Euler plan
# =====================================================================================
class Decoder(_Packed):
    """1-D UNet estimator, matcha_components/decoder.py:208-467.

    ``forward(x, mask, mu, t, speaker_features)`` keeps the reference signature and layouts
    ((B, C, T) tensors, mask (B, 1, T)); internally everything is channels-last.
    The mask must be a prefix mask (as produced by ``make_non_pad_mask``)."""

    def __init__(self, in_channels, out_channels, spk_embed_dim, channels=(512, 512), dropout=0.05,
                 attention_head_dim=512, n_blocks=1, num_mid_blocks=2, num_heads=4, act_fn="snake",
                 down_block_type="transformer", mid_block_type="transformer", up_block_type="transformer"):
        channels = tuple(channels)
        super().__init__(_shapes.decoder_shapes(in_channels, out_channels, spk_embed_dim, channels,
                                                attention_head_dim, n_blocks, num_mid_blocks, num_heads))
        self.in_channels, self.out_channels, self.spk_embed_dim = in_channels, out_channels, spk_embed_dim
        self.channels, self.num_mid_blocks = channels, num_mid_blocks
        self.num_heads, self.head_dim = num_heads, attention_head_dim
        for c in channels:
            assert c % 256 == 0 and c <= 1024, "GroupNorm(8) tiles need channels % 256 == 0"

    # ------------------------------------------------------------------ packing
    def _block_names(self):
        D = len(self.channels)
        return ([f"down_blocks.{i}" for i in range(D)] + [f"mid_blocks.{i}" for i in range(self.num_mid_blocks)] +
                [f"up_blocks.{i}" for i in range(D)])

    def packed(self):
        if self._packed is not None:
            return self._packed
        dev = self._device()
        sd = {k: dev_f32(v, dev) for k, v in self._own_state().items()}
        P = {}
        cp0 = rup(self.in_channels, 32)
        P["cp0"] = cp0
        l1 = sd["time_mlp.linear_1.weight"]
        w = l1.new_zeros(l1.shape[0], cp0)
        w[:, : l1.shape[1]] = l1
        P["t1_w"], P["t1_b"] = w, sd["time_mlp.linear_1.bias"]
        P["t2_w"], P["t2_b"] = sd["time_mlp.linear_2.weight"], sd["time_mlp.linear_2.bias"]
        names = self._block_names()
        P["tb_w"] = torch.cat([sd[b + ".0.mlp.1.weight"] for b in names]).contiguous()
        P["tb_b"] = torch.cat([sd[b + ".0.mlp.1.bias"] for b in names]).contiguous()
        sp_w, sp_b = [], []
        for b in names:
            for nm in ("W_scale", "W_bias"):
                sp_w.append(sd[f"{b}.0.speaker_projection.{nm}.weight"])
                sp_b.append(sd[f"{b}.0.speaker_projection.{nm}.bias"])
        P["spk_w"], P["spk_b"] = torch.cat(sp_w).contiguous(), torch.cat(sp_b).contiguous()
        P["res"], P["tfm"] = [], []
        for b in names:
            r = b + ".0."
            cin = sd[r + "block1.block.0.weight"].shape[1]
            cpad = cp0 if cin == self.in_channels else cin
            P["res"].append(dict(
                cin=cpad, cout=sd[r + "block1.block.0.weight"].shape[0],
                c1_w=ops.pack_conv_weight(sd[r + "block1.block.0.weight"], cpad), c1_b=sd[r + "block1.block.0.bias"],
                g1_w=sd[r + "block1.block.1.weight"], g1_b=sd[r + "block1.block.1.bias"],
                c2_w=ops.pack_conv_weight(sd[r + "block2.block.0.weight"]), c2_b=sd[r + "block2.block.0.bias"],
                g2_w=sd[r + "block2.block.1.weight"], g2_b=sd[r + "block2.block.1.bias"],
                r_w=ops.pack_conv_weight(sd[r + "res_conv.weight"], cpad), r_b=sd[r + "res_conv.bias"]))
            t = b + ".1.0."
            f1w, f1b = ops.pack_geglu(sd[t + "ff.net.0.proj.weight"], sd[t + "ff.net.0.proj.bias"])
            P["tfm"].append(dict(
                ln1_w=sd[t + "norm1.weight"], ln1_b=sd[t + "norm1.bias"],
                qkv_w=torch.cat([sd[t + "attn1.to_q.weight"], sd[t + "attn1.to_k.weight"],
                                 sd[t + "attn1.to_v.weight"]]).contiguous(),
                o_w=sd[t + "attn1.to_out.0.weight"], o_b=sd[t + "attn1.to_out.0.bias"],
                ln3_w=sd[t + "norm3.weight"], ln3_b=sd[t + "norm3.bias"],
                ff1_w=f1w, ff1_b=f1b, ff2_w=sd[t + "ff.net.2.weight"], ff2_b=sd[t + "ff.net.2.bias"]))
        D = len(self.channels)
        P["down"], P["up"] = [], []
        for i in range(D):
            p = f"down_blocks.{i}.2"
            if i < D - 1:
                P["down"].append(dict(stride=2, w=ops.pack_conv_weight(sd[p + ".conv.weight"]), b=sd[p + ".conv.bias"]))
            else:
                P["down"].append(dict(stride=1, w=ops.pack_conv_weight(sd[p + ".weight"]), b=sd[p + ".bias"]))
        for i in range(D):
            p = f"up_blocks.{i}.2"
            if i < D - 1:
                P["up"].append(dict(transpose=True, phases=ops.convtranspose_phases(sd[p + ".conv.weight"], 2, 1),
                                    b=sd[p + ".conv.bias"]))
            else:
                P["up"].append(dict(transpose=False, w=ops.pack_conv_weight(sd[p + ".weight"]), b=sd[p + ".bias"]))
        P["fb_w"] = ops.pack_conv_weight(sd["final_block.block.0.weight"])
        P["fb_b"] = sd["final_block.block.0.bias"]
        P["fg_w"], P["fg_b"] = sd["final_block.block.1.weight"], sd["final_block.block.1.bias"]
        P["fp_w"] = ops.pack_conv_weight(sd["final_proj.weight"])
        P["fp_b"] = sd["final_proj.bias"]
        self._packed = P
        return P

    def plan(self, B, L, n_steps, euler, per_sample_t=False, exact_ragged=False):
        key = (B, L, n_steps, bool(euler), bool(per_sample_t), bool(exact_ragged), ops.DEFAULT_PRECISION,
               ops.attention_precision())
        return lru_get(self._plans, key, 8,
                        lambda: DecoderPlan(self, B, L, n_steps, euler, per_sample_t, exact_ragged))

    @torch.no_grad()
    def forward(self, x, mask, mu, t, speaker_features):
        """decoder.py:384-467.  x (B, out_ch, L), mask (B, 1, L), mu (B, cond, L), spk (B, S);
        t is 0-dim (one time for the batch, as solve_euler passes it) or (B,) (one per sample, as
        CFM.compute_loss passes it)."""
        _require_cuda(x, "Decoder.forward")
        B, _, L = x.shape
        t = torch.as_tensor(t)
        per_sample = t.ndim >= 1 and t.numel() == B and B > 1
        pl = self.plan(B, L, 1, euler=False, per_sample_t=per_sample)
        lens = mask.reshape(B, -1).to(torch.int64).sum(dim=1)
        ts = [float(v) for v in t.reshape(-1).tolist()] if per_sample else [float(t.reshape(-1)[0])]
        pl.set_inputs(x, mu, speaker_features, lens, ts=ts)
        pl.run()
        return pl.read_out()


class DecoderPlan:
    """Preallocated buffers + the op list of `n_steps` estimator calls for one (B, L).

    euler=True : step k ends with the fused Euler update x += dt_k * (final_proj(...) * mask)
                 (flow_matching.py:84-91), written in place into channels [0, out_ch) of h0.
    euler=False: one estimator call, output (B, L, out_ch) in ``self.dphi``."""

    def __init__(self, dec, B, L, n_steps, euler, per_sample_t=False, exact_ragged=False):
        # exact_ragged: every item of a padded batch gets the result of its own B = 1 run.  The one op of the estimator
        # whose result depends on an item's padding is GroupNorm (the reference normalises over the padded length,
        # decoder.py:71-77); here the convs that feed a GroupNorm zero their padded rows (len_out), so those add nothing
        # to the partial sums, and the statistics are divided by the item's own length (valid_stats).
        rg = bool(exact_ragged)
        self.exact_ragged = rg
        P = dec.packed()
        dev = dec._device()
        # per_sample_t: ONE estimator call whose time embedding has one row per batch item
        # (CFM.compute_loss draws t per sample, flow_matching.py:116,123); otherwise one row per Euler step.
        self.per_sample_t = bool(per_sample_t)
        n_iter = 1 if per_sample_t else n_steps
        n_steps = B if per_sample_t else n_steps  # rows of the time-embedding buffers below
        self.n_rows = n_steps
        self.dec, self.B, self.L, self.n, self.euler = dec, B, L, n_iter, euler
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        D = len(dec.channels)
        Ts = [L]
        for _ in range(D - 1):
            Ts.append((Ts[-1] + 1) // 2)
        self.Ts = Ts
        Cmax = max(dec.channels)
        cp0, oc = P["cp0"], dec.out_channels
        H, hd = dec.num_heads, dec.head_dim
        inner = H * hd
        names = dec._block_names()
        nb = len(names)
        # ---- buffers
        self.lens = [torch.zeros(B, device=dev, dtype=torch.int32) for _ in Ts]
        self.h0 = f(B, L, cp0)
        self.t_dev = f(n_steps)
        self.sin = f(n_steps, cp0)
        self.e1 = f(n_steps, P["t1_w"].shape[0])
        self.temb = f(n_steps, P["t2_w"].shape[0])
        self.tb = f(n_steps, P["tb_w"].shape[0])
        self.spk = f(B, dec.spk_embed_dim)
        self.ss = f(B, P["spk_w"].shape[0])
        bufX, bufY = f(B, L, Cmax), f(B, L, Cmax)
        bufC, bufA, bufR = f(B, L, Cmax), f(B, L, Cmax), f(B, L, Cmax)
        bufN = f(B, L, Cmax)
        qkv = f(B, L, 3 * inner)
        self.S = S = attention_scores(B, H, L, dev)  # one bounded buffer for every resolution (tools/footprint.py)
        # V^T per resolution, (B, inner, rup(T, 32)): P.V then contracts k-major rows like every other GEMM.  The pad
        # columns are never written (zeros from allocation) and meet exact zeros of the softmax.
        Vt = {T: f(B, inner, rup(T, 32)) for T in sorted(set(Ts))}
        bufO = f(B, L, inner)
        ffh = max(t["ff2_w"].shape[1] for t in P["tfm"])
        bufG = f(B, L, ffh)
        hid = [f(B, Ts[i], dec.channels[i]) for i in range(D)]
        gnp = f(B, (L + 31) // 32, Cmax // 32, 2)
        self.dphi = f(B, L, oc) if not euler else None
        self.out_ct = f(B, oc, L)

        # ---- once-per-solve conditioning ops (time embedding for all steps, speaker affine)
        tdim = dec.in_channels
        pre = [ops.sinusoidal_emb_op(self.t_dev, self.sin, n_steps, tdim, cp0)]
        pre.append(linear_op(self.sin, n_steps, cp0, P["t1_w"], P["t1_b"], self.e1, self.e1.shape[1]))
        pre.append(linear_op(self.e1, n_steps, self.e1.shape[1], P["t2_w"], P["t2_b"], self.temb, self.temb.shape[1],
                             pro_act=ACT_SILU))
        pre.append(linear_op(self.temb, n_steps, self.temb.shape[1], P["tb_w"], P["tb_b"], self.tb, self.tb.shape[1],
                             pro_act=ACT_MISH))
        pre.append(linear_op(self.spk, B, dec.spk_embed_dim, P["spk_w"], P["spk_b"], self.ss, self.ss.shape[1]))
        self.pre = pre

        tb_ld = self.tb.shape[1]
        ss_ld = self.ss.shape[1]
        tb_off, ss_off = [], []
        o1 = o2 = 0
        for r in P["res"]:
            tb_off.append(o1)
            ss_off.append(o2)
            o1 += r["cout"]
            o2 += 2 * r["cout"]

        conv = functools.partial(conv_op, B)

        def resnet(ol, bi, k, lvl, xin, cin, ld_in, out, xin1=None, cin0=0):
            # the block's tail also writes LayerNorm(out) for the transformer block that follows it (tfm skips its norm1)
            r = P["res"][bi]
            t1 = P["tfm"][bi]
            T, C, ln = Ts[lvl], r["cout"], self.lens[lvl]
            extra = {}
            if xin1 is not None:
                extra = dict(in1=xin1, C_in0=cin0, in1_bs=T * (cin - cin0), ld_in1=cin - cin0)
            t3 = ops.conv_taps(3)
            zero_pad = dict(len_out=ln) if rg else {}
            ol.append(conv(xin, cin, T, r["c1_w"], r["c1_b"], bufC, C, T, t3, ld_in=ld_in, len_in=ln,
                           gn_partials=gnp, **zero_pad, **extra))
            ol.append(ops.gn_mish_apply_op(bufC, gnp, r["g1_w"], r["g1_b"], (self.tb, k * tb_ld + tb_off[bi]), ln,
                                           bufA, B, T, C, tb_bs=tb_ld if self.per_sample_t else 0, valid_stats=rg))
            ol.append(conv(bufA, C, T, r["c2_w"], r["c2_b"], bufC, C, T, t3, gn_partials=gnp, **zero_pad))
            ol.append(conv(xin, cin, T, r["r_w"], r["r_b"], bufR, C, T, [0], ld_in=ld_in, len_in=ln, **extra))
            ol.append(ops.resblock_tail_ln_op(bufC, gnp, r["g2_w"], r["g2_b"], ln, bufR, (self.ss, ss_off[bi]),
                                              (self.ss, ss_off[bi] + C), ss_ld, out, t1["ln1_w"], t1["ln1_b"], bufN, B, T, C,
                                              valid_stats=rg))

        def tfm(ol, bi, lvl, X, C):
            t = P["tfm"][bi]
            T, ln = Ts[lvl], self.lens[lvl]
            Tp = rup(T, 32)
            # norm1(X) is already in bufN: the resnet block's tail wrote it (srn_resblock_tail_ln)
            # q | k row-major into qkv; the v third goes straight to V^T (transposed tail of the epilogue)
            ol.append(conv(bufN, C, T, t["qkv_w"], None, qkv, 3 * inner, T, [0], out_tr=Vt[T], out_tr_col0=2 * inner,
                           out_tr_bs=inner * Tp, ld_out_tr=Tp))
            ol += attention_ops(qkv, Vt[T], S, bufO, ln, B, H, hd, T, ops.attention_precision())
            ol.append(conv(bufO, inner, T, t["o_w"], t["o_b"], X, C, T, [0], res=X, res_mode=RES_ADD, res_bs=T * C,
                           ld_res=C))
            ol.append(ops.layernorm_op(X, t["ln3_w"], t["ln3_b"], bufN, B * T, C))
            fh = t["ff2_w"].shape[1]
            ol.append(conv(bufN, C, T, t["ff1_w"], t["ff1_b"], bufG, 2 * fh, T, [0], geglu=True, N_out=fh,
                           out_bs=T * fh, ld_out=fh))
            ol.append(conv(bufG, fh, T, t["ff2_w"], t["ff2_b"], X, C, T, [0], res=X, res_mode=RES_ADD, res_bs=T * C,
                           ld_res=C))

        def build_step(k, dt):
            ol = []
            bi = 0
            cur, ccur, ld_cur = self.h0, cp0, cp0
            # down path
            for i in range(D):
                C = dec.channels[i]
                resnet(ol, bi, k, i, cur, ccur, ld_cur, hid[i], )
                tfm(ol, bi, i, hid[i], C)
                bi += 1
                dn = P["down"][i]
                if dn["stride"] == 2:
                    ol.append(conv(hid[i], C, Ts[i], dn["w"], dn["b"], bufY, C, Ts[i + 1], ops.conv_taps(3),
                                   len_in=self.lens[i], in_stride=2))
                else:
                    ol.append(conv(hid[i], C, Ts[i], dn["w"], dn["b"], bufY, C, Ts[i], ops.conv_taps(3),
                                   len_in=self.lens[i]))
                cur, ccur, ld_cur = bufY, C, C
            other = bufX
            lvl = D - 1
            for _ in range(dec.num_mid_blocks):
                C = P["res"][bi]["cout"]
                resnet(ol, bi, k, lvl, cur, ccur, ld_cur, other)
                tfm(ol, bi, lvl, other, C)
                bi += 1
                cur, other = other, cur
                ccur, ld_cur = C, C
            # up path
            for j in range(D):
                lvl = D - 1 - j
                C = P["res"][bi]["cout"]
                skip = hid[lvl]
                cs = skip.shape[2]
                resnet(ol, bi, k, lvl, cur, ccur + cs, ld_cur, other, xin1=skip, cin0=ccur)
                tfm(ol, bi, lvl, other, C)
                bi += 1
                cur, other = other, cur
                up = P["up"][j]
                if up["transpose"]:
                    Tn = Ts[lvl - 1]
                    for r, (taps, wp) in enumerate(up["phases"]):
                        n_rows = (Tn - r + 1) // 2
                        if n_rows <= 0:
                            continue
                        ol.append(conv(cur, C, Ts[lvl], wp, up["b"], other, C, n_rows, taps, len_in=self.lens[lvl],
                                       out_bs=Tn * C, out_t_stride=2, out_t_off=r))
                else:
                    ol.append(conv(cur, C, Ts[lvl], up["w"], up["b"], other, C, Ts[lvl], ops.conv_taps(3),
                                   len_in=self.lens[lvl]))
                cur, other = other, cur
                ccur, ld_cur = C, C
            # final block + projection (+ fused Euler update)
            C = ccur
            ln = self.lens[0]
            ol.append(conv(cur, C, L, P["fb_w"], P["fb_b"], bufC, C, L, ops.conv_taps(3), len_in=ln, gn_partials=gnp,
                           **(dict(len_out=ln) if rg else {})))
            ol.append(ops.gn_mish_apply_op(bufC, gnp, P["fg_w"], P["fg_b"], None, ln, bufA, B, L, C, valid_stats=rg))
            if euler:
                ol.append(conv(bufA, C, L, P["fp_w"], P["fp_b"], self.h0, oc, L, [0], len_out=ln, res=self.h0,
                               res_mode=RES_AXPY, beta=dt, res_bs=L * cp0, ld_res=cp0, out_bs=L * cp0, ld_out=cp0))
            else:
                ol.append(conv(bufA, C, L, P["fp_w"], P["fp_b"], self.dphi, oc, L, [0], len_out=ln))
            return ol

        self._build_step = build_step
        self.steps = None
        self._dts = None
        self._runner = ops.GraphRunner(lambda: self.pre + [op for ol in self.steps for op in ol])
        self.io_in = [
            None,  # x transpose (set_inputs fills src)
        ]
        self._xin = f(B, oc, L)
        self._muin = f(B, dec.in_channels - oc, L)
        cm = dec.in_channels - oc
        self.load_ops = [ops.transpose_op(self._xin, self.h0, B, oc, L, oc * L, L, L * cp0, cp0),
                         ops.transpose_op(self._muin, (self.h0, oc), B, cm, L, cm * L, L, L * cp0, cp0)]
        self.store_op = ops.transpose_op(self.h0 if euler else self.dphi, self.out_ct, B, L, oc,
                                         L * (cp0 if euler else oc), cp0 if euler else oc, oc * L, L)

    # ------------------------------------------------------------------
    def set_schedule(self, ts, dts):
        """ts/dts: python floats (already fp32-rounded).  Rebuilds the per-step op lists if dt changed."""
        assert len(ts) == self.n_rows
        ts = [float(t) for t in ts]
        if getattr(self, "_ts", None) != ts:  # uploaded only when it changes (the Euler schedule never does)
            self.t_dev.copy_(torch.tensor(ts, dtype=torch.float32), non_blocking=False)
            self._ts = ts
        dts = [0.0] * self.n if dts is None else list(dts)
        if self.steps is None or self._dts != dts:
            self.steps = [self._build_step(k, dts[k]) for k in range(self.n)]
            self._dts = dts
            self._runner.invalidate()

    def set_lens(self, lens):
        lens = torch.as_tensor(lens).to(torch.int64).cpu()
        key = tuple(lens.tolist())
        if getattr(self, "_lens_key", None) == key:
            return
        self._lens_key = key
        cur = lens
        for i, buf in enumerate(self.lens):
            buf.copy_(cur.to(torch.int32))
            cur = (cur + 1) // 2

    def set_inputs(self, x, mu, spk, lens, ts, dts=None):
        """x (B, out_ch, L), mu (B, cond, L) in the reference's (B, C, T) layout."""
        self.set_schedule(ts, dts)
        self.set_lens(lens)
        self._xin.copy_(x)
        self._muin.copy_(mu)
        self.spk.copy_(spk)
        for op in self.load_ops:
            op()

    def run(self):
        self._runner()

    def read_out(self):
        self.store_op()
        return self.out_ct.clone()


# =====================================================================================
#  CFM
# =====================================================================================
def euler_schedule(n_timesteps):
    """(t_k, dt_k) exactly as flow_matching.py:61,79-91 accumulates them: fp32 torch scalars on the host."""
    t_span = torch.linspace(0, 1, n_timesteps + 1)
    t, dt = t_span[0], t_span[1] - t_span[0]
    ts, dts = [], []
    for step in range(1, len(t_span)):
        ts.append(float(t))
        dts.append(float(dt))
        t = t + dt
        if step < len(t_span) - 1:
            dt = t_span[step + 1] - t
    return ts, dts


class CFM(_Packed):
    """flow_matching.py:9-93.  ``inference`` draws the noise with the CPU generator exactly like the
    reference (so ``torch.manual_seed`` reproduces it) and runs the fused Euler loop on the GPU."""

    def __init__(self, in_channels=80, out_channels=80, solver="euler", sigma_min=1e-4, spk_embed_dim=256,
                 decoder_channels=(512, 512), decoder_attention_head_dim=256):
        super().__init__({})
        self.n_feats = in_channels
        self.spk_embed_dim = spk_embed_dim
        self.solver = solver
        self.sigma_min = sigma_min
        self.conditioning_shape = in_channels + out_channels
        self.out_channels = out_channels
        self.estimator = Decoder(in_channels=in_channels, out_channels=out_channels, spk_embed_dim=spk_embed_dim,
                                 channels=decoder_channels, attention_head_dim=decoder_attention_head_dim)

    def forward(self, x1, mask, mu, spks, mask_l=None):
        return self.compute_loss(x1, mask, mu, spks, mask_l)

    @torch.no_grad()
    def compute_loss(self, x1, mask, mu, spks, mask_l=None, draws=None):
        """Forward value of the conditional flow-matching loss, flow_matching.py:95-133 (no autograd: the
        backward pass is outside this build's scope).  The estimator call -- all of the arithmetic that matters --
        runs on the HIP kernels with one time value per sample; the O(B*80*L) interpolation and the scalar
        reductions around it use torch on the same device.  `draws` = {"t": (B,1,1), "z": like x1} overrides
        the random draws (parity tests)."""
        _require_cuda(x1, "CFM.compute_loss")
        b = mu.shape[0]
        if draws is None:
            t = torch.rand([b, 1, 1], device=mu.device, dtype=mu.dtype)
            z = torch.randn_like(x1)
        else:
            t, z = draws["t"].to(x1), draws["z"].to(x1)
        y = (1 - (1 - self.sigma_min) * t) * z + t * x1
        u = x1 - (1 - self.sigma_min) * z
        denoised = self.estimator(y, mask, mu, t.squeeze(), spks)
        if mask_l is not None:
            denoised = denoised * mask_l
            u = u * mask_l
        loss = torch.nn.functional.mse_loss(denoised, u, reduction="sum")
        denom = torch.sum(mask_l) if mask_l is not None else torch.sum(mask)
        return loss / (denom * u.shape[1]), y

    @torch.inference_mode()
    def inference(self, mu, mask, n_timesteps=10, temperature=0.667, spks=None):
        """flow_matching.py:39-63: mu (B, cond, L), mask (B, 1, L), spks (B, S) -> (B, out_ch, L)."""
        _require_cuda(mu, "CFM.inference")
        z = torch.randn((mu.shape[0], self.out_channels, mu.shape[2])).to(mu.device) * temperature
        return self.solve_euler(z, n_timesteps=n_timesteps, mu=mu, mask=mask, trg_spks=spks)

    @torch.inference_mode()
    def solve_euler(self, x, t_span=None, mu=None, mask=None, trg_spks=None, n_timesteps=None):
        """flow_matching.py:65-93.  Either ``t_span`` (the reference's linspace) or ``n_timesteps``."""
        if n_timesteps is None:
            n_timesteps = len(t_span) - 1
        B, _, L = x.shape
        pl = self.estimator.plan(B, L, n_timesteps, euler=True)
        ts, dts = euler_schedule(n_timesteps)
        lens = mask.reshape(B, -1).to(torch.int64).sum(dim=1)
        pl.set_inputs(x, mu, trg_spks, lens, ts, dts)
        pl.run()
        return pl.read_out()


# =====================================================================================
#  Conv1dResnet content encoder
# =====================================================================================
class Conv1dResnet(_Packed):
    """serenade.py:224-356 (inference path; MDN / embedding options of the original are unused by Serenade)."""

    def __init__(self, in_dim, hidden_dim, out_dim, num_layers=4, **kwargs):
        super().__init__(_shapes.encoder_shapes(in_dim, hidden_dim, out_dim, num_layers))
        self.in_dim, self.hidden_dim, self.out_dim, self.num_layers = in_dim, hidden_dim, out_dim, num_layers

    def packed(self):
        if self._packed is None:
            dev = self._device()
            sd = {k: dev_f32(v, dev) for k, v in self._own_state().items()}
            P = dict(in_w=ops.pack_conv_weight(_fold_wn(sd, "model.1")), in_b=sd["model.1.bias"], blocks=[])
            for n in range(self.num_layers):
                p = f"model.{2 + n}"
                P["blocks"].append(dict(
                    d=2 ** n, sc_w=ops.pack_conv_weight(_fold_wn(sd, p + ".shortcut")), sc_b=sd[p + ".shortcut.bias"],
                    c3_w=ops.pack_conv_weight(_fold_wn(sd, p + ".block.2")), c3_b=sd[p + ".block.2.bias"],
                    c1_w=ops.pack_conv_weight(_fold_wn(sd, p + ".block.4")), c1_b=sd[p + ".block.4.bias"]))
            last = f"model.{2 + self.num_layers + 2}"
            P["out_w"], P["out_b"] = ops.pack_conv_weight(_fold_wn(sd, last)), sd[last + ".bias"]
            self._packed = P
        return self._packed

    def build_ops(self, x, B, T, out, out_bs, ld_out, lens=None):
        """x: (B, T, in_dim) device tensor; writes (B, T, out_dim) rows into `out` (tensor or (tensor, off)).
        lens (int32 device tensor (B,)): items are shorter than T; the ReflectionPad1d layers then mirror at each
        item's own end, as they do for the unpadded item (rows beyond an item's length hold unspecified values)."""
        P = self.packed()
        dev = self._device()
        Hd = self.hidden_dim
        f = lambda: torch.zeros(B, T, Hd, device=dev, dtype=torch.float32)
        h, s, b1, h2 = f(), f(), f(), f()

        conv = functools.partial(conv_op, B)
        rf = dict(reflect=True) if lens is None else dict(reflect=2, len_in=lens)
        ol = [conv(x, self.in_dim, T, P["in_w"], P["in_b"], h, Hd, T, ops.conv_taps(7), **rf)]
        cur, nxt = h, h2
        for blk in P["blocks"]:
            d = blk["d"]
            ol.append(conv(cur, Hd, T, blk["sc_w"], blk["sc_b"], s, Hd, T, [0]))
            ol.append(conv(cur, Hd, T, blk["c3_w"], blk["c3_b"], b1, Hd, T, ops.conv_taps(3, d), pro_act=ACT_LEAKY,
                           pro_slope=0.2, **rf))
            ol.append(conv(b1, Hd, T, blk["c1_w"], blk["c1_b"], nxt, Hd, T, [0], pro_act=ACT_LEAKY, pro_slope=0.2,
                           res=s, res_mode=RES_ADD, res_bs=T * Hd, ld_res=Hd))
            cur, nxt = nxt, cur
        ol.append(conv(cur, Hd, T, P["out_w"], P["out_b"], out, self.out_dim, T, ops.conv_taps(7), pro_act=ACT_LEAKY,
                       pro_slope=0.2, out_bs=out_bs, ld_out=ld_out, **rf))
        return ol

    @torch.no_grad()
    def forward(self, x, lengths=None, y=None):
        """(B, T, in_dim) -> (B, T, out_dim)   (serenade.py:310-342)."""
        _require_cuda(x, "Conv1dResnet.forward")
        B, T, _ = x.shape
        xin = x.detach().to(torch.float32).contiguous()
        out = torch.empty(B, T, self.out_dim, device=x.device, dtype=torch.float32)
        ol = self.build_ops(xin, B, T, out, T * self.out_dim, self.out_dim)
        for op in ol:
            op()
        return out

    inference = forward


# =====================================================================================
#  GST style encoder
# =====================================================================================
class StyleEncoder(_Packed):
    """style_encoder.py:16-91 (+ ReferenceEncoder :94-191, StyleTokenLayer :194-252)."""

    def __init__(self, idim=80, gst_tokens=10, gst_token_dim=256, gst_heads=4, conv_layers=6,
                 conv_chans_list=(32, 32, 64, 64, 128, 128), conv_kernel_size=3, conv_stride=2, gru_layers=1,
                 gru_units=128):
        assert conv_kernel_size == 3 and conv_stride == 2 and gru_layers == 1
        assert len(conv_chans_list) == conv_layers
        super().__init__(_shapes.gst_shapes(idim, gst_tokens, gst_token_dim, gst_heads, tuple(conv_chans_list),
                                            gru_units))
        self.idim, self.chans, self.gru_units = idim, tuple(conv_chans_list), gru_units
        self.gst_tokens, self.gst_token_dim, self.gst_heads = gst_tokens, gst_token_dim, gst_heads

    def packed(self):
        if self._packed is None:
            dev = self._device()
            sd = {k: (dev_f32(v, dev) if v.is_floating_point() else v) for k, v in self._own_state().items()}
            P = dict(convs=[])
            fdim = self.idim
            for i, co in enumerate(self.chans):
                w = sd[f"ref_enc.convs.{3 * i}.weight"].permute(0, 2, 3, 1).contiguous()  # (Co, 3, 3, Ci)
                b = f"ref_enc.convs.{3 * i + 1}."
                scale = sd[b + "weight"] / torch.sqrt(sd[b + "running_var"] + 1e-5)
                shift = sd[b + "bias"] - sd[b + "running_mean"] * scale
                # implicit-GEMM form: BatchNorm scale folded into the weights, one [Co][kw][Ci_pad] matrix per kh
                ci = w.shape[3]
                cpad = rup(ci, 4)
                wf = w * scale.view(-1, 1, 1, 1)
                wk = []
                for kh in range(3):
                    m = wf.new_zeros(co, 3, cpad)
                    m[:, :, :ci] = wf[:, kh]
                    wk.append(m.reshape(co, 3 * cpad).contiguous())
                P["convs"].append(dict(w=w, scale=scale.contiguous(), shift=shift.contiguous(), co=co, wk=wk,
                                       cpad=cpad))
                fdim = (fdim - 1) // 2 + 1
            C = self.chans[-1]
            wih = sd["ref_enc.gru.weight_ih_l0"]  # columns ordered (c, f) by the reference's view (:183-186)
            P["w_ih"] = wih.view(-1, C, fdim).permute(0, 2, 1).reshape(wih.shape[0], -1).contiguous()  # -> (f, c)
            P["w_hh"] = sd["ref_enc.gru.weight_hh_l0"]
            P["b_ih"], P["b_hh"] = sd["ref_enc.gru.bias_ih_l0"], sd["ref_enc.gru.bias_hh_l0"]
            P["fdim"] = fdim
            for nm in ("q", "k", "v", "out"):
                P["w" + nm[0]] = sd[f"stl.mha.linear_{nm}.weight"]
                P["b" + nm[0]] = sd[f"stl.mha.linear_{nm}.bias"]
            P["embs"] = sd["stl.gst_embs"]
            # input-independent parts of the tail, formed once here (like the weight-norm / BatchNorm folds): the
            # style tokens' keys and values, and transposed matrices for coalesced matvecs
            toks = torch.tanh(P["embs"])
            P["tok_k"] = (toks @ P["wk"].t() + P["bk"]).contiguous()
            P["tok_v"] = (toks @ P["wv"].t() + P["bv"]).contiguous()
            P["wq_t"], P["wo_t"] = P["wq"].t().contiguous(), P["wo"].t().contiguous()
            P["w_hh_t"] = P["w_hh"].t().contiguous()
            self._packed = P
        return self._packed

    def length_table(self, B):
        """the per-item heights of a ragged batch at every conv layer (build_ops' `lens`), all zero until set_lengths"""
        return StridedLengthTable(len(self.chans), B, self._device())

    def build_ops(self, speech, B, T, out, lens=None):
        """speech (B, T, idim) device tensor -> out (B, gst_token_dim).
        lens (`length_table(B)`): the items hold lens.rows[0][b] <= T prompt rows each, read when the ops RUN; item b's
        style vector is then what this encoder gives for that prompt alone.  Time is the head axis of the Conv2d
        launches, which a conv's own len_in / len_out do not reach, so the prompt image and every layer output but the
        last are masked behind the item's height (srn_zero_rows_ragged): the next layer's kernel row 2 reads the row
        just behind an odd height and must find the zero padding there that the item alone has, not ReLU(shift) or an
        earlier batch's leftovers.  The last layer feeds the GRU, which stops at the item's own step count."""
        P = self.packed()
        dev = self._device()
        ol = []
        # Conv2d(k3, s2, p1) + BN + ReLU as three implicit GEMMs per layer (one per kernel row kh): for a fixed
        # kh the op is a stride-2, 3-tap conv along W over input row 2*ho + kh - 1, batched over (b, ho).
        # Every layer input lives in a buffer with one zero row above and below (so kh = 0 / 2 never leave it);
        # the kh = 1 launch initialises the output (+ folded BN shift), kh = 0 accumulates, kh = 2 accumulates
        # and applies the ReLU.
        H, W, Ci = T, self.idim, 1
        c0 = P["convs"][0]["cpad"]
        cur = torch.zeros(B, H + 2, W, c0, device=dev, dtype=torch.float32)
        ol.append(ops.copy_channels_op(speech, T * W, 1, 0, (cur, W * c0), (H + 2) * W * c0, c0, 0, B, T * W, 1))
        if lens is not None:
            ol.append(ops.zero_rows_ragged_op((cur, W * c0), (H + 2) * W * c0, W * c0, lens.rows[0], B, H))
        n_l = len(P["convs"])
        for li, c in enumerate(P["convs"]):
            Ho, Wo, Co, Cp = (H - 1) // 2 + 1, (W - 1) // 2 + 1, c["co"], c["cpad"]
            last = li == n_l - 1
            pad = 0 if last else 1  # the last layer feeds the GRU: plain (B, Ho, Wo*Co)
            y = torch.zeros(B, Ho + 2 * pad, Wo, Co, device=dev, dtype=torch.float32)
            yo = (y, pad * Wo * Co)
            for j, kh in enumerate((1, 0, 2)):
                kw = dict(in0=(cur, kh * W * Cp), w=c["wk"][kh], out=yo, n_batch=B, n_head=Ho, T_in=W, T_out=Wo,
                          C_in=Cp, N=Co, in0_bs=(H + 2) * W * Cp, in0_hs=2 * W * Cp, ld_in0=Cp, ldw=3 * Cp,
                          out_bs=(Ho + 2 * pad) * Wo * Co, out_hs=Wo * Co, ld_out=Co, taps=[-1, 0, 1], in_stride=2)
                if j == 0:
                    kw.update(bias=c["shift"])
                else:
                    kw.update(res=yo, res_mode=RES_ADD, res_bs=(Ho + 2 * pad) * Wo * Co, res_hs=Wo * Co, ld_res=Co)
                if j == 2:
                    kw.update(post=ops.POST_RELU)
                ol.append(ConvOp(**kw))
            if lens is not None and not last:
                ol.append(ops.zero_rows_ragged_op(yo, (Ho + 2) * Wo * Co, Wo * Co, lens.rows[li + 1], B, Ho))
            cur, H, W, Ci = y, Ho, Wo, Co
        ref = torch.zeros(B, self.gru_units, device=dev, dtype=torch.float32)
        # GRU: input projection of all (b, t) rows as one contraction over the chip, then the short recurrence
        G3, I = 3 * self.gru_units, W * Ci
        if I % 4 != 0:
            raise ValueError(f"GRU input width {I} (mel bins left x channels) must be a multiple of 4")
        gi = torch.zeros(B, H, G3, device=dev, dtype=torch.float32)
        ol.append(linear_op(cur, B * H, I, P["w_ih"], P["b_ih"], gi, G3))
        if lens is None:
            ol.append(ops.gru_recur_last_op(gi, P["w_hh_t"], P["b_hh"], ref, B, H, self.gru_units))
        else:  # the projection above ran over all B * H rows; the recurrence reads an item's first lens.rows[-1][b]
            ol.append(ops.gru_recur_last_ragged_op(gi, P["w_hh_t"], P["b_hh"], ref, lens.rows[n_l], B, H,
                                                   self.gru_units))
        ol.append(ops.style_token_attention_kv_op(ref, P["wq_t"], P["bq"], P["tok_k"], P["tok_v"], P["wo_t"], P["bo"],
                                                  out, B, self.gru_units, self.gst_tokens, self.gst_token_dim,
                                                  self.gst_heads))
        self._last_ref = ref
        return ol

    @torch.no_grad()
    def forward(self, speech, lengths=None):
        """(B, Lmax, idim) -> (B, gst_token_dim)   (style_encoder.py:78-91).
        lengths (B row counts in [1, Lmax]): a padded batch of prompts; item b's vector is what forward gives for
        speech[b:b + 1, :lengths[b]], whatever the rows behind an item hold.  One plan per (B, Lmax) serves every set
        of lengths."""
        _require_cuda(speech, "StyleEncoder.forward")
        B, T, _ = speech.shape
        if lengths is not None:
            lens = item_lengths(lengths, B, T, "StyleEncoder.forward")
            key = ("ragged", B, T, ops.DEFAULT_PRECISION)
            rp = lru_get(self._plans, key, 4, lambda: StyleEncoderRaggedPlan(self, B, T))
            return rp.run(speech, lens)
        out = torch.empty(B, self.gst_token_dim, device=speech.device, dtype=torch.float32)
        ol = self.build_ops(speech.detach().to(torch.float32).contiguous(), B, T, out)
        for op in ol:
            op()
        return out


class StyleEncoderRaggedPlan:
    """`StyleEncoder.forward(speech, lengths=)`: staging buffer, length table and the batched op list for one
    (B, T_cap); the lengths are rewritten in place before each run."""

    def __init__(self, gst, B, T_cap):
        dev = gst._device()
        self.speech = torch.zeros(B, T_cap, gst.idim, device=dev, dtype=torch.float32)
        self.out = torch.zeros(B, gst.gst_token_dim, device=dev, dtype=torch.float32)
        self.table = gst.length_table(B)
        self.ops = gst.build_ops(self.speech, B, T_cap, self.out, lens=self.table)

    def run(self, speech, lens):
        self.speech.copy_(speech.detach())
        self.table.set_lengths(lens)
        for op in self.ops:
            op()
        return self.out.clone()


# =====================================================================================
#  Serenade
# =====================================================================================
RAGGED_BUCKET = 64  # rows: the length bucket of `Serenade.inference_ragged(bucket=)` that the decode CLI uses


class Serenade(_Packed):
    """serenade/models/serenade.py:35-221."""

    def __init__(self, input_dim=768, output_dim=80, encoder_channels=80, decoder_channels=512, gst_embed_dim=256,
                 decoder_attention_head_dim=512, mask_size=[0.1, 0.5], cfg_prob=0.1):
        super().__init__({})
        self.input_dim, self.output_dim, self.cfg_prob = input_dim, output_dim, cfg_prob
        self.encoder_channels = encoder_channels
        self.encoder = Conv1dResnet(in_dim=input_dim, hidden_dim=512, num_layers=2, out_dim=encoder_channels)
        self.gst = StyleEncoder(gst_tokens=50, conv_chans_list=(128, 128, 256, 256, 512, 512),
                                gst_token_dim=gst_embed_dim)
        conditioning_dim = output_dim + encoder_channels + 1 + 1
        self.cfm_decoder = CFM(in_channels=conditioning_dim + output_dim, out_channels=output_dim,
                               spk_embed_dim=gst_embed_dim, decoder_channels=(decoder_channels, decoder_channels),
                               decoder_attention_head_dim=decoder_attention_head_dim)
        self.mask_size = mask_size

    @torch.no_grad()
    def forward(self, x, lengths, logmel, midi, lft, draws=None):
        """Forward value of the training objective, serenade.py:90-166: returns
        {"gauss_mel", "prior_loss", "cfm_loss"} like the reference (values only -- no autograd graph; training /
        backward is out of scope).  Encoder, GST and the estimator run on the HIP kernels; the infill-mask
        bookkeeping and the scalar reductions use torch on the same device.  `draws` (tests) may carry
        {"uniform", "seg_start", "t", "z"} to replace the random draws."""
        import random
        _require_cuda(x, "Serenade.forward")
        ret = {}
        enc_outs = self.encoder(x, lengths)
        ret["gauss_mel"] = enc_outs
        speaker_features = self.gst(logmel)
        mask = make_non_pad_mask(lengths).to(x.device).unsqueeze(1)
        uni = random.uniform(self.mask_size[0], self.mask_size[1]) if draws is None else draws["uniform"]
        mask_size = int(uni * enc_outs.size(1))
        seg_start = random.randint(0, enc_outs.size(1) - mask_size) if draws is None else int(draws["seg_start"])
        seg_end = seg_start + mask_size
        mask_l = mask.clone()
        mask_l[:, :, 0:seg_start] = 0
        mask_l[:, :, seg_end:] = 0
        mask_c = mask.clone()
        mask_c[:, :, seg_start:seg_end] = 0
        prior_loss = torch.sum(0.5 * ((logmel.permute(0, 2, 1) - enc_outs.permute(0, 2, 1)) ** 2
                                      + math.log(2 * math.pi)) * mask)
        ret["prior_loss"] = prior_loss / (torch.sum(mask) * self.output_dim)
        targets = logmel * mask_l.permute(0, 2, 1)
        cond = logmel * mask_c.permute(0, 2, 1)
        mu = torch.cat([enc_outs, midi, lft, cond], dim=-1)
        ret["cfm_loss"], _ = self.cfm_decoder.compute_loss(
            x1=targets.permute(0, 2, 1).contiguous(), mask=mask, mu=mu.permute(0, 2, 1).contiguous(),
            spks=speaker_features, mask_l=mask_l, draws=draws)
        return ret

    @torch.inference_mode()
    def inference_ragged(self, items, n_timesteps=10, temperature=0.667, noises=None, bucket=None):
        """Several conversions in ONE batch, each exactly what `inference` returns for it alone (B = 1): `items` is a
        list of (x (T,in), midi (T,1), lft (T,1), ref_x (R,in), ref_logmel (R,out), ref_midi (R,1), ref_lft (R,1));
        T and R may differ per item.  Returns a list of (T, out) tensors.  `noises` (optional list of (out, R + T)
        tensors) replaces the draws; by default the noise of item b is drawn on the CPU generator in item order, as a
        loop of B = 1 calls would (flow_matching.py:57-60).  This is what the decode CLI batches its styles with.
        bucket (int >= 1; the CLI passes RAGGED_BUCKET): lengths as data -- one plan, and with graphs on one capture,
        per (B, longest R + T rounded up to `bucket`) instead of one per tuple of shapes (BucketedInferencePlan)."""
        if len(items) == 0:
            raise ValueError("Serenade.inference_ragged: no items")
        if bucket is not None:
            if isinstance(bucket, bool) or not isinstance(bucket, int) or bucket < 1:
                raise ValueError(f"Serenade.inference_ragged: bucket must be an int >= 1, not {bucket!r}")
            shapes = _ragged_item_shapes(items)
        _require_cuda(items[0][0], "Serenade.inference_ragged")
        if bucket is not None:
            L_cap = rup(max(t + r for t, r in shapes), bucket)
            key = ("ragged-bucket", len(items), L_cap, n_timesteps, ops.DEFAULT_PRECISION, ops.attention_precision())
            rp = lru_get(self._plans, key, 4, lambda: BucketedInferencePlan(self, len(items), L_cap, n_timesteps))
            rp.set_lengths(shapes)
            rp.load(items)
            if noises is None:
                dev = items[0][0].device
                noises = [torch.randn((1, self.output_dim, t + r)).to(dev)[0] * temperature for t, r in shapes]
            return rp.run(noises)
        shapes = tuple((int(it[0].shape[0]), int(it[3].shape[0])) for it in items)
        key = ("ragged", shapes, n_timesteps, ops.DEFAULT_PRECISION, ops.attention_precision())
        rp = lru_get(self._plans, key, 4, lambda: RaggedInferencePlan(self, shapes, n_timesteps))
        rp.load(items)
        dev = items[0][0].device
        if noises is None:
            noises = [torch.randn((1, self.output_dim, t + r)).to(dev)[0] * temperature for t, r in shapes]
        return rp.run(noises)

    def _inference_plan(self, B, T, Tr, n_timesteps):
        key = (B, T, Tr, n_timesteps, ops.DEFAULT_PRECISION, ops.attention_precision())
        return lru_get(self._plans, key, 8, lambda: InferencePlan(self, B, T, Tr, n_timesteps))

    @torch.inference_mode()
    def inference(self, x, lengths, midi, lft, ref_x, ref_lengths, ref_logmel, ref_midi, ref_lft,
                  n_timesteps=10, temperature=0.667, noise=None):
        """serenade.py:168-221.  Returns (T, out) if B == 1 else (B, T, out).

        ``noise`` (optional, (B, out, T_ref + T)) replaces ``randn * temperature`` for reproducible parity runs;
        by default the noise is drawn on the CPU generator exactly like the reference."""
        _require_cuda(x, "Serenade.inference")
        B, T, _ = x.shape
        Tr = ref_x.shape[1]
        ip = self._inference_plan(B, T, Tr, n_timesteps)
        ip.load(x, midi, lft, ref_x, ref_logmel, ref_midi, ref_lft)
        if noise is None:  # drawn on the CPU generator, then moved (flow_matching.py:57-60)
            z = torch.randn((B, self.output_dim, Tr + T)).to(x.device) * temperature
        else:
            z = noise
        total = lengths.to(torch.int64).cpu() + ref_lengths.to(torch.int64).cpu()
        mel = ip.run(z, total).permute(0, 2, 1)  # (B, L, oc)
        mel = mel[:, int(ref_lengths[0]):, :]
        return mel.squeeze(0)


class RaggedInferencePlan:
    """`Serenade.inference_ragged`: a batch of conversions whose source AND prompt lengths differ, every item computed
    exactly as its own B = 1 call (the reference's decode loop, ssc_decode.py:346-438, is B = 1 by construction).
    Per item b the sequence is [prompt rows (R_b) | source rows (T_b)] from row 0, padded to the batch maximum:
    * the two content-encoder passes mirror at each item's own end (`pad_reflect = 2`);
    * prompt conditioning is written from row 0, source conditioning is scattered to row R_b (`srn_scatter_rows`);
    * the style encoder runs per item (its conv stack / GRU see the whole prompt: no masking exists there);
    * the estimator plan is built `exact_ragged` (GroupNorm over valid rows)."""

    def __init__(self, model, shapes, n_timesteps):
        dev = model._device()
        self.shapes = shapes = [(int(t), int(r)) for t, r in shapes]
        B = self.B = len(shapes)
        Tm, Rm = max(t for t, _ in shapes), max(r for _, r in shapes)
        Lm = self.Lm = max(t + r for t, r in shapes)
        oc, ec = model.output_dim, model.encoder_channels
        self.pl = pl = model.cfm_decoder.estimator.plan(B, Lm, n_timesteps, euler=True, exact_ragged=True)
        h0, cp0 = pl.h0, pl.h0.shape[2]
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.x, self.ref_x = f(B, Tm, model.input_dim), f(B, Rm, model.input_dim)
        self.ref_mel = f(B, Rm, oc)
        self.midi, self.lft, self.ref_midi, self.ref_lft = f(B, Tm, 1), f(B, Tm, 1), f(B, Rm, 1), f(B, Rm, 1)
        self.zeros, self.enc_src = f(B, Tm, oc), f(B, Tm, ec)
        self.t_len, self.r_len = i32([t for t, _ in shapes]), i32([r for _, r in shapes])
        c0 = oc + ec
        ol = model.encoder.build_ops(self.ref_x, B, Rm, (h0, oc), Lm * cp0, cp0, lens=self.r_len)
        ol.append(ops.copy_channels_op(self.ref_midi, Rm, 1, 0, h0, Lm * cp0, cp0, c0, B, Rm, 1))
        ol.append(ops.copy_channels_op(self.ref_lft, Rm, 1, 0, h0, Lm * cp0, cp0, c0 + 1, B, Rm, 1))
        ol.append(ops.copy_channels_op(self.ref_mel, Rm * oc, oc, 0, h0, Lm * cp0, cp0, c0 + 2, B, Rm, oc))
        # source rows start where the item's prompt ends (they overwrite whatever the padded prompt rows left there)
        ol += model.encoder.build_ops(self.x, B, Tm, self.enc_src, Tm * ec, ec, lens=self.t_len)
        for src, ch, width in ((self.enc_src, oc, ec), (self.midi, c0, 1), (self.lft, c0 + 1, 1),
                               (self.zeros, c0 + 2, oc)):
            ol.append(ops.scatter_rows_op(src, Tm * width, width, h0, Lm * cp0, cp0, ch, self.r_len, self.t_len, B, Tm,
                                          width))
        for b, (_, r) in enumerate(shapes):
            ol += model.gst.build_ops((self.ref_mel, b * Rm * oc), 1, r, (pl.spk, b * pl.spk.shape[1]))
        self.ops = ol
        self._runner = ops.GraphRunner(lambda: self.ops)
        self._sched = euler_schedule(n_timesteps)
        self._z = f(B, oc, Lm)

    def load(self, items):
        """items: per conversion (x, midi, lft, ref_x, ref_logmel, ref_midi, ref_lft), 2-D tensors"""
        for b, it in enumerate(items):
            t, r = self.shapes[b]
            for buf, src, n in ((self.x, it[0], t), (self.midi, it[1], t), (self.lft, it[2], t), (self.ref_x, it[3], r),
                                (self.ref_mel, it[4], r), (self.ref_midi, it[5], r), (self.ref_lft, it[6], r)):
                buf[b, :n].copy_(src.detach().reshape(n, -1), non_blocking=True)

    def run(self, noises):
        pl = self.pl
        for b, z in enumerate(noises):  # (oc, L_b) each
            self._z[b, :, : z.shape[-1]].copy_(z.reshape(self._z.shape[1], -1), non_blocking=True)
        pl.set_schedule(*self._sched)
        pl.set_lens(torch.tensor([t + r for t, r in self.shapes]))
        pl._xin.copy_(self._z, non_blocking=True)
        pl.load_ops[0]()
        self._runner()
        pl.run()
        out = pl.read_out()  # (B, oc, Lm)
        return [out[b, :, r:r + t].t().contiguous() for b, (t, r) in enumerate(self.shapes)]


RAGGED_MIN_ROWS = 4  # the content encoder's ReflectionPad1d(3) needs more than 3 rows of the longest track


def _ragged_item_shapes(items):
    """[(T_b, R_b)] of `inference_ragged`'s items, or ValueError: every track of an item must have the item's row
    count, and the lengths must be ones the shape-keyed plan accepts (no empty track; the longest source and the
    longest prompt of the batch carry the encoder's reflection padding)."""
    shapes = []
    for b, it in enumerate(items):
        if len(it) != 7:
            raise ValueError(f"Serenade.inference_ragged: item {b} has {len(it)} tensors, not (x, midi, lft, ref_x, "
                             "ref_logmel, ref_midi, ref_lft)")
        t, r = int(it[0].shape[0]), int(it[3].shape[0])
        for name, src, n in (("midi", it[1], t), ("lft", it[2], t), ("ref_logmel", it[4], r), ("ref_midi", it[5], r),
                             ("ref_lft", it[6], r)):
            if int(src.shape[0]) != n:
                raise ValueError(f"Serenade.inference_ragged: item {b}: {name} has {int(src.shape[0])} rows, its "
                                 f"{'prompt' if name.startswith('ref') else 'source'} has {n}")
        if t < 1 or r < 1:
            raise ValueError(f"Serenade.inference_ragged: item {b} has an empty track (T = {t}, R = {r})")
        shapes.append((t, r))
    if max(t for t, _ in shapes) < RAGGED_MIN_ROWS or max(r for _, r in shapes) < RAGGED_MIN_ROWS:
        raise ValueError(f"Serenade.inference_ragged: the longest source and the longest prompt need at least "
                         f"{RAGGED_MIN_ROWS} rows each (reflection padding), got (T, R) = {shapes}")
    return shapes


class BucketedInferencePlan(RaggedInferencePlan):
    """`Serenade.inference_ragged(bucket=)`: RaggedInferencePlan with every length as DATA, one plan per (B, L_cap)
    where L_cap is the batch's longest R_b + T_b rounded up to the bucket.  The source and the prompt staging buffers
    have L_cap rows each (either track of an item may be as long as the cap), the estimator plan is (B, L_cap)
    `exact_ragged`, and the style encoder is ONE batched op list over (B, L_cap) prompt rows with per-item heights
    (`StyleEncoder.build_ops(lens=)`), not one list per item.  `set_lengths` rewrites t_len, r_len, the style encoder's
    table and the estimator's lengths in place before a run -- outside the captured graphs, whose nodes carry only the
    buffers' addresses -- so one capture serves every batch of the bucket.  What lies behind an item's rows in any
    buffer (an earlier batch's leftovers) is never read as data.  `load` and `run` are the shape-keyed plan's."""

    def __init__(self, model, B, L_cap, n_timesteps):
        dev = model._device()
        self.B, self.Lm, self.shapes = B, L_cap, None
        oc, ec = model.output_dim, model.encoder_channels
        self.pl = pl = model.cfm_decoder.estimator.plan(B, L_cap, n_timesteps, euler=True, exact_ragged=True)
        h0, cp0 = pl.h0, pl.h0.shape[2]
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.x, self.ref_x = f(B, L_cap, model.input_dim), f(B, L_cap, model.input_dim)
        self.ref_mel = f(B, L_cap, oc)
        self.midi, self.lft, self.ref_midi, self.ref_lft = f(B, L_cap, 1), f(B, L_cap, 1), f(B, L_cap, 1), f(B, L_cap, 1)
        self.zeros, self.enc_src = f(B, L_cap, oc), f(B, L_cap, ec)
        self.t_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.r_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.gst_lens = model.gst.length_table(B)
        c0 = oc + ec
        ol = model.encoder.build_ops(self.ref_x, B, L_cap, (h0, oc), L_cap * cp0, cp0, lens=self.r_len)
        ol.append(ops.copy_channels_op(self.ref_midi, L_cap, 1, 0, h0, L_cap * cp0, cp0, c0, B, L_cap, 1))
        ol.append(ops.copy_channels_op(self.ref_lft, L_cap, 1, 0, h0, L_cap * cp0, cp0, c0 + 1, B, L_cap, 1))
        ol.append(ops.copy_channels_op(self.ref_mel, L_cap * oc, oc, 0, h0, L_cap * cp0, cp0, c0 + 2, B, L_cap, oc))
        # source rows start where the item's prompt ends; R_b + T_b <= L_cap keeps them inside the item's rows of h0
        ol += model.encoder.build_ops(self.x, B, L_cap, self.enc_src, L_cap * ec, ec, lens=self.t_len)
        for src, ch, width in ((self.enc_src, oc, ec), (self.midi, c0, 1), (self.lft, c0 + 1, 1),
                               (self.zeros, c0 + 2, oc)):
            ol.append(ops.scatter_rows_op(src, L_cap * width, width, h0, L_cap * cp0, cp0, ch, self.r_len, self.t_len, B,
                                          L_cap, width))
        ol += model.gst.build_ops(self.ref_mel, B, L_cap, pl.spk, lens=self.gst_lens)
        self.ops = ol
        self._runner = ops.GraphRunner(lambda: self.ops)
        self._sched = euler_schedule(n_timesteps)
        self._z = f(B, oc, L_cap)

    def set_lengths(self, shapes):
        """shapes: B pairs (T_b, R_b) with R_b + T_b <= L_cap (validated by the caller, _ragged_item_shapes)"""
        shapes = [(int(t), int(r)) for t, r in shapes]
        assert len(shapes) == self.B and max(t + r for t, r in shapes) <= self.Lm
        self.shapes = shapes
        self.t_len.copy_(torch.tensor([t for t, _ in shapes], dtype=torch.int32))
        self.r_len.copy_(torch.tensor([r for _, r in shapes], dtype=torch.int32))
        self.gst_lens.set_lengths([r for _, r in shapes])
        self.pl.set_lens(torch.tensor([t + r for t, r in shapes]))


class InferencePlan:
    """Everything `Serenade.inference` does before the Euler loop, planned once per (B, T, T_ref): staging buffers for
    the caller's tensors (the prebuilt calls hold raw pointers, so inputs are copied into stable storage), the two
    content-encoder passes, the conditioning copies and the GST pass as ONE prebuilt op list that writes `mu` in place
    into the estimator plan's h0 and the style vector into its speaker buffer.  (Round 1 rebuilt ~100 op objects and
    re-zeroed ~20 scratch tensors per call.)"""

    def __init__(self, model, B, T, Tr, n_timesteps):
        dev = model._device()
        L = Tr + T
        oc, ec = model.output_dim, model.encoder_channels
        self.pl = pl = model.cfm_decoder.estimator.plan(B, L, n_timesteps, euler=True)
        self.n = n_timesteps
        h0, cp0 = pl.h0, pl.h0.shape[2]
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.x, self.ref_x = f(B, T, model.input_dim), f(B, Tr, model.input_dim)
        self.ref_mel = f(B, Tr, oc)
        self.midi, self.lft, self.ref_midi, self.ref_lft = f(B, T, 1), f(B, T, 1), f(B, Tr, 1), f(B, Tr, 1)
        self.zeros = f(B, T, oc)  # zero conditioning of the source rows (serenade.py:193-199)
        ol = []
        # mu, built in place in h0 channels [oc, oc + cond): time-concat of reference and source rows
        ol += model.encoder.build_ops(self.ref_x, B, Tr, (h0, oc), L * cp0, cp0)
        ol += model.encoder.build_ops(self.x, B, T, (h0, Tr * cp0 + oc), L * cp0, cp0)
        c0 = oc + ec
        ol.append(ops.copy_channels_op(self.ref_midi, Tr, 1, 0, h0, L * cp0, cp0, c0, B, Tr, 1))
        ol.append(ops.copy_channels_op(self.ref_lft, Tr, 1, 0, h0, L * cp0, cp0, c0 + 1, B, Tr, 1))
        ol.append(ops.copy_channels_op(self.ref_mel, Tr * oc, oc, 0, h0, L * cp0, cp0, c0 + 2, B, Tr, oc))
        ol.append(ops.copy_channels_op(self.midi, T, 1, 0, (h0, Tr * cp0), L * cp0, cp0, c0, B, T, 1))
        ol.append(ops.copy_channels_op(self.lft, T, 1, 0, (h0, Tr * cp0), L * cp0, cp0, c0 + 1, B, T, 1))
        ol.append(ops.copy_channels_op(self.zeros, T * oc, oc, 0, (h0, Tr * cp0), L * cp0, cp0, c0 + 2, B, T, oc))
        # style vector straight into the estimator plan's speaker buffer
        ol += model.gst.build_ops(self.ref_mel, B, Tr, pl.spk)
        self.ops = ol
        self._runner = ops.GraphRunner(lambda: self.ops)
        self._sched = euler_schedule(n_timesteps)

    def load(self, x, midi, lft, ref_x, ref_logmel, ref_midi, ref_lft):
        for dst, src in ((self.x, x), (self.midi, midi), (self.lft, lft), (self.ref_x, ref_x),
                         (self.ref_mel, ref_logmel), (self.ref_midi, ref_midi), (self.ref_lft, ref_lft)):
            dst.copy_(src.detach().reshape(dst.shape), non_blocking=True)

    def run(self, z, total_lengths):
        """z (B, oc, L) noise (already temperature-scaled); returns the estimator plan's (B, oc, L) output"""
        pl = self.pl
        pl.set_schedule(*self._sched)
        pl.set_lens(total_lengths)
        pl._xin.copy_(z, non_blocking=True)
        pl.load_ops[0]()
        self._runner()
        pl.run()
        return pl.read_out()
