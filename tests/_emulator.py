"""TEST-ONLY executable specification of the C ABI (include/serenade_hip.h) in CPU torch.

It lets the CPU test-suite exercise all *host logic* of the product (weight packing, buffer plans,
strides, tap tables, phase decomposition) without a GPU: ``install()`` swaps the ``__call__`` of
``ops.ConvOp`` / ``ops.CallOp`` for these functions.  It is never importable from the product and it
is NOT a fallback: on the GPU box the real library runs and is checked against the oracle.
"""
import inspect
import math

import torch
import torch.nn.functional as F

from serenade_amd import _lib, models, ops, training, vocoder


def _flat(x):
    if x is None:
        return None, 0
    if isinstance(x, tuple):
        t, off = x
        return t.view(-1), int(off)
    return x.view(-1), 0


def _act(a, act, slope):
    if act == _lib.ACT_LEAKY:
        return F.leaky_relu(a, slope)
    if act == _lib.ACT_SILU:
        return F.silu(a)
    if act == _lib.ACT_MISH:
        return F.mish(a)
    return a


def emul_conv(kw):
    g = kw.get
    nb, nh = g("n_batch"), g("n_head", 1)
    T_in, T_out, C_in, N = g("T_in"), g("T_out"), g("C_in"), g("N")
    C_in0 = g("C_in0", 0) or C_in
    C_w = g("C_w", 0) or C_in
    taps = list(g("taps", (0,)))
    in_stride = g("in_stride", 1) or 1
    geglu = bool(g("geglu", False))
    N_out = g("N_out", 0) or (N // 2 if geglu else N)
    in0, o_in0 = _flat(g("in0"))
    in1, o_in1 = _flat(g("in1"))
    w, o_w = _flat(g("w"))
    out, o_out = _flat(g("out"))
    res, o_res = _flat(g("res"))
    res2, o_res2 = _flat(g("res2"))
    gnp, o_gnp = _flat(g("gn_partials"))
    bias = g("bias")
    len_in, len_out = g("len_in"), g("len_out")
    ots, oto = g("out_t_stride", 1) or 1, g("out_t_off", 0)
    assert C_in % 4 == 0 and g("ld_in0") % 4 == 0 and g("ldw") % 4 == 0
    assert o_in0 % 4 == 0 and o_w % 4 == 0, "16-byte alignment of in0 / w"
    t = torch.arange(T_out)
    for zb in range(nb):
        li = T_in if len_in is None else min(int(len_in[zb]), T_in)
        lo = T_out if len_out is None else min(int(len_out[zb]), T_out)
        for zh in range(nh):
            A = torch.zeros(T_out, len(taps), C_in)
            for j, off in enumerate(taps):
                ti = t * in_stride + off
                if g("reflect", False):
                    t_ref = li if int(g("reflect")) == 2 else T_in  # 2: mirror at the item's own end
                    ti = torch.where(ti < 0, -ti, ti)
                    ti = torch.where(ti >= t_ref, 2 * (t_ref - 1) - ti, ti)
                valid = ((ti >= 0) & (ti < li)).float().unsqueeze(1)
                tic = ti.clamp(0, T_in - 1)
                base = o_in0 + zb * g("in0_bs", 0) + zh * g("in0_hs", 0)
                idx = base + tic.unsqueeze(1) * g("ld_in0") + torch.arange(C_in0).unsqueeze(0)
                A[:, j, :C_in0] = in0[idx] * valid
                if C_in0 < C_in:
                    assert C_in0 % 32 == 0
                    c1 = C_in - C_in0
                    idx = o_in1 + zb * g("in1_bs", 0) + tic.unsqueeze(1) * g("ld_in1") + torch.arange(c1).unsqueeze(0)
                    A[:, j, C_in0:] = in1[idx] * valid
            A = _act(A, g("pro_act", 0), g("pro_slope", 0.0))
            wb = o_w + zb * g("w_bs", 0) + zh * g("w_hs", 0)
            if g("w_nmajor", False):
                assert len(taps) == 1
                idx = wb + torch.arange(C_w).unsqueeze(1) * g("ldw") + torch.arange(N).unsqueeze(0)
                Wm = torch.zeros(C_in, N)
                Wm[:C_w] = w[idx]
                val = A.reshape(T_out, -1) @ Wm
            else:
                idx = wb + torch.arange(N).unsqueeze(1) * g("ldw") + torch.arange(len(taps) * C_in).unsqueeze(0)
                Wm = w[idx].reshape(N, len(taps), C_in).clone()
                Wm[:, :, C_w:] = 0
                val = A.reshape(T_out, -1) @ Wm.reshape(N, -1).t()
            val = val * g("alpha", 1.0)
            if bias is not None:
                val = val + bias.view(-1)[:N]
            if geglu:
                v = val.reshape(T_out, N // 64, 2, 32)
                val = (v[:, :, 0] * F.gelu(v[:, :, 1])).reshape(T_out, N // 2)
            val = val[:, :N_out].clone()
            val[lo:] = 0
            cols = torch.arange(N_out).unsqueeze(0)
            if g("res_mode", 0):
                ridx = o_res + zb * g("res_bs", 0) + zh * g("res_hs", 0) + (t * ots + oto).unsqueeze(1) * g("ld_res") + cols
                if g("res_mode") == _lib.RES_ADD:
                    val = val + res[ridx]
                else:
                    val = res[ridx] + g("beta", 0.0) * val
            if res2 is not None:
                val = val + res2[o_res2 + zb * g("res2_bs", 0) + (t * ots + oto).unsqueeze(1) * g("ld_res2") + cols]
            if g("post", 0) == _lib.POST_DIV:
                val = val / g("post_div", 1.0)
            elif g("post", 0) == _lib.POST_TANH:
                val = torch.tanh(val)
            elif g("post", 0) == _lib.POST_RELU:
                val = torch.relu(val)
            elif g("post", 0) == _lib.POST_LEAKY:
                val = F.leaky_relu(val, g("post_div", 1.0))
            elif g("post", 0) == _lib.POST_GELU:
                val = F.gelu(val)
            oidx = o_out + zb * g("out_bs", 0) + zh * g("out_hs", 0) + (t * ots + oto).unsqueeze(1) * g("ld_out") + cols
            if g("out_tr") is not None:  # transposed tail: columns >= col0 go to out_tr[zb][c - col0][t] instead
                c0 = g("out_tr_col0", 0)
                assert c0 % 32 == 0 and nh == 1 and ots == 1 and not geglu
                otr, o_otr = _flat(g("out_tr"))
                tidx = o_otr + zb * g("out_tr_bs", 0) + (cols[:, c0:] - c0) * g("ld_out_tr") + t.unsqueeze(1)
                otr[tidx] = val[:, c0:]
                out[oidx[:, :c0]] = val[:, :c0]
            else:
                out[oidx] = val
            if gnp is not None:
                mt, nt = (T_out + 31) // 32, N // 32
                pad = torch.zeros(mt * 32, nt * 32)
                pad[:T_out, :N_out] = val
                tiles = pad.reshape(mt, 32, nt, 32)
                part = torch.stack([tiles.sum(dim=(1, 3)), (tiles ** 2).sum(dim=(1, 3))], dim=-1)
                gnp[o_gnp + zb * mt * nt * 2: o_gnp + (zb + 1) * mt * nt * 2] = part.reshape(-1)


def _v(x, n=None):
    """flat view of a tensor or (tensor, offset), optionally the first n elements"""
    f, o = _flat(x)
    return f[o:] if n is None else f[o:o + n]


def _group_stats(partials, b, T, C, groups, eps, n_rows=None):
    mt, nt = (T + 31) // 32, C // 32
    p = _v(partials)[b * mt * nt * 2:(b + 1) * mt * nt * 2].reshape(mt, nt, 2).double()
    per = (C // groups) // 32
    s = p.reshape(mt, groups, per, 2).sum(dim=(0, 2))
    cnt = max(T if n_rows is None else n_rows, 1) * (C // groups)
    mean = s[:, 0] / cnt
    var = (s[:, 1] / cnt - mean * mean).clamp_min(0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float()


def _c_float(x):
    """a Python float as it arrives behind the C ABI's `float` parameters: 1 - beta2 is formed from the ROUNDED beta2
    (1 - float(0.999) is 1.3e-5 below 0.001)"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _sumsq_blocks(n):
    return max(1, min(1024, ((n + 7) // 8 + 255) // 256))  # srn_sumsq_blocks


def emul_call(name, a):
    if name == "srn_gn_mish_apply":
        x, part, gamma, beta, tb, tb_bs, lens, y, B, T, C, groups, eps, valid = a
        xv, yv = _v(x, B * T * C).reshape(B, T, C), _v(y, B * T * C).reshape(B, T, C)
        lens = None if lens is None else _v(lens)
        for b in range(B):
            mean, rstd = _group_stats(part, b, T, C, groups, eps, min(int(lens[b]), T) if valid else None)
            m = mean.repeat_interleave(C // groups)
            r = rstd.repeat_interleave(C // groups)
            o = F.mish((xv[b] - m) * r * gamma + beta)
            if tb is not None:
                o = o + _v(tb)[b * tb_bs: b * tb_bs + C]
            ln = T if lens is None else min(int(lens[b]), T)
            o[ln:] = 0
            yv[b] = o
    elif name in ("srn_resblock_tail", "srn_resblock_tail_ln"):
        ln2 = None
        if name == "srn_resblock_tail_ln":
            a, ln2 = a[:17], a[17:]
        c2, part, gamma, beta, lens, r, scale, shift, ld_ss, y, B, T, C, groups, ge, le, valid = a
        xv, rv, yv = (_v(t, B * T * C).reshape(B, T, C) for t in (c2, r, y))
        lens = None if lens is None else _v(lens)
        for b in range(B):
            mean, rstd = _group_stats(part, b, T, C, groups, ge, min(int(lens[b]), T) if valid else None)
            m = mean.repeat_interleave(C // groups)
            rs = rstd.repeat_interleave(C // groups)
            o = F.mish((xv[b] - m) * rs * gamma + beta)
            ln = T if lens is None else min(int(lens[b]), T)
            o[ln:] = 0
            v = o + rv[b]
            mu = v.mean(dim=-1, keepdim=True)
            var = ((v - mu) ** 2).mean(dim=-1, keepdim=True)
            yv[b] = (v - mu) / (var + le).sqrt() * _v(scale)[b * ld_ss: b * ld_ss + C] + _v(shift)[b * ld_ss: b * ld_ss + C]
        if ln2 is not None:
            g2, b2, y2, e2 = ln2
            _v(y2, B * T * C).reshape(B * T, C)[:] = F.layer_norm(yv.reshape(B * T, C), (C,), g2, b2, e2)
    elif name == "srn_layernorm":
        x, gamma, beta, y, rows, C, eps = a
        _v(y, rows * C).reshape(rows, C)[:] = F.layer_norm(_v(x, rows * C).reshape(rows, C), (C,), gamma, beta, eps)
    elif name == "srn_softmax_rows":
        s, lens, Z, nh, L, ld = a
        sv = _v(s, Z * L * ld).reshape(Z, L, ld)
        lens = None if lens is None else _v(lens)
        for z in range(Z):
            ln = L if lens is None else min(int(lens[z // nh]), L)
            row = sv[z, :, :L].clone()
            row[:, ln:] = float("-inf")
            sv[z, :, :L] = torch.softmax(row, dim=-1)
            sv[z, :, L:] = 0
    elif name == "srn_sinusoidal_emb":
        t, out, n, dim, ld, scale = a
        half = dim // 2
        e = math.log(10000) / (half - 1)
        f = torch.exp(torch.arange(half).float() * -e)
        arg = scale * _v(t, n).unsqueeze(1) * f.unsqueeze(0)
        ov = _v(out, n * ld).reshape(n, ld)
        ov[:, :half] = arg.sin()
        ov[:, half:dim] = arg.cos()
    elif name == "srn_copy_channels":
        src, sbs, lds, sc0, dst, dbs, ldd, dc0, B, T, C = a
        sf, df = _v(src), _v(dst)
        tt, cc = torch.arange(T).unsqueeze(1), torch.arange(C).unsqueeze(0)
        for b in range(B):
            df[b * dbs + tt * ldd + dc0 + cc] = sf[b * sbs + tt * lds + sc0 + cc]
    elif name == "srn_weight_norm_fwd":
        v, g, w, wd, inv, N, C, k = a
        vv = _v(v, N * C * k).reshape(N, C, k).double()
        nrm = vv.reshape(N, -1).norm(dim=1)
        wp = (vv * (_v(g, N).double() / nrm).reshape(N, 1, 1)).permute(0, 2, 1)  # (N, k, C)
        _v(w, N * k * C).reshape(N, k, C)[:] = wp.float()
        _v(inv, N)[:] = (1.0 / nrm).float()
        if wd is not None:
            _v(wd, C * k * N).reshape(C, k, N)[:] = wp.permute(2, 1, 0).float()
    elif name == "srn_weight_norm_bwd":
        dw, v, g, inv, dv, dg, N, C, k = a
        vv = _v(v, N * C * k).reshape(N, C, k).double()
        dd = _v(dw, N * k * C).reshape(N, k, C).double().permute(0, 2, 1)  # (N, C, k)
        iv, gg = _v(inv, N).double(), _v(g, N).double()
        dot = (dd * vv).reshape(N, -1).sum(1)
        _v(dg, N)[:] = (dot * iv).float()
        _v(dv, N * C * k).reshape(N, C, k)[:] = ((gg * iv).reshape(N, 1, 1) * (dd - vv * (dot * iv * iv).reshape(N, 1, 1))).float()
    elif name == "srn_transpose_ct":
        src, dst, B, R, Cc, sbs, lds, dbs, ldd = a
        sf, df = _v(src), _v(dst)
        rr, cc = torch.arange(R).unsqueeze(1), torch.arange(Cc).unsqueeze(0)
        for b in range(B):
            df[b * dbs + cc * ldd + rr] = sf[b * sbs + rr * lds + cc]
    elif name == "srn_renorm":
        x, ts, tm, vm, vs, y, rows, C = a
        v = _v(x, rows * C).reshape(rows, C)
        if ts is not None:
            v = v * ts + tm
        _v(y, rows * C).reshape(rows, C)[:] = (v - vm) / vs
    elif name == "srn_out_conv_tanh":
        x, w, bias, y, B, T, C, k, slope = a
        xv = F.leaky_relu(_v(x, B * T * C).reshape(B, T, C), slope).transpose(1, 2)
        wv = _v(w, k * C).reshape(k, C).t().unsqueeze(0)
        _v(y, B * T).reshape(B, T)[:] = torch.tanh(F.conv1d(xv, wv, bias.view(-1), padding=(k - 1) // 2))[:, 0]
    elif name == "srn_pd_gather":
        x, d, out, B, T, C, dil, slope = a
        xv = F.leaky_relu(_v(x, B * T * C).reshape(B, T, C), slope)
        r = torch.round(_v(d, B * T).reshape(B, T) * dil).long()
        t = torch.arange(T).unsqueeze(0)
        ov = _v(out, B * T * 3 * C).reshape(B, T, 3 * C)
        ov[:, :, :C] = xv
        for k, idx in ((1, t - r), (2, t + r)):
            ok = ((idx >= 0) & (idx < T)).unsqueeze(-1)
            ov[:, :, k * C:(k + 1) * C] = torch.gather(xv, 1, idx.clamp(0, T - 1).unsqueeze(-1).expand(B, T, C)) * ok
    elif name == "srn_scatter_rows":
        src, src_bs, ld_src, dst, dst_bs, ld_dst, dc0, row_off, n_rows, B, T, C = a
        sv, dv = _v(src), _v(dst)
        ro = None if row_off is None else _v(row_off)
        nr = None if n_rows is None else _v(n_rows)
        for b in range(B):
            off = 0 if ro is None else int(ro[b])
            n = T if nr is None else min(int(nr[b]), T)
            for t in range(n):
                dv[b * dst_bs + (off + t) * ld_dst + dc0: b * dst_bs + (off + t) * ld_dst + dc0 + C] = \
                    sv[b * src_bs + t * ld_src: b * src_bs + t * ld_src + C]
    elif name == "srn_pad_signal":
        x, out, B, n, pad, ld, mode = a
        xv = _v(x, B * n).reshape(B, n)
        ov = _v(out, B * ld).reshape(B, ld)
        ov[:] = 0
        ov[:, :n + 2 * pad] = F.pad(xv.unsqueeze(1), (pad, pad), mode="constant" if mode else "reflect").squeeze(1)
    elif name == "srn_logmel":
        spec, mel_t, out, frames, nb, ld, n_mels, eps, mode = a
        sv = _v(spec, frames * ld).reshape(frames, ld)
        mag = torch.sqrt(sv[:, :nb] ** 2 + sv[:, nb:2 * nb] ** 2)
        m = torch.clamp(mag @ mel_t, min=eps)
        _v(out, frames * n_mels).reshape(frames, n_mels)[:] = {10: torch.log10, 2: torch.log2, 0: torch.log}[mode](m)
    elif name == "srn_loudness":
        spec, aw, ws, out, B, frames, nb, ld, amin, top_db, add_eps = a
        sv = _v(spec, B * frames * ld).reshape(B, frames, ld)
        p = sv[..., :nb] ** 2 + sv[..., nb:2 * nb] ** 2
        db = 10 * torch.log10(torch.clamp(p, min=amin))
        db = torch.maximum(db, db.amax(dim=(1, 2), keepdim=True) - top_db) + aw
        _v(out, B * frames).reshape(B, frames)[:] = torch.log(torch.pow(10.0, 0.05 * db).mean(dim=-1) + add_eps)
    elif name == "srn_gru_recur_last":
        gi_all, whh_t, bhh, h, B, T, H = a
        gv = _v(gi_all, B * T * 3 * H).reshape(B, T, 3 * H)
        hh = torch.zeros(B, H)
        for t in range(T):
            gi, gh = gv[:, t], hh @ whh_t + bhh
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            hh = (1 - z) * n + z * hh
        _v(h, B * H).reshape(B, H)[:] = hh
    elif name == "srn_style_token_attention_kv":
        ref, wq_t, bq, k, v, wo_t, bo, out, B, Dq, n_tok, Fd, nh = a
        q = _v(ref, B * Dq).reshape(B, Dq) @ wq_t + bq
        dk = Fd // nh
        sc = torch.einsum("bhd,thd->bht", q.view(B, nh, dk), k.view(n_tok, nh, dk)) / math.sqrt(dk)
        ctx = torch.einsum("bht,thd->bhd", torch.softmax(sc, -1), v.view(n_tok, nh, dk)).reshape(B, Fd)
        _v(out, B * Fd).reshape(B, Fd)[:] = ctx @ wo_t + bo
    elif name == "srn_rowln_fwd":
        x, m, m_bs, a_, a_bs, y, B, T, C, eps = a
        xv = _v(x, B * T * C).reshape(B, T, C)
        mv = _v(m).reshape(-1)[: (B if m_bs else 1) * C].reshape(-1, C)
        av = _v(a_).reshape(-1)[: (B if a_bs else 1) * C].reshape(-1, C)
        _v(y, B * T * C).reshape(B, T, C)[:] = F.layer_norm(xv, (C,), None, None, eps) * mv.unsqueeze(1) + av.unsqueeze(1)
    elif name == "srn_rowln_bwd":
        x, dy, m, m_bs, dx, part, B, T, C, eps = a
        xv = _v(x, B * T * C).reshape(B, T, C).clone().requires_grad_(True)
        dv = _v(dy, B * T * C).reshape(B, T, C)
        mv = _v(m).reshape(-1)[: (B if m_bs else 1) * C].reshape(-1, C)
        with torch.enable_grad():
            xh = F.layer_norm(xv, (C,), None, None, eps)
            (xh * mv.unsqueeze(1)).backward(dv)
        _v(dx, B * T * C).reshape(B, T, C)[:] = xv.grad
        R = training.NORM_BWD_ROWS
        nch = (T + R - 1) // R
        pv = _v(part, B * nch * 2 * C).reshape(B, nch, 2, C)
        xh = xh.detach()
        for c in range(nch):
            sl = slice(c * R, min(T, (c + 1) * R))
            pv[:, c, 0] = (dv[:, sl] * xh[:, sl]).sum(1)
            pv[:, c, 1] = dv[:, sl].sum(1)
    elif name in ("srn_gn_mish_bwd_partial", "srn_gn_mish_bwd_apply"):
        if name.endswith("partial"):
            h, dy, mean, rstd, gamma, beta, lens, out, B, T, C, G = a
        else:
            h, dy, mean, rstd, gamma, beta, gsum, lens, out, B, T, C, G = a
        hv, dv = (_v(t, B * T * C).reshape(B, T, C) for t in (h, dy))
        mu = _v(mean, B * G).reshape(B, 1, G).repeat_interleave(C // G, dim=2)
        rs = _v(rstd, B * G).reshape(B, 1, G).repeat_interleave(C // G, dim=2)
        xh = (hv - mu) * rs
        gpre = (xh * gamma + beta).clone().requires_grad_(True)
        with torch.enable_grad():
            F.mish(gpre).backward(torch.ones_like(gpre))
        valid = (torch.arange(T)[None, :, None] < (_v(lens, B).reshape(B, 1, 1) if lens is not None else T)).float()
        dg = dv * gpre.grad * valid
        if name.endswith("partial"):
            R = training.NORM_BWD_ROWS
            nch = (T + R - 1) // R
            pv = _v(out, B * nch * 2 * C).reshape(B, nch, 2, C)
            for c in range(nch):
                sl = slice(c * R, min(T, (c + 1) * R))
                pv[:, c, 0] = dg[:, sl].sum(1)
                pv[:, c, 1] = (dg[:, sl] * xh[:, sl]).sum(1)
        else:
            n = float(T * (C // G))
            gs = _v(gsum, B * G * 2).reshape(B, G, 2)
            A = gs[:, :, 0].reshape(B, 1, G).repeat_interleave(C // G, dim=2) / n
            Bq = gs[:, :, 1].reshape(B, 1, G).repeat_interleave(C // G, dim=2) / n
            _v(out, B * T * C).reshape(B, T, C)[:] = rs * (dg * gamma - A - xh * Bq)
    elif name == "srn_gn_stats":
        part, mean, rstd, B, T, C, G, eps = a
        mv, rv = _v(mean, B * G).reshape(B, G), _v(rstd, B * G).reshape(B, G)
        for b in range(B):
            mv[b], rv[b] = _group_stats(part, b, T, C, G, eps)
    elif name == "srn_bn_relu_fwd":
        x, gamma, beta, rm, rv, part, stats, y, rows, C, eps, mom = a
        xv = _v(x, rows * C).reshape(rows, C).double()
        mean, var = xv.mean(0), xv.var(0, unbiased=False)
        sv = _v(stats, 2 * C).reshape(2, C)
        sv[0], sv[1] = mean.float(), (1.0 / torch.sqrt(var + eps)).float()
        _v(y, rows * C).reshape(rows, C)[:] = torch.relu((xv - mean) / torch.sqrt(var + eps) * _v(gamma, C).double()
                                                         + _v(beta, C).double()).float()
        if rm is not None:
            unb = var * (rows / (rows - 1)) if rows > 1 else var
            _v(rm, C)[:] = ((1 - mom) * _v(rm, C).double() + mom * mean).float()
            _v(rv, C)[:] = ((1 - mom) * _v(rv, C).double() + mom * unb).float()
    elif name == "srn_bn_relu_bwd":
        x, y, dy, stats, gamma, part, sums, dx, rows, C = a
        xv, yv, gv = (_v(t, rows * C).reshape(rows, C).double() for t in (x, y, dy))
        sv = _v(stats, 2 * C).reshape(2, C).double()
        g = gv * (yv > 0)
        xhat = (xv - sv[0]) * sv[1]
        s0, s1 = g.sum(0), (g * xhat).sum(0)
        ov = _v(sums, 2 * C).reshape(2, C)
        ov[0], ov[1] = s0.float(), s1.float()
        _v(dx, rows * C).reshape(rows, C)[:] = (_v(gamma, C).double() * sv[1] * (g - (s0 + xhat * s1) / rows)).float()
    elif name in ("srn_im2col_s2", "srn_col2im_s2"):
        src, dst, B, H, W, C, ld = a
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        if name == "srn_im2col_s2":
            xv = F.pad(_v(src, B * H * W * C).reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
            cv = _v(dst, B * Ho * Wo * ld).reshape(B, Ho, Wo, ld)
            for kh in range(3):
                for kw in range(3):
                    k = kh * 3 + kw
                    cv[..., k * C:(k + 1) * C] = xv[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][:, :Ho, :Wo]
        else:
            cv = _v(src, B * Ho * Wo * ld).reshape(B, Ho, Wo, ld)
            acc = torch.zeros(B, H + 2, W + 2, C)
            for kh in range(3):
                for kw in range(3):
                    k = kh * 3 + kw
                    acc[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][:, :Ho, :Wo] += cv[..., k * C:(k + 1) * C]
            _v(dst, B * H * W * C).reshape(B, H, W, C)[:] = acc[:, 1:H + 1, 1:W + 1]
    elif name == "srn_gru_train_fwd":
        gi, w_hh_t, b_hh, hs, gates, B, T, H = a
        giv = _v(gi, B * T * 3 * H).reshape(B, T, 3 * H)
        wt, bh = _v(w_hh_t, H * 3 * H).reshape(H, 3 * H), _v(b_hh, 3 * H)
        hv, gv = _v(hs, B * (T + 1) * H).reshape(B, T + 1, H), _v(gates, B * T * 4 * H).reshape(B, T, 4 * H)
        hv[:, 0] = 0
        for t in range(T):
            gh = hv[:, t] @ wt + bh
            r = torch.sigmoid(giv[:, t, :H] + gh[:, :H])
            z = torch.sigmoid(giv[:, t, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(giv[:, t, 2 * H:] + r * gh[:, 2 * H:])
            hv[:, t + 1] = (1 - z) * n + z * hv[:, t]
            gv[:, t] = torch.cat([r, z, n, gh[:, 2 * H:]], dim=1)
    elif name == "srn_gru_train_bwd":
        dh_last, w_hh, hs, gates, dgi, dgh, B, T, H = a
        w = _v(w_hh, 3 * H * H).reshape(3 * H, H)
        hv, gv = _v(hs, B * (T + 1) * H).reshape(B, T + 1, H), _v(gates, B * T * 4 * H).reshape(B, T, 4 * H)
        di, dg = _v(dgi, B * T * 3 * H).reshape(B, T, 3 * H), _v(dgh, B * T * 3 * H).reshape(B, T, 3 * H)
        d = _v(dh_last, B * H).reshape(B, H).clone()
        for t in range(T - 1, -1, -1):
            r, z, n, ghn = gv[:, t, :H], gv[:, t, H:2 * H], gv[:, t, 2 * H:3 * H], gv[:, t, 3 * H:]
            dn = d * (1 - z) * (1 - n * n)
            dz = d * (hv[:, t] - n) * z * (1 - z)
            dr = dn * ghn * r * (1 - r)
            di[:, t] = torch.cat([dr, dz, dn], dim=1)
            dg[:, t] = torch.cat([dr, dz, dn * r], dim=1)
            d = d * z + dg[:, t] @ w
    elif name == "srn_token_attn_fwd":
        q, k, v, p, ctx, B, n_tok, F_, nh = a
        dk = F_ // nh
        qv = _v(q, B * F_).reshape(B, nh, dk)
        kv, vv = _v(k, n_tok * F_).reshape(n_tok, nh, dk), _v(v, n_tok * F_).reshape(n_tok, nh, dk)
        pr = torch.softmax(torch.einsum("bhd,thd->bht", qv, kv) / math.sqrt(dk), dim=-1)
        _v(p, B * nh * n_tok).reshape(B, nh, n_tok)[:] = pr
        _v(ctx, B * F_).reshape(B, nh, dk)[:] = torch.einsum("bht,thd->bhd", pr, vv)
    elif name == "srn_token_attn_bwd":
        dctx, q, k, v, p, dq, dkp, dvp, B, n_tok, F_, nh = a
        dk = F_ // nh
        dc, qv = _v(dctx, B * F_).reshape(B, nh, dk), _v(q, B * F_).reshape(B, nh, dk)
        kv, vv = _v(k, n_tok * F_).reshape(n_tok, nh, dk), _v(v, n_tok * F_).reshape(n_tok, nh, dk)
        pr = _v(p, B * nh * n_tok).reshape(B, nh, n_tok)
        dp = torch.einsum("bhd,thd->bht", dc, vv)
        ds = pr * (dp - (pr * dp).sum(-1, keepdim=True)) / math.sqrt(dk)
        _v(dq, B * F_).reshape(B, nh, dk)[:] = torch.einsum("bht,thd->bhd", ds, kv)
        _v(dkp, B * n_tok * F_).reshape(B, n_tok, nh, dk)[:] = torch.einsum("bht,bhd->bthd", ds, qv)
        _v(dvp, B * n_tok * F_).reshape(B, n_tok, nh, dk)[:] = torch.einsum("bht,bhd->bthd", pr, dc)
    elif name == "srn_colsum":
        x, part, out, B, R, N, ld = a
        _v(out, B * N).reshape(B, N)[:] = _v(x, B * R * ld).reshape(B, R, ld)[:, :, :N].sum(1)
    elif name == "srn_chunk_colsum":
        part, gamma, col, gsum, B, nch, C, G = a
        pv = _v(part, B * nch * 2 * C).reshape(B, nch, 2, C)
        cv = _v(col, B * 2 * C).reshape(B, 2, C)
        cv[:] = pv.sum(1)
        if gsum is not None:
            _v(gsum, B * G * 2).reshape(B, G, 2)[:] = (cv * gamma).reshape(B, 2, G, C // G).sum(-1).transpose(1, 2)
    elif name == "srn_softmax_bwd":
        pm, dp, rows, L, ld, scale = a
        pv = _v(pm, rows * ld).reshape(rows, ld)[:, :L]
        dv = _v(dp, rows * ld).reshape(rows, ld)
        g = dv[:, :L].clone()
        dv[:, :L] = scale * pv * (g - (g * pv).sum(-1, keepdim=True))
    elif name == "srn_geglu_fwd":
        hg, out, rows, inner = a
        hv = _v(hg, rows * 2 * inner).reshape(rows, 2 * inner)
        _v(out, rows * inner).reshape(rows, inner)[:] = hv[:, :inner] * F.gelu(hv[:, inner:])
    elif name == "srn_geglu_bwd":
        hg, da, dhg, rows, inner = a
        hv = _v(hg, rows * 2 * inner).reshape(rows, 2 * inner).clone().requires_grad_(True)
        with torch.enable_grad():
            (hv[:, :inner] * F.gelu(hv[:, inner:])).backward(_v(da, rows * inner).reshape(rows, inner))
        _v(dhg, rows * 2 * inner).reshape(rows, 2 * inner)[:] = hv.grad
    elif name == "srn_dot":
        x, y, n, part = a
        pv = _v(part)[:_sumsq_blocks(n)]  # the entries past srn_sumsq_blocks(n) are the caller's
        pv.zero_()
        pv[0] = (_v(x, n).double() * (1.0 if y is None else _v(y, n).double())).sum()
    elif name == "srn_sumsq":
        g, n, part = a
        pv = _v(part)[:_sumsq_blocks(n)]
        pv.zero_()
        pv[0] = (_v(g, n).double() ** 2).sum()
    elif name == "srn_adamw_dyn":
        pp, g, m, v, n, b1, b2, eps, wd, dyn = a
        b1, b2, eps, wd = (_c_float(x) for x in (b1, b2, eps, wd))
        lr, bc1, bc2, gscale = (float(x) for x in _v(dyn, 4))
        pv, gv, mv, vv = (_v(t, n) for t in (pp, g, m, v))
        gi = gv * gscale
        pv.mul_(1 - lr * wd)
        mv.mul_(b1).add_(gi, alpha=1 - b1)
        vv.mul_(b2).addcmul_(gi, gi, value=1 - b2)
        pv.addcdiv_(mv / bc1, (vv / bc2).sqrt() + eps, value=-lr)
    elif name == "srn_adamw":
        pp, g, m, v, n, lr, b1, b2, eps, wd, step, gscale = a
        lr, b1, b2, eps, wd, gscale = (_c_float(x) for x in (lr, b1, b2, eps, wd, gscale))
        pv, gv, mv, vv = (_v(t, n) for t in (pp, g, m, v))
        gi = gv * gscale
        pv.mul_(1 - lr * wd)
        mv.mul_(b1).add_(gi, alpha=1 - b1)
        vv.mul_(b2).addcmul_(gi, gi, value=1 - b2)
        pv.addcdiv_(mv / (1 - b1 ** step), (vv / (1 - b2 ** step)).sqrt() + eps, value=-lr)
    else:
        raise NotImplementedError(name)


def emul_resunit(kw):
    """srn_hifigan_resunit: y = conv2(lrelu(conv1(lrelu(x)))) + x [+ res2] [/ post_div], channels-last views; items
    x_bs / res2_bs / out_bs apart (T * C unless given)"""
    g = kw.get
    B, T, C, k, d, slope = g("n_batch"), g("T"), g("C"), g("k"), g("dilation"), g("slope")

    def items(t, bs):  # (B, T, C) view of a tensor or (tensor, offset) with its batch stride
        f, o = _flat(t)
        return torch.as_strided(f, (B, T, C), (bs or T * C, C, 1), o + f.storage_offset())

    x = items(g("x"), g("x_bs"))
    w1 = g("w1").reshape(C, k, C).permute(0, 2, 1)  # packed [C_out][k][C_in] -> torch (C_out, C_in, k)
    w2 = g("w2").reshape(C, k, C).permute(0, 2, 1)
    xt = F.conv1d(F.leaky_relu(x.transpose(1, 2), slope), w1, g("b1"), padding=(k - 1) // 2 * d, dilation=d)
    xt = F.conv1d(F.leaky_relu(xt, slope), w2, g("b2"), padding=(k - 1) // 2)
    y = xt.transpose(1, 2) + x
    if g("res2") is not None:
        y = y + items(g("res2"), g("res2_bs"))
    if g("post_div", 0.0) not in (0.0, 1.0):
        y = y / g("post_div")
    items(g("out"), g("out_bs"))[:] = y


def emul_tn_gemm(kw):
    """executable spec of srn_tn_gemm; keywords the caller left out take the defaults of ops.TnGemmOp._fill"""
    g = {**{k: p.default for k, p in inspect.signature(ops.TnGemmOp._fill).parameters.items()}, **kw}.get
    a, oa = _flat(g("a"))
    b, ob = _flat(g("b"))
    out, oo = _flat(g("out"))
    oa, ob, oo = oa + a.storage_offset(), ob + b.storage_offset(), oo + out.storage_offset()  # as_strided counts from the storage
    M, N, T_a, T_b, stride = g("M"), g("N"), g("T_a"), g("T_b"), g("stride")
    len_b, colsum = g("len_b"), g("colsum")
    if colsum is not None:
        assert g("n_batch") == 1 and g("n_head") == 1 and M % 4 == 0, "colsum: one problem, M % 4 == 0"
        cs = torch.zeros(M, dtype=torch.float64)
        for it in range(g("n_items")):
            i1, i2 = divmod(it, max(1, g("n_inner", 1)))
            cs += torch.as_strided(a, (T_a, M), (g("lda"), 1), oa + i1 * g("a_is") + i2 * g("a_is2", 0)).double().sum(0)
        colsum.view(-1)[:M] = (cs * g("alpha")).float()
    for zb in range(g("n_batch")):
        for zh in range(g("n_head")):
            for j, sh in enumerate(g("shifts")):
                acc = torch.zeros(M, N, dtype=torch.float64)
                ninner = max(1, g("n_inner", 1))
                for it in range(g("n_items")):
                    i1, i2 = divmod(it, ninner)
                    a0 = oa + zb * g("a_bs") + zh * g("a_hs") + i1 * g("a_is") + i2 * g("a_is2", 0)
                    b0 = ob + zb * g("b_bs") + zh * g("b_hs") + i1 * g("b_is") + i2 * g("b_is2", 0)
                    am = torch.as_strided(a, (T_a, M), (g("lda"), 1), a0).double()
                    tb = torch.arange(T_a) * stride + sh
                    end = T_b
                    if len_b is not None:
                        assert ninner == 1, "len_b: one-level items"
                        end = min(T_b, int(len_b.view(-1)[zb * g("n_items") + it]))
                    ok = (tb >= 0) & (tb < end)
                    rows = torch.as_strided(b, (T_b, N), (g("ldb"), 1), b0).double()[tb.clamp(0, T_b - 1)]
                    # (a select, not a product: whatever the rows outside [0, end) hold, they count as zero)
                    acc += am.t() @ torch.where(ok[:, None], rows, torch.zeros((), dtype=torch.float64))
                o0 = oo + zb * g("out_bs") + zh * g("out_hs") + j * N
                torch.as_strided(out, (M, N), (g("ldc"), 1), o0).copy_((acc * g("alpha")).float())


def emul_multi_copy(self_, stream=None):
    flat = self_.dst.view(-1)
    for t, o in zip(self_.srcs, self_.offs):
        flat[o:o + t.numel()] = t.reshape(-1)


def emul_transpose_multi(self_, stream=None):
    """executable spec of srn_transpose_multi: entry e does dst[b][c][r] = src[b][r][c]"""
    for src, dst, B, R, Cc, sbs, lds, dbs, ldd in self_.entries:
        (sf, so), (df, do) = _flat(src), _flat(dst)
        # (as_strided offsets count from the storage, and parameters are views into the flat buffer)
        torch.as_strided(df, (B, Cc, R), (dbs, ldd, 1), do + df.storage_offset()).copy_(
            torch.as_strided(sf, (B, R, Cc), (sbs, lds, 1), so + sf.storage_offset()).transpose(1, 2))


class installed:
    """context manager: route every op through the emulator and lift the CUDA-only guard"""

    def __enter__(self):
        from serenade_amd import features, sifigan, training
        self._mods = (models, vocoder, sifigan, features, training)
        self._saved = (ops.ConvOp.__call__, ops.CallOp.__call__, [m._require_cuda for m in self._mods],
                       ops.ResUnitOp.__call__)
        self._saved_mc = ops.MultiCopyOp.__call__
        ops.MultiCopyOp.__call__ = emul_multi_copy
        self._saved_tm = ops.TransposeMultiOp.__call__
        ops.TransposeMultiOp.__call__ = emul_transpose_multi
        self._saved_tn = ops.TnGemmOp.__call__
        ops.TnGemmOp.__call__ = lambda self_, stream=None: emul_tn_gemm(self_.kw)
        ops.ConvOp.__call__ = lambda self_, stream=None: emul_conv(self_.kw)
        ops.ResUnitOp.__call__ = lambda self_, stream=None: emul_resunit(self_.kw)
        ops.CallOp.__call__ = lambda self_, stream=None: emul_call(self_.name, self_.targs)
        for m in self._mods:
            m._require_cuda = lambda *a, **k: None
        return self

    def __exit__(self, *exc):
        ops.ConvOp.__call__, ops.CallOp.__call__, guards, ops.ResUnitOp.__call__ = self._saved
        ops.MultiCopyOp.__call__ = self._saved_mc
        ops.TransposeMultiOp.__call__ = self._saved_tm
        ops.TnGemmOp.__call__ = self._saved_tn
        for m, g in zip(self._mods, guards):
            m._require_cuda = g
