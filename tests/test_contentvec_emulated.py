"""ContentVec's whole plan (per-layer length tables, ping-pong buffers, the zero padding of V^T, weight packing) run on
the CPU through the C-ABI emulator (tests/_emulator.py, plus CPU statements of the three ContentVec entry points below),
as a ragged batch of the two items of tests/golden/contentvec_small.npz, against transformers' own hidden states in that
fixture and at the GPU test's gate.  Host logic only: the kernels themselves are checked on the GPU."""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

from serenade_amd import contentvec as cvm
from tests import _emulator as E

C0_FRAMES = 64  # frames per partial-sum chunk (srn_frame_stats_chunks)


def _items(x, B, n, bs=None):
    """(B, n) view, item stride bs (n unless given), of a tensor / (tensor, element offset)"""
    t, off = E._flat(x)
    return torch.as_strided(t, (B, n), (n if bs is None else bs, 1), t.storage_offset() + off)


def emul_contentvec(name, a):
    if name == "srn_cvec_conv0":
        wave, wave_bs, n, lens, w, out, parts, B, T0, C, k, stride = a
        chunks = (T0 + C0_FRAMES - 1) // C0_FRAMES
        need = (T0 - 1) * stride + k
        wv = torch.zeros(B, max(need, n))
        wv[:, :n] = _items(wave, B, n, wave_bs)  # samples at or past n read as zero
        ov = _items(out, B, T0 * C).view(B, T0, C)
        pv = _items(parts, B, chunks * C * 2).view(B, chunks, C, 2)
        wk = E._v(w, C * k).reshape(C, 1, k)
        for b in range(B):
            L = min(int(lens[b]), T0)
            ov[b] = 0
            if L:
                ov[b, :L] = F.conv1d(wv[b, :(L - 1) * stride + k].view(1, 1, -1), wk, stride=stride)[0].t()
            v = torch.zeros(chunks * C0_FRAMES, C, dtype=torch.float64)
            v[:T0] = ov[b].double()
            v = v.view(chunks, C0_FRAMES, C)
            pv[b, :, :, 0], pv[b, :, :, 1] = v.sum(1), (v * v).sum(1)
    elif name == "srn_channel_norm_gelu":
        x, parts, chunks, lens, gamma, beta, stats, y, B, T, C, eps = a
        assert chunks == (T + C0_FRAMES - 1) // C0_FRAMES
        xv, yv = _items(x, B, T * C).view(B, T, C), _items(y, B, T * C).view(B, T, C)
        pv = _items(parts, B, chunks * C * 2).view(B, chunks, C, 2)
        sv = _items(stats, B, C * 2).view(B, C, 2)
        for b in range(B):
            L = min(int(lens[b]), T)
            s = pv[b].sum(0)
            mean = s[:, 0] / max(L, 1)
            var = (s[:, 1] / max(L, 1) - mean * mean).clamp_min(0)
            sv[b, :, 0], sv[b, :, 1] = mean.float(), (1.0 / torch.sqrt(var + float(np.float32(eps)))).float()
            o = F.gelu((xv[b, :L] - sv[b, :, 0]) * sv[b, :, 1] * E._v(gamma, C) + E._v(beta, C))
            yv[b, L:] = 0
            yv[b, :L] = o
    elif name == "srn_posconv_gelu_res":
        x, lens, wp, bias, y, B, T, C, G, k, pad = a
        Cg = C // G
        npad = 32 if Cg <= 32 else 64
        w = E._v(wp, G * k * Cg * npad).reshape(G, k, Cg, npad)[..., :Cg].permute(0, 3, 2, 1).reshape(C, Cg, k)
        xv, yv = _items(x, B, T * C).view(B, T, C), _items(y, B, T * C).view(B, T, C)
        for b in range(B):
            L = T if lens is None else min(int(E._v(lens)[b]), T)
            xz = torch.zeros(T, C)
            xz[:L] = xv[b, :L]  # rows at or past the length read as zero
            xp = F.pad(xz, (0, 0, pad, k - 1 - pad)).view(T + k - 1, G, Cg)
            c = torch.zeros(T, G, Cg)
            for j in range(k):  # tap by tap, as the kernel orders its sum: one (T, Cg) x (Cg, Cg) product per group
                c += torch.einsum("tgc,gnc->tgn", xp[j:j + T], w.view(G, Cg, Cg, k)[..., j])
            yv[b] = xv[b] + F.gelu(c.view(T, C) + E._v(bias, C))
    else:
        return E.emul_call(name, a)


def test_plan_on_the_emulator_matches_the_reference(golden):
    d = golden("contentvec_small")
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    m = cvm.ContentVec(device="cpu", **cfg).load_state_dict(sd)
    n0, n1 = len(d["wave0"]), len(d["wave1"])
    n, lens = max(n0, n1), [n0, n1]
    assert n0 != n1 and m.frames(n0) != m.frames(n1)  # a ragged batch: the length tables differ per item and layer
    with E.installed():  # restores CallOp.__call__ on exit
        cvm.ops.CallOp.__call__ = lambda self_, stream=None: emul_contentvec(self_.name, self_.targs)
        plan = cvm._Plan(m, torch.device("cpu"), 2, n, lens)
        plan.wave.fill_(7.0)  # padding never reaches a valid frame
        plan.wave[0, :n0] = torch.from_numpy(d["wave0"])
        plan.wave[1, :n1] = torch.from_numpy(d["wave1"])
        for op in plan.ops:
            op()
    for i, ni in enumerate(lens):
        ref, T = d[f"ref{i}"], m.frames(ni)
        assert ref.shape[0] == T
        err = (plan.out[i, :T].double() - torch.from_numpy(ref).double()).abs()
        scale = np.abs(ref).max()
        mx, rms = err.max().item() / scale, err.pow(2).mean().sqrt().item() / scale
        assert mx <= 2e-5 and rms <= 2e-6, f"item {i}: max {mx:.2e} rms {rms:.2e} of max|ref|"
    assert math.isfinite(float(plan.out.abs().max()))
