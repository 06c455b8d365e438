"""The transcriber's whole plan (buffers, strides, tap tables, padding, weight packing) run on the CPU through the C-ABI
emulator (tests/_emulator.py, plus CPU statements of the five transcriber entry points below), against the reference's
own logits in tests/golden/transcriber_small.npz.  Host logic only: the kernels themselves are checked on the GPU."""
import json

import numpy as np
import torch

from serenade_amd import transcriber as tr
from tests import _emulator as E


def _tview(x, B, rows, ld, bs, width=None):
    """(B, rows, width or ld) view, row stride ld, item stride bs, of a tensor / (tensor, element offset)"""
    t, off = E._flat(x)
    return torch.as_strided(t, (B, rows, ld if width is None else width), (bs, ld, 1), t.storage_offset() + off)


def emul_transcriber(name, a):
    if name == "srn_pad_ragged":
        x, x_bs, lens, out, B, n, pad, ld = a
        xv, ov = _tview(x, B, 1, n, x_bs)[:, 0], _tview(out, B, 1, ld, ld)[:, 0]
        for b in range(B):
            L = min(int(lens[b]), n)
            i = torch.arange(L + 2 * pad) - pad
            i = torch.where(i < 0, -i, i)
            i = torch.where(i >= L, 2 * (L - 1) - i, i)
            ov[b] = 0
            ov[b, :L + 2 * pad] = xv[b, i]
    elif name == "srn_mel_db":
        spec, ld_spec, nb, mel_t, lens, gmax, out, ld_out, B, T, n_mels, amin, top_db = a
        sv, ov = _tview(spec, B, T, ld_spec, T * ld_spec), _tview(out, B, T, ld_out, T * ld_out)
        for b in range(B):
            L = min(int(lens[b]), T)
            ov[b, :, :n_mels] = 0
            if L == 0:
                continue
            p = sv[b, :L, :nb] ** 2 + sv[b, :L, nb:2 * nb] ** 2
            db = 10 * torch.log10(torch.clamp(p @ E._v(mel_t, nb * n_mels).view(nb, n_mels), min=amin))
            ov[b, :L, :n_mels] = torch.max(db, db.max() - top_db)
    elif name == "srn_trans_conv0":
        x, x_bs, ld_x, lens, w, bias, out, B, T, Fq, C, dil = a
        xv = _tview(x, B, T, ld_x, x_bs)
        ov = _tview(out, B, T, (Fq + 2) * C, T * (Fq + 2) * C).view(B, T, Fq + 2, C)
        for b in range(B):
            L = min(int(lens[b]), T)
            ov[b] = 0
            if L == 0:
                continue
            y = torch.nn.functional.conv2d(xv[b, :L, :Fq][None, None], E._v(w, C * 9).view(C, 1, 3, 3), E._v(bias, C),
                                           padding=(dil, 1), dilation=(dil, 1))[0]
            ov[b, :L, 1:Fq + 1] = torch.relu(y).permute(1, 2, 0)
    elif name == "srn_trans_pool":
        x, lens, out, B, T, Fin, C, Cv, flatten, ld_out = a
        Fo = Fin // 2
        xv = _tview(x, B, T, (Fin + 2) * C, T * (Fin + 2) * C).view(B, T, Fin + 2, C)
        pooled = torch.maximum(xv[:, :, 1:2 * Fo + 1:2], xv[:, :, 2:2 * Fo + 2:2])  # (B, T, Fo, C)
        if flatten:
            ov = _tview(out, B, T, ld_out, T * ld_out)
            ov.zero_()
            ov[:, :, :Cv * Fo] = pooled[..., :Cv].permute(0, 1, 3, 2).reshape(B, T, Cv * Fo)
        else:
            ov = _tview(out, B, T, (Fo + 2) * C, T * (Fo + 2) * C).view(B, T, Fo + 2, C)
            ov.zero_()
            ov[:, :, 1:Fo + 1] = pooled
        for b in range(B):
            ov[b, min(int(lens[b]), T):] = 0
    elif name == "srn_bilstm_recur":
        g, g_bs, ld_g, lens, w_t, out, out_bs, ld_out, B, T, H = a
        gv, ov = _tview(g, B, T, ld_g, g_bs), _tview(out, B, T, ld_out, out_bs, 2 * H)
        W = w_t.view(2, H, H, 4)
        for b in range(B):
            L = min(int(lens[b]), T)
            ov[b] = 0
            for d in range(2):
                h, c = torch.zeros(H), torch.zeros(H)
                Wd = W[d].permute(2, 1, 0).reshape(4 * H, H)  # back to W_hh
                for t in (range(L - 1, -1, -1) if d else range(L)):
                    z = gv[b, t, d * 4 * H:(d + 1) * 4 * H] + Wd @ h
                    i, f, gg, o = z.view(4, H)
                    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
                    h = torch.sigmoid(o) * torch.tanh(c)
                    ov[b, t, d * H:(d + 1) * H] = h
    else:
        return E.emul_call(name, a)


def test_plan_on_the_emulator_matches_the_reference(golden):
    d = golden("transcriber_small")
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    m = tr.TranscriptionModel(cfg, device="cpu").load_state_dict(sd)
    n0, n1 = len(d["wave0"]), len(d["wave1"])
    with E.installed():  # restores CallOp.__call__ on exit
        tr.ops.CallOp.__call__ = lambda self_, stream=None: emul_transcriber(self_.name, self_.targs)
        plan = tr._Plan(m, torch.device("cpu"), 2, n0, [n0, n1])
        plan.wave[0] = torch.from_numpy(d["wave0"])
        plan.wave[1] = 5.0  # padding never reaches a valid frame
        plan.wave[1, :n1] = torch.from_numpy(d["wave1"])
        for op in plan.ops:
            op()
    for i in range(2):
        ref, T = d[f"ref{i}"], d[f"ref{i}"].shape[0]
        for got, want in ((plan.logits[i, :T, :3], ref), (plan.phon[i, :T, :tr.N_PHONEMES], d[f"phon{i}"])):
            err = (got.double() - torch.from_numpy(want).double()).abs()
            scale = np.abs(want).max()
            assert err.max().item() <= 1e-4 * scale and err.pow(2).mean().sqrt().item() <= 1e-5 * scale, i
