#!/usr/bin/env python3
"""Developer tool (GPU): throughput of the MIDI note transcriber (serenade_amd/transcriber.py, DEFAULT_CONFIG geometry
with seeded weights) on B utterances of `seconds` s at 16 kHz, eager and as a replayed hipGraph, with a per-entry
breakdown (LSTM recurrence vs everything else, microseconds per LSTM step).  For comparison it times a torch `nn`
restatement of the same network on the same GPU (fp32, torch.stft front-end), batched and as the reference's B = 1
loop over the items.  Prints one JSON line.

    python tools/transbench.py [B=8] [seconds=10]
"""
import json
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serenade_amd import ops  # noqa: E402
from serenade_amd.transcriber import N_PHONEMES, TranscriptionModel  # noqa: E402


def seeded_state(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in m.state_shapes().items():
        r = torch.randn(shp, generator=g)
        if len(shp) == 4:
            sd[k] = r * math.sqrt(2.0 / (shp[1] * 9))
        elif len(shp) == 2:
            sd[k] = r / math.sqrt(shp[1])
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shp, generator=g)
        elif "cnn" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * r
        else:
            sd[k] = 0.1 * r
    return sd


# ---------------------------------------------------------------------------------------------- torch restatement
class _Stack(nn.Module):
    def __init__(self, F_in, m, dil):
        super().__init__()
        c0, c2 = m // 16, m // 8
        self.cnn = nn.Sequential(
            nn.Conv2d(1, c0, 3, padding=(dil, 1), dilation=(dil, 1)), nn.BatchNorm2d(c0), nn.ReLU(),
            nn.Conv2d(c0, c0, 3, padding=1), nn.BatchNorm2d(c0), nn.ReLU(), nn.MaxPool2d((1, 2)), nn.Identity(),
            nn.Conv2d(c0, c2, 3, padding=1), nn.BatchNorm2d(c2), nn.ReLU(), nn.MaxPool2d((1, 2)))
        self.fc = nn.Sequential(nn.Linear(c2 * (F_in // 4), m))

    def forward(self, x):  # (B, 1, T, F)
        return self.fc(self.cnn(x).transpose(1, 2).flatten(-2))


class _BiLSTM(nn.Module):
    def __init__(self, I, H):
        super().__init__()
        self.rnn = nn.LSTM(I, H, batch_first=True, bidirectional=True)

    def forward(self, x):
        return self.rnn(x)[0]


class _Front(nn.Module):
    def __init__(self, c, mel):
        super().__init__()
        self.n_fft, self.hop = c["win_length"], c["hop_length"]
        self.register_buffer("win", torch.hann_window(self.n_fft))
        self.register_buffer("mel", torch.from_numpy(mel).float())

    def forward(self, x):  # (B, n) -> (B, 1, T, n_mels), top_db per item
        s = torch.stft(x, self.n_fft, self.hop, window=self.win, center=True, pad_mode="reflect", return_complex=True)
        db = 10.0 * torch.log10(torch.clamp(torch.matmul(self.mel, s.abs() ** 2), min=1e-10)).transpose(1, 2)
        return torch.max(db, db.amax(dim=(1, 2), keepdim=True) - 80.0).unsqueeze(1)


class TorchTranscriber(nn.Module):
    def __init__(self, tm):
        super().__init__()
        c, lc = tm.config, tm.config["lang_model_config"]
        m, ml = tm.m, tm.m_lang
        self.front_p, self.front_l = _Front(c, tm.mel_matrix("pitch")), _Front(lc, tm.mel_matrix("lang"))
        self.phon_stack, self.phon_rnn = _Stack(lc["n_mels"], ml, 1), _BiLSTM(ml, ml // 2)
        self.phon_fc = nn.Linear(ml, N_PHONEMES)
        self.pitch_conv_stack, self.lang_conv_stack = _Stack(c["n_mels"], m, 2), _Stack(N_PHONEMES, m, 2)
        self.pitch_rnn, self.lang_rnn = _BiLSTM(m, m // 2), _BiLSTM(m, m // 2)
        self.combined_rnn, self.combined_fc = _BiLSTM(2 * m, m // 2), nn.Linear(m, 3)

    def load(self, sd):
        ren = {"lang_model.conv_stack.": "phon_stack.", "lang_model.rnn.": "phon_rnn.", "lang_model.fc.": "phon_fc."}
        out = {}
        for k, v in sd.items():
            for a, b in ren.items():
                if k.startswith(a):
                    k = b + k[len(a):]
            out[k] = v
        missing, _ = self.load_state_dict(out, strict=False)
        assert all(k.startswith("front_") for k in missing), missing
        return self

    def forward(self, x):
        ph = self.phon_fc(self.phon_rnn(self.phon_stack(self.front_l(x))))
        lang = self.lang_rnn(self.lang_conv_stack(ph.unsqueeze(1)))
        pitch = self.pitch_rnn(self.pitch_conv_stack(self.front_p(x)))
        return self.combined_fc(self.combined_rnn(torch.cat([pitch, lang], -1)))


# ---------------------------------------------------------------------------------------------- timing
def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e))
    return best


def breakdown(plan):
    """eager per-entry times (ms) of one pass, summed per kernel entry point"""
    ev = []
    for op in plan.ops:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        op()
        e.record()
        ev.append((getattr(op, "name", "srn_conv_gemm"), s, e))
    torch.cuda.synchronize()
    per = {}
    for name, s, e in ev:
        per[name] = per.get(name, 0.0) + s.elapsed_time(e)
    return per


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    B = int(args[0]) if args else 8
    seconds = float(args[1]) if len(args) > 1 else 10.0
    dev = torch.device("cuda:0")
    n = int(16000 * seconds)
    tm = TranscriptionModel(device=dev)
    sd = seeded_state(tm)
    tm.load_state_dict(sd)
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(B, n, generator=g)).to(dev)
    T = tm.frames(n)

    ops.set_graphs(False)
    eager_ms = timed(lambda: tm(x))
    plan = next(iter(tm._plans.values()))
    breakdown(plan)  # warm
    per = breakdown(plan)
    ops.set_graphs(True)
    try:
        tm._plans.clear()
        graph_ms = timed(lambda: tm(x), reps=10, warm=3)
    finally:
        ops.set_graphs(False)
    rec_ms = per.get("srn_bilstm_recur", 0.0)
    n_rec = sum(1 for op in plan.ops if getattr(op, "name", "") == "srn_bilstm_recur")

    ref = TorchTranscriber(tm).load(sd).to(dev).eval()
    with torch.no_grad():
        torch_batched_ms = timed(lambda: ref(x), reps=3, warm=1)
        torch_b1_ms = timed(lambda: [ref(x[i:i + 1]) for i in range(B)], reps=3, warm=1)
        diff = (ref(x) - tm(x)[0]).abs().max().item()
    res = {
        "metric": "transcriber_ms_per_batch", "B": B, "seconds": seconds, "frames": T,
        "hip_eager_ms": round(eager_ms, 3), "hip_graph_ms": round(graph_ms, 3),
        "recurrence_ms": round(rec_ms, 3), "rest_ms": round(sum(per.values()) - rec_ms, 3),
        "lstm_recurrences": n_rec, "us_per_lstm_step": round(1000.0 * rec_ms / max(1, n_rec * T), 3),
        "per_entry_ms": {k: round(v, 3) for k, v in sorted(per.items(), key=lambda kv: -kv[1])},
        "torch_batched_ms": round(torch_batched_ms, 3), "torch_b1_loop_ms": round(torch_b1_ms, 3),
        "speedup_vs_torch_b1_loop": round(torch_b1_ms / graph_ms, 2),
        "audio_s_per_s": round(B * seconds / (graph_ms / 1000.0), 1),
        "max_abs_diff_vs_torch_fp32": diff,
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
