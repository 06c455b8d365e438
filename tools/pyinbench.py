#!/usr/bin/env python3
"""Developer tool (GPU): time of pYIN (serenade_amd/pitch.py) on B utterances of `seconds` s at the transcriber's
settings (16 kHz, frame 1024, hop 320, 65-2093 Hz), warm, with HIP events: the whole call and the two kernels
(srn_pyin_observe, srn_pyin_viterbi) on their own.  Next to it, the float64 CPU restatement tests/_pyin_ref.py on
`cpu_items` of the utterances (its per-utterance time, scaled to B), and librosa.pyin if it is installed.  The signals
are seeded harmonic note sequences with silences and a little noise.  Prints one JSON line.

    python tools/pyinbench.py [B=8] [seconds=10] [cpu_items=1]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from serenade_amd import pitch  # noqa: E402
from tests import _pyin_ref as R  # noqa: E402

KW = dict(fmin=65, fmax=2093, sr=16000, frame_length=1024, hop_length=320)


def signals(B, seconds, sr=16000, seed=0):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    out = []
    for b in range(B):
        notes = 110.0 * 2 ** (rng.integers(0, 36, size=int(seconds * 3) + 1) / 12)
        notes[rng.random(len(notes)) < 0.2] = 0.0
        f = np.repeat(notes, -(-n // len(notes)))[:n]
        ph = 2 * np.pi * np.cumsum(np.where(f > 0, f, 100.0)) / sr
        y = sum(0.3 / k * np.sin(k * ph) for k in range(1, 6)) * (f > 0)
        out.append((y + 1e-3 * rng.standard_normal(n)).astype(np.float32))
    return np.stack(out)


def gpu_ms(fn, reps=20):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e))
    return best


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    sec = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    cpu_items = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    assert torch.cuda.is_available(), "pyinbench needs an MI355X"
    y = signals(B, sec)
    x = torch.from_numpy(y).to("cuda:0")
    lens = [y.shape[1]] * B
    for _ in range(3):  # warm: plan, code objects
        pitch.pyin(x, lens, **KW)
    torch.cuda.synchronize()
    plan = next(iter(pitch._PLANS.values()))  # the one plan the warm-up made
    stream = torch.cuda.current_stream().cuda_stream
    res = dict(tool="pyinbench", B=B, seconds=sec, frames=plan.T, states=2 * plan.g["n_bins"])
    res["gpu_call_ms"] = gpu_ms(lambda: pitch.pyin(x, lens, **KW))
    res["gpu_observe_ms"] = gpu_ms(lambda: plan.observe(x, stream))
    res["gpu_viterbi_ms"] = gpu_ms(lambda: plan.viterbi(stream))
    t0 = time.perf_counter()
    for b in range(cpu_items):
        R.pyin(y[b], **KW)
    per = (time.perf_counter() - t0) / cpu_items
    res["cpu_restatement_s_per_item"] = per
    res["cpu_restatement_s_batch_est"] = per * B
    try:
        import librosa
        t0 = time.perf_counter()
        for b in range(cpu_items):
            librosa.pyin(y[b].astype(np.float64), fill_na=np.nan, center=True, **KW)
        res["librosa_s_per_item"] = (time.perf_counter() - t0) / cpu_items
    except ImportError:
        res["librosa_s_per_item"] = None
    res["speedup_vs_restatement"] = res["cpu_restatement_s_batch_est"] * 1e3 / res["gpu_call_ms"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
