#!/usr/bin/env python3
"""Developer tool (GPU): time of Harvest (serenade_amd/harvest.py) on B utterances of `seconds` s at 24 kHz with
pyworld's defaults (71-800 Hz, 5 ms), warm, with HIP events: the whole call and the five entry points on their own
(srn_harvest_decimate, _channels, _candidates, _refine, _contour).  Next to it, the float64 CPU restatement
tests/_harvest_ref.py on one of the utterances (its time, scaled to B), and pyworld.harvest if it is installed.  The
signals are seeded harmonic note sequences with silences and a little noise.  Prints one JSON line.

    python tools/harvestbench.py [B=8] [seconds=10]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from serenade_amd import harvest as H  # noqa: E402
from tests import _harvest_ref as R  # noqa: E402

FS = 24000


def signals(B, seconds, sr=FS, seed=0):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    out = []
    for b in range(B):
        notes = 110.0 * 2 ** (rng.integers(0, 30, size=int(seconds * 3) + 1) / 12)
        notes[rng.random(len(notes)) < 0.2] = 0.0
        f = np.repeat(notes, -(-n // len(notes)))[:n]
        ph = 2 * np.pi * np.cumsum(np.where(f > 0, f, 100.0)) / sr
        y = sum(0.3 / k * np.sin(k * ph) for k in range(1, 6)) * (f > 0)
        out.append((y + 1e-3 * rng.standard_normal(n)).astype(np.float32))
    return np.stack(out)


def gpu_ms(fn, reps=10):
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
    assert torch.cuda.is_available(), "harvestbench needs an MI355X"
    y = signals(B, sec)
    x = torch.from_numpy(y).to("cuda:0")
    for _ in range(2):  # warm: plan, code objects
        f0, _ = H.harvest(x, FS)
    torch.cuda.synchronize()
    plan = next(iter(H._PLANS.values()))  # the one plan the warm-up made (the batch fits the workspace budget)
    assert plan.B == B, "the batch ran in chunks: lower B or seconds"
    stream = torch.cuda.current_stream().cuda_stream
    res = dict(tool="harvestbench", B=B, seconds=sec, fs=FS, internal_frames=plan.F1, channels=plan.g["n_ch"],
               candidates=plan.g["n_cand"], voiced_fraction=float((f0 > 0).float().mean()))
    res["gpu_call_ms"] = gpu_ms(lambda: H.harvest(x, FS))
    res["gpu_decimate_ms"] = gpu_ms(lambda: plan.decimate(x, stream))
    res["gpu_channels_ms"] = gpu_ms(lambda: plan.channels(stream))
    res["gpu_candidates_ms"] = gpu_ms(lambda: plan.candidates(stream))
    res["gpu_refine_ms"] = gpu_ms(lambda: plan.refine(stream))
    res["gpu_contour_ms"] = gpu_ms(lambda: plan.contour(stream))
    t0 = time.perf_counter()
    ref, _, _ = R.harvest(y[0], FS)
    res["cpu_restatement_s_per_item"] = time.perf_counter() - t0
    res["cpu_restatement_s_batch_est"] = res["cpu_restatement_s_per_item"] * B
    got = f0[0].cpu().numpy()
    res["item0_voiced_flags_equal_restatement"] = bool(np.array_equal(got > 0, ref > 0))
    try:
        import pyworld
        t0 = time.perf_counter()
        pyworld.harvest(y[0].astype(np.float64), FS)
        res["pyworld_s_per_item"] = time.perf_counter() - t0
    except ImportError:
        res["pyworld_s_per_item"] = None
    res["speedup_vs_restatement"] = res["cpu_restatement_s_batch_est"] * 1e3 / res["gpu_call_ms"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
