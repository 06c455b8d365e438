#!/usr/bin/env python3
"""Developer tool (GPU): throughput of the feature front-end -- log-mel (fft 512 / win 480 / hop 240 /
80 mels, conf/serenade.yaml:4-21) and A-weighted loudness (n_fft 2048) of B utterances of T frames.  Prints one JSON
object.  (The comparison with the numpy restatement, values and host timing, is tests/test_features.py: only tests may
use oracle/.)

    featbench.py B T                      B equal utterances of T frames, one dense call per function
    featbench.py B T --ragged             B utterances of distinct lengths spread over 0.5 .. 1.0 x T frames:
                                          (a) one call per function with lengths=, (b) the loop of per-item dense calls
                                          over the same items; each with its plans warm, and over a fresh set of lengths
                                          per pass (a corpus: no two batches share their lengths, every plan is new)
    featbench.py B T --ragged --loop-only (b) alone, which also runs on a build whose calls take no lengths="""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serenade_amd import features  # noqa: E402

SR, HOP = 24000, 240
KW = dict(fft_size=512, hop_size=HOP, win_length=480, num_mels=80, fmin=63, fmax=12000)


def _timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def dense(B, T):
    n = T * HOP
    rng = np.random.default_rng(0)
    audio = (rng.standard_normal((B, n)) * 0.1).astype(np.float32)
    a = torch.from_numpy(audio).cuda()
    out = {"workload": f"B={B} utterances x {T} frames ({n / SR:.2f} s each at 24 kHz)"}
    for name, fn in (("logmel", lambda: features.logmelfilterbank(a, SR, **KW)),
                     ("loudness", lambda: features.loudness_extract(a, SR, HOP))):
        dt = _timed(fn, 3, 20)
        out[name] = {"ms": dt * 1e3, "frames_per_s": B * (1 + n // HOP) / dt, "x_realtime": B * n / SR / dt}
    return out


def ragged_lengths(B, T, shift=0):
    """B distinct sample counts, their frame counts spread evenly over 0.5 .. 1.0 x T, none on the hop grid; `shift`
    moves every one of them (by less than a hop per unit) to a set that shares no length with another shift's"""
    fr = [round(T * (0.5 + 0.5 * b / max(B - 1, 1))) for b in range(B)]
    return [f * HOP + 1 + (7 * b + 3 * shift) % (HOP - 1) for b, f in enumerate(fr)]


def ragged(B, T, loop_only=False, passes=5):
    rng = np.random.default_rng(0)
    n_top = (T + 1) * HOP
    a = torch.from_numpy((rng.standard_normal((B, n_top)) * 0.1).astype(np.float32)).cuda()
    lens = ragged_lengths(B, T)
    assert len(set(lens)) == B
    frames = sum(1 + n // HOP for n in lens)
    out = {"workload": f"B={B} utterances of {min(lens)} .. {max(lens)} samples ({frames} frames, "
                       f"{sum(lens) / SR:.2f} s at 24 kHz), lengths all distinct",
           "plan_lru": 8}
    calls = {"logmel": (lambda x, **k: features.logmelfilterbank(x, SR, **KW, **k)),
             "loudness": (lambda x, **k: features.loudness_extract(x, SR, HOP, **k))}

    def one_call(fn, ln):
        return lambda: fn(a[:, :max(ln)], lengths=ln)

    def loop(fn, ln):
        return lambda: [fn(a[b:b + 1, :n]) for b, n in enumerate(ln)]

    for name, fn in calls.items():
        r = {}
        for label, make in (("ragged_call", one_call), ("per_item_loop", loop)):
            if loop_only and label == "ragged_call":
                continue
            features._PLANS.clear()
            warm = _timed(make(fn, lens), 3, 100)
            # a corpus: every pass has lengths no earlier pass had, so no plan is reused
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(1, passes + 1):
                make(fn, ragged_lengths(B, T, s))()
            torch.cuda.synchronize()
            fresh = (time.perf_counter() - t0) / passes
            r[label] = {"warm_ms": warm * 1e3, "fresh_lengths_ms": fresh * 1e3,
                        "warm_frames_per_s": frames / warm, "fresh_frames_per_s": frames / fresh}
        out[name] = r
    return out


def main():
    args = [v for v in sys.argv[1:] if not v.startswith("--")]
    flags = {v for v in sys.argv[1:] if v.startswith("--")}
    if flags - {"--ragged", "--loop-only"}:
        sys.exit(__doc__)
    B, T = (int(v) for v in (args[:2] + ["8", "1024"][len(args):]))
    out = ragged(B, T, "--loop-only" in flags) if "--ragged" in flags else dense(B, T)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
