#!/usr/bin/env python3
"""Developer tool (GPU): what the note decoding of a batch costs after the transcriber, per utterance on the host
against once on the GPU.  B utterances of `seconds` s of synthetic logits at the transcriber's frame rate (16 kHz, hop
320: 50 frames / s) with about three notes a second, and a pYIN-like contour on the device.

    host loop   what extract_features does per item by default: the device-to-host copy of the item's logits and of
                the contours (reference_f0's), FramewiseDecoder.decode and estimate_score -- wall clock around the
                loop, the device idle before it starts
    device      FramewiseDecoder.decode_batch + estimate_score_batch (srn_note_decode, srn_note_frames), results left
                on the device: HIP events around the two calls, and the wall clock of the same calls up to a
                synchronisation (they are launch-bound)
Both warm, best of `reps`.  Prints one JSON line.

    python tools/notebench.py [B=8] [seconds=10] [reps=20]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from serenade_amd.transcriber import DEFAULT_CONFIG, FramewiseDecoder, estimate_score, estimate_score_batch  # noqa: E402


def batch(B, seconds, rate=50, seed=0):
    """logits (B, T, 3) float32 and contour (B, T) float64: notes of 0.15-0.6 s with short gaps, an onset bump at the
    start of each, an offset bump at its end, frames active inside; the contour holds the note's pitch with vibrato"""
    rng = np.random.default_rng(seed)
    T = int(seconds * rate) + 1
    logits = np.full((B, T, 3), -4.0, dtype=np.float32) + 0.5 * rng.standard_normal((B, T, 3)).astype(np.float32)
    f0 = np.full((B, T), np.nan)
    for b in range(B):
        t = int(rng.integers(2, 10))
        while t < T - 4:
            n = int(rng.integers(8, 30))
            e = min(t + n, T - 3)
            logits[b, t, 0] += 8.0
            logits[b, t + 1, 0] += 5.0
            logits[b, e - 1, 1] += 7.0
            logits[b, t:e, 2] += 8.0
            midi = rng.integers(48, 72) + 0.3 * np.sin(np.arange(e - t) * 0.8)
            f0[b, t + 1:e] = 440.0 * 2.0 ** ((midi[1:] - 69) / 12)
            t = e + int(rng.integers(1, 8))
    return logits, f0


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    sec = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    assert torch.cuda.is_available(), "notebench needs an MI355X"
    cfg = DEFAULT_CONFIG
    dec = FramewiseDecoder(cfg)
    logits_h, f0_h = batch(B, sec)
    T = logits_h.shape[1]
    logits, f0 = torch.from_numpy(logits_h).to("cuda:0"), torch.from_numpy(f0_h).to("cuda:0")
    frames = [T] * B
    n24 = [int(sec * 24000)] * B

    def host_loop():
        contours = f0.cpu().numpy()  # reference_f0's copy
        notes = 0
        for b in range(B):
            p, iv = dec.decode(logits[b, :frames[b]], f0=contours[b, :frames[b]].copy())
            if p:
                estimate_score(p, iv, n24[b], cfg, sampling_rate=24000, shiftms=10)
            notes += len(p)
        return notes

    def device():
        c, iv, p = dec.decode_batch(logits, frames, f0, frames)
        return estimate_score_batch(c, iv, p, n24, cfg, sampling_rate=24000, shiftms=10)

    notes = host_loop()
    for _ in range(3):
        device()
    torch.cuda.synchronize()
    host_ms, dev_wall_ms, dev_event_ms = float("inf"), float("inf"), float("inf")
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_loop()
        host_ms = min(host_ms, (time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        device()
        e.record()
        e.synchronize()
        dev_wall_ms = min(dev_wall_ms, (time.perf_counter() - t0) * 1e3)
        dev_event_ms = min(dev_event_ms, s.elapsed_time(e))
    print(json.dumps(dict(tool="notebench", B=B, seconds=sec, frames=T, notes=notes, pitch_sum=cfg["pitch_sum"],
                          host_loop_ms=host_ms, device_wall_ms=dev_wall_ms, device_event_ms=dev_event_ms)), flush=True)


if __name__ == "__main__":
    main()
