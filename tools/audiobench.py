#!/usr/bin/env python3
"""Developer tool (GPU): time of the waveform preparation (serenade_amd/audio.py) on B utterances of `seconds` s, warm,
with HIP events: the three entry points on their own -- srn_resample at 44.1 -> 24 kHz and at 24 -> 16 kHz,
srn_trim_bounds at 2048 / 512, srn_wave_window with a tail pad of 2048 -- and the whole of `prepare` from 44.1 kHz
float64 input (which adds the mono mean, the peak check, two host round trips for the lengths and the allocations).
Next to them, scipy.signal.resample_poly with the same taps on one utterance.  The signals are those of
tools/harvestbench.py between stretches of silence.  Prints one JSON line.

    python tools/audiobench.py [B=8] [seconds=10]
"""
import json
import os
import sys
import time

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from serenade_amd import audio as A  # noqa: E402
from tools.harvestbench import gpu_ms, signals  # noqa: E402

CONFIG = dict(sampling_rate=24000, trim_silence=True, trim_threshold_in_db=60, trim_frame_size=2048,
              trim_hop_size=512, fft_size=2048)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    sec = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    assert torch.cuda.is_available(), "audiobench needs an MI355X"
    y44 = signals(B, sec, sr=44100).astype(np.float64)
    edge = int(0.3 * 44100)
    y44[:, :edge] = 0.0
    y44[:, -edge:] = 0.0
    x44 = torch.from_numpy(y44).to("cuda:0")
    x24, lens24 = A.resample(x44, 44100, 24000, [y44.shape[1]] * B)
    res = dict(tool="audiobench", B=B, seconds=sec, dtype="float64", samples_44k=y44.shape[1], samples_24k=lens24[0],
               taps_44k_to_24k=2 * A.resample_geometry(44100, 24000)[2] + 1,
               taps_24k_to_16k=2 * A.resample_geometry(24000, 16000)[2] + 1)
    for _ in range(2):  # warm: tables, code objects
        A.prepare(x44, 44100, CONFIG)
    torch.cuda.synchronize()
    res["gpu_resample_44k_24k_ms"] = gpu_ms(lambda: A.resample(x44, 44100, 24000, [y44.shape[1]] * B))
    res["gpu_resample_24k_16k_ms"] = gpu_ms(lambda: A.resample(x24, 24000, 16000, lens24))
    res["gpu_trim_bounds_ms"] = gpu_ms(lambda: A.trim_index(x24, 60, 2048, 512, lens24))  # with the read-back
    res["gpu_wave_window_ms"] = gpu_ms(lambda: A.pad_tail(x24, 2048, lens24))
    res["gpu_prepare_ms"] = gpu_ms(lambda: A.prepare(x44, 44100, CONFIG))
    res["trimmed_24k"] = A.prepare(x44, 44100, CONFIG)[1]
    L, M, _ = A.resample_geometry(44100, 24000)
    h = A.resample_taps(44100, 24000)
    t0 = time.perf_counter()
    ref = scipy.signal.resample_poly(y44[0], L, M, window=h / L)
    res["scipy_resample_poly_44k_24k_s_per_item"] = time.perf_counter() - t0
    res["item0_max_diff_vs_scipy"] = float(np.abs(x24[0, :len(ref)].cpu().numpy() - ref).max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
