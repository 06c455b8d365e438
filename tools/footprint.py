#!/usr/bin/env python3
"""Developer tool (GPU): HBM footprint of the plans (weights, weight planes, activations, attention scores, vocoder
stages) after one conversion at the given sizes.

    python tools/footprint.py B T [B T ...]      e.g.  python tools/footprint.py 8 1024 8 4096 32 4096
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from serenade_amd.utils.synth import synth_inputs  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    a = [int(x) for x in sys.argv[1:]]
    for B, T in zip(a[0::2], a[1::2]):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        model, voc, _, _ = bench.build_models(dev)
        base = torch.cuda.memory_allocated()
        d = synth_inputs(B, T, T_ref=256, seed=1)
        g = {k: (v.to(dev) if v.is_floating_point() else v) for k, v in d.items()}
        mel = model.inference(g["x"], g["lengths"], g["midi"], g["lft"], g["ref_x"], g["ref_lengths"], g["ref_logmel"],
                              g["ref_midi"], g["ref_lft"], noise=g["z"])
        voc.decode_batch(mel if mel.dim() == 3 else mel.unsqueeze(0))
        torch.cuda.synchronize()
        pl = model.cfm_decoder.estimator.plan(B, T + 256, 10, euler=True)
        print(f"B={B} T={T}: weights {base / 2**30:.2f} GiB, total allocated {torch.cuda.memory_allocated() / 2**30:.2f} "
              f"GiB, peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB; attention score buffer "
              f"{pl.S.numel() * 4 / 2**20:.0f} MiB "
              f"(unchunked it would be {B * 4 * (T + 256) * ((T + 256 + 31) // 32 * 32) * 4 / 2**30:.2f} GiB)", flush=True)
        del model, voc, pl, mel, g, d


if __name__ == "__main__":
    main()
