#!/usr/bin/env python3
"""Developer tool (GPU): time of stage 2 and of the training batch (serenade_amd/stats.py) on B utterances of `seconds` s
at 100 frames per second -- hubert (T, 768), logmel (T, 80), loud and score (T, 1), float32 -- warm, best of 10 by HIP
events: fit_statistics and the Collater from host dumps (which adds the packing, the upload and the read-back), and
the two entry points on their own from device-resident tracks.  Next to them, on the host for the same items: sklearn's
four scalers fed one partial_fit per utterance, and FeatsDataset's numpy normalisation + a literal SSCCollater.  Checks
agreement on item 0.  Prints one JSON line.

    python tools/statsbench.py [B=8] [seconds=10]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from serenade_amd import stats as S  # noqa: E402
from serenade_amd.datasets import _scale  # noqa: E402
from tools.harvestbench import gpu_ms  # noqa: E402

TRACKS = {"hubert": (0.1, 0.4, 768), "logmel": (-4.0, 2.0, 80), "loud": (-30.0, 8.0, 1), "est_lf0_score": (5.5, 0.4, 1)}
ENTRY = {"hubert": "hubert", "logmel": "logmel", "loud": "loud", "est_lf0_score": "score"}


def host_best(fn, reps=10):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return 1e3 * best


def host_chain(dumps, scaler, max_frames=3000):
    """datasets._scale per track, then SSCCollater's sort, filter, .float() and zero padding"""
    items = [{k: _scale(d[k], scaler[e], S.ENTRIES[e]) for k, e in ENTRY.items()} for d in dumps]
    batch = [b for b in sorted(items, key=lambda x: -x["hubert"].shape[0]) if len(b["hubert"]) < max_frames]
    out = {}
    for k in ENTRY:
        pad = np.zeros((len(batch), len(batch[0]["hubert"]), batch[0][k].shape[1]), dtype=np.float32)
        for i, b in enumerate(batch):
            pad[i, :len(b[k])] = b[k]
        out[k] = pad
    return out


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    sec = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    assert torch.cuda.is_available(), "statsbench needs an MI355X"
    rng = np.random.default_rng(0)
    lens = [int(100 * sec) - 7 * b for b in range(B)]  # ragged
    dumps = [{k: (m + s * rng.standard_normal((n, C))).astype(np.float32) for k, (m, s, C) in TRACKS.items()}
             for n in lens]
    res = dict(tool="statsbench", B=B, seconds=sec, frames=lens[0], rows=sum(lens))
    scaler = S.fit_statistics(dumps, batch=B)
    collater = S.Collater(scaler)
    for _ in range(2):  # warm: code objects, allocator
        S.fit_statistics(dumps, batch=B), collater(dumps)
    torch.cuda.synchronize()
    res["gpu_fit_statistics_ms"] = gpu_ms(lambda: S.fit_statistics(dumps, batch=B))
    res["gpu_collater_ms"] = gpu_ms(lambda: collater(dumps))
    dev = {k: [torch.from_numpy(d[k]).to("cuda:0") for d in dumps] for k in TRACKS}
    packed = {k: S._Packed(v, "statsbench") for k, v in dev.items()}
    order = torch.arange(B, dtype=torch.int32, device="cuda:0")
    for k, (_, _, C) in TRACKS.items():
        p = packed[k]
        f64 = torch.empty(2, B, C, dtype=torch.float64, device="cuda:0")
        f32 = torch.empty(2, B, C, dtype=torch.float32, device="cuda:0")
        bad = torch.empty(B, dtype=torch.int32, device="cuda:0")
        op = S.ops.CallOp("srn_col_moments", (p.x, p.row_off, p.R, f64[0], f64[1], f32[0], f32[1], bad, B, C))
        op()
        res[f"gpu_col_moments_{ENTRY[k]}_ms"] = gpu_ms(op)
        sub, div = (torch.from_numpy(v).to("cuda:0") for v in collater.operands[ENTRY[k]])
        out = torch.empty(B, lens[0], C, dtype=torch.float32, device="cuda:0")
        op = S.ops.CallOp("srn_scale_collate", (p.x, p.row_off, p.R, order, sub, div, int(sub.dtype == torch.float64),
                                                out, lens[0], B, B, C))
        op()
        res[f"gpu_scale_collate_{ENTRY[k]}_ms"] = gpu_ms(op)
    got = collater(dumps)
    try:
        from sklearn.preprocessing import MinMaxScaler, StandardScaler
    except ImportError:
        res["sklearn"] = None
        ref = scaler
    else:
        def fit():
            sk = {"hubert": StandardScaler(), "logmel": StandardScaler(), "score": MinMaxScaler(), "loud": MinMaxScaler()}
            for d in dumps:
                for k, e in ENTRY.items():
                    sk[e].partial_fit(d[k])
            return sk

        ref = fit()
        res["host_sklearn_fit_ms"] = host_best(fit, reps=3)
        res["mean_max_diff_vs_sklearn"] = float(max(np.abs(scaler[e].mean_ - ref[e].mean_).max() for e in ("hubert", "logmel")))
        res["var_max_rel_diff_vs_sklearn"] = float(max((np.abs(scaler[e].var_ - ref[e].var_) / ref[e].var_).max()
                                                       for e in ("hubert", "logmel")))
        res["minmax_bitwise_vs_sklearn"] = all(scaler[e].data_min_.tobytes() == ref[e].data_min_.tobytes()
                                               and scaler[e].data_max_.tobytes() == ref[e].data_max_.tobytes()
                                               for e in ("score", "loud"))
    res["host_numpy_collate_ms"] = host_best(lambda: host_chain(dumps, scaler), reps=3)
    want = host_chain(dumps, scaler)
    names = {"hubert": "xs", "logmel": "ys", "loud": "louds", "est_lf0_score": "scores"}
    res["item0_bitwise_vs_numpy"] = all(got[names[k]][0].cpu().numpy().tobytes() == want[k][0].tobytes() for k in TRACKS)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
