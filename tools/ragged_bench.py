#!/usr/bin/env python3
"""Developer tool (GPU): the decode CLI's style loop (B = 1 per style) against one exact ragged batch of the same items.

`--distinct`: a corpus-like stream instead, B items with a NEW set of (T_b, R_b) in every batch and
the batches' longest R + T spread over two 64-row buckets, through the B = 1 `inference` loop, the shape-keyed
`inference_ragged` and the bucketed one (`bucket=`), graphs off and on; the same equal-length batch through both ragged
plans; the bucket table; and what the op list in front of the estimator costs on either plan.  Wall clock to a device
synchronise, milliseconds per batch.

    python tools/ragged_bench.py --distinct --B 4 --T 256 [--batches 6] [--buckets 1,32,64,128]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import serenade_amd  # noqa: E402
from serenade_amd import models  # noqa: E402
from serenade_amd.utils.synth import SERENADE_PARAMS, fill_state_dict, synth_inputs  # noqa: E402
from serenade_amd import _shapes  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    m = models.Serenade(**SERENADE_PARAMS)
    m.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.serenade_shapes(**SERENADE_PARAMS)), seed=0))
    m = m.eval().to(dev)
    T = int(os.environ.get("SRN_T", "256"))
    refs = [int(v) for v in os.environ.get("SRN_REFS", "200,256,310,280").split(",")]
    ds = [synth_inputs(1, T, T_ref=r, seed=i) for i, r in enumerate(refs)]
    g = lambda d, k: d[k].to(dev)
    items = [tuple(g(d, k)[0] for k in ("x", "midi", "lft", "ref_x", "ref_logmel", "ref_midi", "ref_lft")) for d in ds]
    zs = [g(d, "z") for d in ds]
    for mode in ("fp32", "bf16x6", "bf16x3"):
        serenade_amd.set_precision(mode)

        def loop():
            return [m.inference(g(d, "x"), d["lengths"], g(d, "midi"), g(d, "lft"), g(d, "ref_x"), d["ref_lengths"],
                                g(d, "ref_logmel"), g(d, "ref_midi"), g(d, "ref_lft"), noise=z) for d, z in zip(ds, zs)]

        def batch():
            return m.inference_ragged(items, noises=[z[0] for z in zs])

        res = {}
        for name, fn in (("loop", loop), ("ragged", batch)):
            for _ in range(3):
                out = fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                out = fn()
            torch.cuda.synchronize()
            res[name] = ((time.perf_counter() - t0) / 10 * 1e3, out)
        err = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(res["ragged"][1], res["loop"][1]))
        print(f"{mode}: T={T} refs={refs}: loop {res['loop'][0]:.2f} ms, ragged {res['ragged'][0]:.2f} ms, "
              f"max rel diff {err:.2e}", flush=True)


def _stream(B, T, n, seed=0):
    """n batches of B (T_b, R_b) pairs, all distinct: the longest R + T of batch i lies in the bucket below 2 T for even
    i and in the last bucket up to 2 T for odd i; no track is shorter than 16 rows or longer than T"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cap = 2 * T - 64 * (1 - i % 2)
        totals = [int(rng.integers(cap - 63, cap + 1))] + [int(v) for v in rng.integers(cap // 2, cap - 63, B - 1)]
        shapes = []
        for tot in totals:
            r = min(max(int(tot * rng.uniform(0.3, 0.5)), 16, tot - T), T)
            shapes.append((tot - r, r))
        out.append(shapes)
    return out


def _timed(fn, batches, warm):
    for b in batches[:warm]:
        fn(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches[warm:]:
        fn(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (len(batches) - warm) * 1e3


def distinct(args):
    from serenade_amd import ops
    dev = torch.device("cuda:0")
    m = models.Serenade(**SERENADE_PARAMS)
    m.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.serenade_shapes(**SERENADE_PARAMS)), seed=0))
    m = m.eval().to(dev)
    B, T, warm = args.B, args.T, 4  # warm-up: two batches per bucket (with graphs on: the eager run and the capture)
    keys = ("x", "midi", "lft", "ref_x", "ref_logmel", "ref_midi", "ref_lft")

    def make(shapes, seed):
        ds = [synth_inputs(1, t, T_ref=r, seed=seed + i) for i, (t, r) in enumerate(shapes)]
        return dict(ds=[{k: (v.to(dev) if k not in ("lengths", "ref_lengths") else v) for k, v in d.items()} for d in ds],
                    items=[tuple(d[k][0].to(dev) for k in keys) for d in ds], z=[d["z"][0].to(dev) for d in ds])

    stream = [make(s, 100 * i) for i, s in enumerate(_stream(B, T, warm + args.batches))]
    equal = [make([(T, T)] * B, 9000)] * (warm + args.batches)

    def loop(b):
        return [m.inference(d["x"], d["lengths"], d["midi"], d["lft"], d["ref_x"], d["ref_lengths"], d["ref_logmel"],
                            d["ref_midi"], d["ref_lft"], noise=d["z"]) for d in b["ds"]]

    def keyed(b):
        return m.inference_ragged(b["items"], noises=b["z"])

    def bucketed(b, bucket=models.RAGGED_BUCKET):
        return m.inference_ragged(b["items"], noises=b["z"], bucket=bucket)

    def fresh():
        m._plans.clear()
        m.cfm_decoder.estimator._plans.clear()
        torch.cuda.synchronize()

    print(f"--distinct: B={B} T={T}, {args.batches} timed batches after {warm}, ms per batch", flush=True)
    for graphs in (False, True):
        ops.set_graphs(graphs)
        for rep in range(2):  # every row twice: the run-to-run spread
            row = {}
            for name, fn, data in (("B=1 loop", loop, stream), ("shape-keyed", keyed, stream),
                                   ("bucketed", bucketed, stream), ("shape-keyed, equal lengths", keyed, equal),
                                   ("bucketed, equal lengths", bucketed, equal)):
                fresh()
                row[name] = _timed(fn, data, warm)
            print(f"graphs {'on ' if graphs else 'off'} run {rep}: " + ", ".join(f"{k} {v:.1f}" for k, v in row.items()),
                  flush=True)
    for graphs in (False, True):
        ops.set_graphs(graphs)
        row = {}
        for bucket in args.buckets:
            fresh()
            ms = _timed(lambda b: bucketed(b, bucket), stream, warm)
            row[bucket] = (ms, sum(k[0] == "ragged-bucket" for k in m._plans))
        print(f"graphs {'on ' if graphs else 'off'} bucket table (ms per batch, plans alive of 4): "
              + ", ".join(f"{k}: {v[0]:.1f} ({v[1]})" for k, v in row.items()), flush=True)
    # the op lists in front of the estimator (encoder passes, conditioning, style encoder) on the equal-length batch:
    # the bucketed plan runs both encoder passes over L_cap rows each, the shape-keyed one over Tm and Rm
    ops.set_graphs(False)
    fresh()
    keyed(equal[0]), bucketed(equal[0])
    for key, plan in m._plans.items():
        def front():
            for op in plan.ops:
                op()
        ms = _timed(lambda _: front(), [None] * 25, 5)
        print(f"front op list of the {key[0]} plan ({len(plan.ops)} ops, equal lengths T = R = {T}): {ms:.3f} ms", flush=True)
    err = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(bucketed(stream[0]), loop(stream[0])))
    print(f"bucketed against the B=1 loop on the first batch: max rel diff {err:.2e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--distinct", action="store_true", help="the distinct-lengths stream (see above)")
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--batches", type=int, default=6, help="timed batches (after 4 warm-up batches)")
    ap.add_argument("--buckets", type=lambda v: [int(x) for x in v.split(",")], default=[1, 32, 64, 128])
    a = ap.parse_args()
    distinct(a) if a.distinct else main()
