#!/usr/bin/env python3
"""Developer tool (GPU): HiFi-GAN vocoder throughput, dense against ragged.  The generator is
the path's HiFi-GAN (serenade_amd.utils.synth.HIFIGAN_PARAMS, procedural weights), driven through `Vocoder` as the
decode CLI drives it.  Prints one JSON object.

    vocbench.py B T                 the dense `decode_batch` on B utterances of T frames
    vocbench.py B T --ragged        the same dense call; the ragged call (`decode_batch(lengths=)`) on the same equal
                                    lengths; then B DISTINCT lengths per batch, a new set every batch as a corpus has
                                    them, the batch maxima spread over the 128 frames below T: (a) the decode CLI's
                                    `by_len` loop (one dense call per distinct length: plan build, buffers and -- with
                                    graphs on -- capture included), (b) one `decode_ragged` call per batch, at bucket
                                    sizes 1, 32, 64 and 128 frames (plans reused where a batch falls into a bucket seen
                                    before, dead frames up to the bucket's end computed)
    --causal                        the generator with use_causal_conv=True: the same calls
    --stream N                      (implies --causal; may be given several times) besides the one-shot call, the same
                                    B x T frames through `Vocoder.stream(B, N)` in chunks of N frames: wall time for the
                                    whole batch, per chunk, and from reset() to the first chunk's samples on the host
    --sessions                      (implies --causal) 8 live sessions with staggered starts and
                                    unequal frames per tick, N = the first --stream value (default 32) frames at most:
                                    (a) ONE `Vocoder.stream(8, N, ragged=True)` push per tick; (b) one B = 1
                                    `Vocoder.stream(1, N)` per session, pushed in turn for every session that gives
                                    frames in the tick -- timed with full chunks, since a push runs the same op list at
                                    any length and a short chunk would end a lock-step stream; (c) equal chunks of N
                                    frames through the ragged stream and through the lock-step `Vocoder.stream(8, N)`.
                                    ms per tick, launches per push, and the ragged stream's worst difference from each
                                    session's one-shot decode
    --graphs                        replay plans as captured hipGraphs (ops.set_graphs)
    --passes N                      batches of fresh lengths per measurement (default 6)

Every figure is wall time per batch over the passes, after a warm-up on lengths the passes do not reuse (kernels loaded,
allocator warm); a median of one run is not a distribution -- repeat the run before relying on a difference of a few
per cent."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serenade_amd import _shapes, build, ops, vocoder  # noqa: E402
from serenade_amd.utils.synth import HIFIGAN_PARAMS, fill_state_dict  # noqa: E402

BUCKETS = (1, 32, 64, 128)


def make_vocoder(dev, causal=False):
    params = dict(HIFIGAN_PARAMS, use_causal_conv=causal)
    gen = vocoder.HiFiGANGenerator(**params)
    gen.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**params, weight_norm=True)), seed=0))
    one = np.ones(80, dtype=np.float32)
    return vocoder.Vocoder.from_generator(gen, {"sampling_rate": 24000}, {"mean": 0 * one, "scale": one}, dev,
                                          trg_stats={"mean": 0 * one, "scale": one})


def _timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def distinct_length_sets(B, T, n_sets):
    """n_sets batches of B distinct frame counts, no count in two batches: each batch spread evenly over about half
    of T below its longest item, the longest items spread evenly over the min(128, T / 2) frames below T -- so the batch
    maxima fall into one bucket of 128 frames, two of 64, four of 32 and n_sets of 1"""
    step = max(1, (T // 2) // max(B - 1, 1))
    gap = min(128, T // 2) // n_sets
    used, sets = set(), []
    for s in range(n_sets):
        lens = []
        for b in range(B):
            v = T - s * gap - b * step
            while v in used:
                v -= 1
            if v < 1:
                sys.exit(f"vocbench: {n_sets} sets of {B} distinct lengths do not fit under {T} frames")
            used.add(v)
            lens.append(v)
        sets.append(lens)
    return sets


def by_len_loop(voc, mels):
    """what ssc_decode._run_jobs does without --ragged-vocoder"""
    by_len = {}
    for i, m in enumerate(mels):
        by_len.setdefault(m.shape[0], []).append(i)
    return [voc.decode_batch(torch.stack([mels[i] for i in idx])) for idx in by_len.values()]


def launches(plan):
    """kernel launches of one run of a plan (a MultiCopyOp launches once per table)"""
    return sum(len(op._lists) if isinstance(op, ops.MultiCopyOp) else 1 for op in plan.ops)


def session_schedule(n_sessions, n_ticks, chunk, rng):
    """[(lengths, restart)] per tick: session s starts at tick 2 s, gives 0 to `chunk` frames per tick (0 about one
    tick in six) and begins a new utterance every 10 ticks"""
    ticks = []
    for t in range(n_ticks):
        lens, restart = [0] * n_sessions, [False] * n_sessions
        for s in range(n_sessions):
            if t >= 2 * s:
                lens[s] = 0 if rng.random() < 1 / 6 else int(rng.integers(1, chunk + 1))
                restart[s] = (t - 2 * s) % 10 == 0
        ticks.append((lens, restart))
    return ticks


def sessions_bench(voc, dev, chunk, rng):
    S, n_ticks = 8, 36
    hop = voc.model.hop
    ticks = session_schedule(S, n_ticks, chunk, rng)
    feed = torch.from_numpy(rng.standard_normal((n_ticks, S, chunk, 80)).astype(np.float32)).to(dev)
    for t, (lens, _) in enumerate(ticks):
        for s, n in enumerate(lens):
            feed[t, s, n:] = float("nan")  # never read as data
    n_maxes = [max(max(lens), 1) for lens, _ in ticks]
    rag = voc.stream(S, chunk, ragged=True)

    def ragged_run(keep=None):
        for t, (lens, restart) in enumerate(ticks):
            y = rag.push(feed[t, :, :n_maxes[t]], lens, restart)
            if keep is not None:
                keep.append(y)

    # each utterance (a session's frames between two restarts) against its one-shot decode
    outs = []
    ragged_run(outs)
    worst, n_utt = 0.0, 0
    for s in range(S):
        mel, wav = [], []
        for t, (lens, restart) in enumerate(ticks + [([0] * S, [True] * S)]):
            if restart[s] and mel:
                worst = max(worst, float((torch.cat(wav) - voc.decode(torch.cat(mel))[0]).abs().max()))
                n_utt, mel, wav = n_utt + 1, [], []
            if t < n_ticks and lens[s]:
                mel.append(feed[t, s, :lens[s]])
                wav.append(outs[t][s, :lens[s] * hop])
    singles = [voc.stream(1, chunk) for _ in range(S)]
    full = feed[0, :1].nan_to_num()

    def singles_run():
        for lens, restart in ticks:
            for s in range(S):
                if restart[s]:
                    singles[s].reset()
                if lens[s]:
                    singles[s].push(full)
    pushes = sum(1 for lens, _ in ticks for n in lens if n)
    dt_r, dt_s = _timed(ragged_run, 2, 5), _timed(singles_run, 2, 5)
    lock = voc.stream(S, chunk)
    equal = feed[0].nan_to_num()
    every = [chunk] * S
    dt_re, dt_le = _timed(lambda: rag.push(equal, every), 5, 40), _timed(lambda: lock.push(equal), 5, 40)
    return {"sessions": S, "ticks": n_ticks, "chunk_frames": chunk, "frames": sum(sum(lens) for lens, _ in ticks),
            "utterances_checked": n_utt, "worst_abs_diff_vs_one_shot": worst,
            "ragged_stream": {"ms_per_tick": dt_r * 1e3 / n_ticks, "pushes": n_ticks,
                              "launches_per_push": launches(rag.stream._pl)},
            "b1_stream_per_session": {"ms_per_tick": dt_s * 1e3 / n_ticks, "pushes": pushes,
                                      "launches_per_push": launches(singles[0].stream._plan())},
            "equal_chunks": {"ragged_ms_per_push": dt_re * 1e3, "lock_step_ms_per_push": dt_le * 1e3,
                             "lock_step_launches_per_push": launches(lock.stream._plan())}}


def main():
    args, flags, passes, chunks = [], [], 6, []
    argv = sys.argv[1:]
    while argv:
        v = argv.pop(0)
        if v in ("--passes", "--stream"):
            if not argv:
                sys.exit(__doc__)
            n = int(argv.pop(0))
            if v == "--passes":
                passes = n
            else:
                chunks.append(n)
        (flags if v.startswith("--") else args).append(v)
    if set(flags) - {"--ragged", "--graphs", "--passes", "--causal", "--stream", "--sessions"}:
        sys.exit(__doc__)
    B, T = (int(v) for v in (args[:2] + ["8", "1024"][len(args):]))
    dev = torch.device("cuda:0")
    ops.set_graphs("--graphs" in flags)
    causal = "--causal" in flags or bool(chunks) or "--sessions" in flags
    voc = make_vocoder(dev, causal)
    hop = voc.model.hop
    rng = np.random.default_rng(0)
    pool = torch.from_numpy(rng.standard_normal((B, T, 80)).astype(np.float32)).to(dev)
    out = {"build_id": build.built_id(), "graphs": "--graphs" in flags, "passes": passes, "causal": causal,
           "workload": f"B={B} utterances x {T} frames, hop {hop}"}

    def rate(dt, frames):
        return {"ms_per_batch": dt * 1e3, "frames_per_s": frames / dt}

    if "--sessions" in flags:
        with torch.no_grad():
            out["workload"] = "8 sessions, staggered starts, unequal frames per tick"
            out["sessions"] = sessions_bench(voc, dev, chunks[0] if chunks else 32, rng)
        print(json.dumps(out, indent=1))
        return
    with torch.no_grad():
        out["dense_equal"] = rate(_timed(lambda: voc.decode_batch(pool), 3, 10), B * T)
        for n in chunks:
            st = voc.stream(B, n)
            pieces = [pool[:, t:t + n] for t in range(0, T, n)]

            def whole():
                st.reset()
                for c in pieces:
                    st.push(c)

            def first():
                st.reset()
                return st.push(pieces[0]).cpu()
            dt = _timed(whole, 2, 5)
            out[f"stream_{n}"] = dict(rate(dt, B * T), chunks=len(pieces), ms_per_chunk=dt * 1e3 / len(pieces),
                                      first_chunk_ms=_timed(first, 2, 10) * 1e3)
        if "--ragged" in flags:
            full = [T] * B
            out["ragged_equal"] = rate(_timed(lambda: voc.decode_batch(pool, lengths=full), 3, 10), B * T)
            sets = distinct_length_sets(B, T, passes + 1)
            sets = sets[-1:] + sets[:-1]  # the warm-up batch is the shortest, so every plan of the passes is new
            frames = sum(sum(s) for s in sets[1:]) / passes

            def corpus(fn):
                voc.model._plans.clear()
                fn([pool[b, :n] for b, n in enumerate(sets[0])])  # warm-up on lengths no pass reuses
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in sets[1:]:
                    fn([pool[b, :n] for b, n in enumerate(s)])
                torch.cuda.synchronize()
                return rate((time.perf_counter() - t0) / passes, frames)

            out["distinct_by_len_loop"] = corpus(lambda mels: by_len_loop(voc, mels))
            out["distinct_ragged_call"] = {}
            for bucket in BUCKETS:
                vocoder.RAGGED_BUCKET = bucket
                out["distinct_ragged_call"][f"bucket_{bucket}"] = corpus(voc.decode_ragged)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
