"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy (float32, under 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_small_arrays_are_written_whole(tmp_path):
    rng = np.random.default_rng(1)
    mel, wave = rng.standard_normal((2, 64, 80)), rng.standard_normal((2, 64 * 240)).astype(np.float32)
    info = bench.dump_outputs(str(tmp_path), {"mel": mel, "wave": wave, "absent": None})
    assert sorted(os.listdir(tmp_path)) == ["mel.npy", "wave.npy"]
    got = np.load(tmp_path / "mel.npy")
    assert got.dtype == np.float32 and np.array_equal(got, mel.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "wave.npy"), wave)
    assert info["arrays"]["mel"] == {"shape": [2, 64, 80], "dtype": "float32"}


def test_dump_large_arrays_are_a_fixed_sample_under_64_mb(tmp_path):
    big = np.arange(16 * 10**6, dtype=np.float32).reshape(40, -1)  # 64 MB, every value exact in float32
    small = np.ones((1000,), np.float32)
    sizes = []
    for sub in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / sub), {"wave": big, "mel": small})
        sizes.append(sum(os.path.getsize(tmp_path / sub / f) for f in os.listdir(tmp_path / sub)))
    assert max(sizes) < 64 * 10**6
    a, b = np.load(tmp_path / "a" / "wave.npy"), np.load(tmp_path / "b" / "wave.npy")
    assert np.array_equal(a, b) and a.dtype == np.float32  # the same seeded sample every time
    assert np.all(np.diff(a) > 0) and a.size == info["arrays"]["wave"]["sampled"]["elements"]
    assert info["arrays"]["wave"]["sampled"]["of"] == big.size and info["arrays"]["wave"]["shape"] == [40, 400000]


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """a tiny bench run: --steps sets the timed steps, ms_per_step is reported, and the dumped mel / waveform are what
    the oracle computes from the same seeded inputs and weights"""
    from oracle import serenade_oracle as O
    from serenade_amd import _shapes
    from serenade_amd.utils.synth import HIFIGAN_PARAMS, SERENADE_PARAMS, fill_state_dict, synth_inputs

    B, T, T_ref, n = 2, 64, 32, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-sweep", "--no-train", "--no-mixed", "--no-post", "--modes", "fp32",
                        "--batch", str(B), "--frames", str(T), "--ref-frames", str(T_ref), "--euler", str(n),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["mel.npy", "wave.npy"]
    mel, wave = np.load(tmp_path / "mel.npy"), np.load(tmp_path / "wave.npy")
    assert mel.dtype == wave.dtype == np.float32 and mel.shape == (B, T, 80) and wave.shape == (B, T * 240)

    sd = fill_state_dict(_shapes.as_meta(_shapes.serenade_shapes(**SERENADE_PARAMS)), seed=0)
    gsd = fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**HIFIGAN_PARAMS, weight_norm=True)), seed=0)
    d = synth_inputs(B, T, T_ref=T_ref, seed=1235)
    ref = O.serenade_inference(sd, d["x"], d["lengths"], d["midi"], d["lft"], d["ref_x"], d["ref_lengths"],
                               d["ref_logmel"], d["ref_midi"], d["ref_lft"], d["z"], n_timesteps=n)
    t1 = torch.ones(80)
    wref = O.vocoder_decode(gsd, ref, HIFIGAN_PARAMS, {"mean": 0 * t1, "scale": t1}, {"mean": 0 * t1, "scale": t1})
    assert np.abs(mel - ref.numpy()).max() <= 1e-3 * np.abs(ref.numpy()).max()
    assert np.abs(wave - wref.reshape(B, -1).numpy()).max() <= 1e-4
