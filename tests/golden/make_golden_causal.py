"""Capture the causal HiFi-GAN goldens from the REFERENCE itself (run in the build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_causal.py

Like make_golden.py: imports the reference through tests/golden/_ref_harness.py, builds its HiFiGANGenerator with
use_causal_conv=True in the small configuration of tests/_weights.hifigan_weights(small=True) (channels 64, scales
(4, 2), kernels (3, 5), dilations [(1, 2), (2, 6, 3)]: one fused stage at C = 32, one unfused at C = 16), fills it with
the procedural name-keyed weights of serenade_amd/utils/synth.py (seed 1) and stores
    hifigan_causal_small.npz    c (2, 80, 9), y = gen(c) (2, 1, 72), y5 = gen(c[:, :, :5]) (2, 1, 40)
    hifigan_causal_keys.json    the state_dict keys of the reference class, with and without weight norm
and, for the full HIFIGAN_PARAMS with use_causal_conv (seed 0),
    hifigan_causal.npz          c (2, 80, 5), y = gen(c) (2, 1, 1200)
Only data is stored: the weights are regenerated from the seed by whoever reads the fixtures.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_harness  # noqa: E402

_ref_harness.install()

from serenade.vocoder.models.hifigan import HiFiGANGenerator  # noqa: E402

from serenade_amd.utils.synth import HIFIGAN_PARAMS, fill_state_dict  # noqa: E402

SMALL = dict(HIFIGAN_PARAMS, channels=64, upsample_scales=(4, 2), upsample_kernel_sizes=(8, 4),
             resblock_kernel_sizes=(3, 5), resblock_dilations=[(1, 2), (2, 6, 3)], use_causal_conv=True)
SEED = 1


def main():
    torch.set_grad_enabled(False)
    gen = HiFiGANGenerator(**SMALL).eval()
    keys_wn = {k: list(v.shape) for k, v in gen.state_dict().items()}
    gen.load_state_dict(fill_state_dict(gen.state_dict(), seed=SEED))
    gen.remove_weight_norm()
    keys = {k: list(v.shape) for k, v in gen.state_dict().items()}
    c = torch.from_numpy(np.random.default_rng(778).standard_normal((2, 80, 9)).astype(np.float32))
    y, y5 = gen(c), gen(c[:, :, :5])
    print("prefix property of the reference: max |y5 - y[..., :40]| =", float((y5 - y[..., :y5.shape[-1]]).abs().max()))
    np.savez_compressed(os.path.join(HERE, "hifigan_causal_small.npz"), c=c.numpy(), y=y.numpy(), y5=y5.numpy())
    with open(os.path.join(HERE, "hifigan_causal_keys.json"), "w") as f:
        json.dump({"hifigan_causal_small_wn": keys_wn, "hifigan_causal_small": keys}, f, indent=0, sort_keys=True)
        f.write("\n")
    full = HiFiGANGenerator(**dict(HIFIGAN_PARAMS, use_causal_conv=True)).eval()
    full.load_state_dict(fill_state_dict(full.state_dict(), seed=0))
    full.remove_weight_norm()
    cf = torch.from_numpy(np.random.default_rng(779).standard_normal((2, 80, 5)).astype(np.float32))
    np.savez_compressed(os.path.join(HERE, "hifigan_causal.npz"), c=cf.numpy(), y=full(cf).numpy())
    print("wrote hifigan_causal_small.npz", tuple(c.shape), tuple(y.shape), tuple(y5.shape), "and", len(keys_wn), "keys")


if __name__ == "__main__":
    main()
