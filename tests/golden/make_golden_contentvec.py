"""Writes tests/golden/contentvec_small.npz: seeded weights of a reduced ContentVec (HubertModel) whose structure is
hubert-base's (group-norm feature extractor, 10 ms last stride, weight-normed grouped positional conv, post-LN layers),
two 16 kHz inputs of different odd lengths, and transformers' output of each on its own (B = 1, float64).

    python tests/golden/make_golden_contentvec.py

Needs `transformers` (the GPU tests that read the file do not)."""
import json
import os

import numpy as np
import torch
from transformers import HubertConfig, HubertModel

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, conv_dim=[32] * 7,
              conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 1], num_conv_pos_embeddings=16,
              num_conv_pos_embedding_groups=4)
LENGTHS = (4001, 6397)


def seeded_model(config, seed):
    """HubertModel in eval mode with every parameter drawn from a seeded generator (norm affines included)"""
    torch.manual_seed(seed)
    cfg = HubertConfig(**config)
    m = HubertModel(cfg).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("layer_norm.weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("layer_norm.bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return m


def reference(model, wave):
    """last_hidden_state of one utterance, in float64"""
    m = model.double()
    with torch.no_grad():
        out = m(torch.as_tensor(wave, dtype=torch.float64).view(1, -1)).last_hidden_state[0]
    model.float()
    return out.numpy()


def main():
    model = seeded_model(CONFIG, 1234)
    rng = np.random.default_rng(5)
    out = {"config": np.array(json.dumps(CONFIG))}
    for k, v in model.state_dict().items():
        out["sd." + k] = v.numpy().astype(np.float32)
    for i, n in enumerate(LENGTHS):
        t = np.arange(n) / 16000.0
        wave = (0.3 * np.sin(2 * np.pi * (140 + 60 * i) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
        out[f"wave{i}"] = wave
        out[f"ref{i}"] = reference(model, wave).astype(np.float32)
    np.savez(os.path.join(HERE, "contentvec_small.npz"), **out)


if __name__ == "__main__":
    main()
