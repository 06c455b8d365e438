#!/usr/bin/env python3
"""Developer tool (GPU): throughput of the ContentVec content encoder (serenade_amd/contentvec.py, hubert-base geometry
with seeded weights) on B utterances of `seconds` s at 16 kHz.  Prints one JSON line: ms per batch, seconds of audio per
second, TFLOP/s and its fraction of the 157.3 TFLOP/s fp32 matrix roof, the share of the HBM-bound passes (layer-0
conv, channel norm, LayerNorms, softmax) with the channel norm's bandwidth, and -- when transformers imports -- a
16-thread CPU transformers baseline (one item, scaled to B).

    python tools/cvecbench.py [B=8] [seconds=10] [--no-cpu]
"""
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serenade_amd import ops  # noqa: E402
from serenade_amd.contentvec import ContentVec  # noqa: E402

FP32_ROOF_TFLOPS = 157.3
HBM_TBPS = 8.0
MEMORY_BOUND = ("srn_cvec_conv0", "srn_channel_norm_gelu", "srn_layernorm", "srn_softmax_rows")


def seeded_state(cv, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in cv.state_shapes().items():
        r = torch.randn(shp, generator=g)
        if k.endswith("weight_g") or ("norm" in k and k.endswith("weight")):
            sd[k] = 1.0 + 0.1 * r
        elif k.endswith("weight_v") or k.endswith("conv.weight"):
            sd[k] = r * math.sqrt(2.0 / (shp[1] * shp[2]))
        elif k.endswith("bias"):
            sd[k] = 0.05 * r
        else:
            sd[k] = 0.02 * r
    return sd


def flops(cv, n):
    """multiply-adds x 2 of one utterance of n samples"""
    c = cv.config
    Ts = cv.layer_frames(n)
    C, D, H, FF = c["conv_dim"][0], c["hidden_size"], c["num_attention_heads"], c["intermediate_size"]
    T = Ts[-1]
    f = 2 * Ts[0] * C * c["conv_kernel"][0]
    f += sum(2 * Ts[l] * C * C * c["conv_kernel"][l] for l in range(1, len(Ts)))
    f += 2 * T * C * D + 2 * T * D * (D // c["num_conv_pos_embedding_groups"]) * c["num_conv_pos_embeddings"]
    f += c["num_hidden_layers"] * (2 * T * D * 4 * D + 4 * T * D * FF + 4 * T * T * D)
    return f


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 8
    sec = float(args[1]) if len(args) > 1 else 10.0
    n = int(round(sec * 16000))
    cv = ContentVec(device="cuda")
    sd = seeded_state(cv)
    cv.load_state_dict(sd)
    x = 0.3 * torch.randn(B, n, generator=torch.Generator().manual_seed(1)).cuda()
    for _ in range(3):
        cv(x)
    torch.cuda.synchronize()
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        cv(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    # per-launch times of one pass over the plan (events around every op)
    plan = next(iter(cv._plans.values()))
    ev = []
    for op in plan.ops:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        op()
        e.record()
        ev.append((s, e, op))
    torch.cuda.synchronize()
    per = {}
    for s, e, op in ev:
        name = getattr(op, "name", "srn_conv_gemm")
        per[name] = per.get(name, 0.0) + s.elapsed_time(e)
    total = sum(per.values())
    mem = sum(v for k, v in per.items() if k in MEMORY_BOUND)
    T0 = plan.Ts[0]
    cn_bytes = 2 * B * T0 * cv.config["conv_dim"][0] * 4
    fl = B * flops(cv, n)
    out = {"workload": f"ContentVec hubert-base, B={B} x {sec:g} s at 16 kHz ({cv.frames(n)} frames each), exact fp32",
           "ms_per_batch": dt * 1e3, "audio_s_per_s": B * sec / dt, "gflop_per_batch": fl / 1e9,
           "tflops": fl / dt / 1e12, "fraction_of_fp32_roof": fl / dt / 1e12 / FP32_ROOF_TFLOPS,
           "memory_bound_share": mem / total, "per_entry_ms": {k: round(v, 4) for k, v in sorted(per.items())},
           "channel_norm_tbps": cn_bytes / (per["srn_channel_norm_gelu"] * 1e-3) / 1e12,
           "channel_norm_fraction_of_hbm": cn_bytes / (per["srn_channel_norm_gelu"] * 1e-3) / 1e12 / HBM_TBPS,
           "graphs": ops.GRAPHS}
    if "--no-cpu" not in sys.argv:
        try:
            import transformers
        except ImportError:
            transformers = None
        if transformers is not None:
            torch.set_num_threads(16)
            m = transformers.HubertModel(transformers.HubertConfig()).eval()
            m.feature_extractor.conv_layers[-1].conv.stride = (1,)
            pre = "encoder.pos_conv_embed.conv."
            sd_t = dict(sd)
            sd_t[pre + "parametrizations.weight.original0"] = sd_t.pop(pre + "weight_g")
            sd_t[pre + "parametrizations.weight.original1"] = sd_t.pop(pre + "weight_v")
            m.load_state_dict(sd_t, strict=False)
            xc = x[:1].cpu()
            with torch.no_grad():
                m(xc[:, :16000])
                t0 = time.perf_counter()
                m(xc)
                tc = time.perf_counter() - t0
            out["cpu_transformers_16t_ms_per_batch"] = tc * B * 1e3
            out["speedup_vs_cpu"] = tc * B / dt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
