"""ContentVec content encoder on the GPU: the `hubert` track of a dump (768-dim features per 10 ms frame, the `x` /
`ref_x` of Serenade.inference), computed by the reference in serenade/bin/preprocess.py:41-50,361-368,495-503 with
`transformers.HubertModel` (hubert-base geometry, `lengyue233/content-vec-best` weights), the last feature-conv stride
set to 1 (10 ms instead of 20 ms frames), one utterance at a time, then a nearest `F.interpolate`.

    ContentVec(**geometry)          HubertConfig-style keyword arguments; defaults = hubert-base with the 10 ms stride
      .load_state_dict(sd)          HubertModel keys (both weight-norm spellings); final_proj.* / masked_spec_embed ignored
      .forward(wave16k, lengths)    (B, T', hidden) = HubertModel(...).last_hidden_state of every item on its own
      .frames(n_samples)            T' for an utterance of n samples
    extract_hubert(model, audio16k, sampling_rate, shiftms)    preprocess.py:495-503

Every item of a padded batch gets exactly what its own B = 1 call gets (`lengths`): layer 0's GroupNorm takes its
statistics over the item's valid frames, the positional conv reads rows past the item's length as zero and attention
keys stop at it.  (The reference cannot batch: transformers derives its mask length from `config.conv_stride`, which does
not know the stride override, and its GroupNorm runs over padded samples; so it runs B = 1.)

Arithmetic is exact fp32 throughout, all of it in libserenade_hip.so: layer 0 + its per-channel statistics
(srn_cvec_conv0), the channel norm + GELU (srn_channel_norm_gelu), feature convs 1-6, projections, Q K^T and P V
(srn_conv_gemm; GELU as the SRN_POST_GELU epilogue), the grouped positional conv with its GELU and residual
(srn_posconv_gelu_res), srn_layernorm and srn_softmax_rows.  Plans are cached per (B, samples, lengths) and replayed
through ops.GraphRunner; no torch arithmetic runs inside a plan and there is no CPU path.
"""
import math

import numpy as np
import torch

from . import _lib, ops
from .ops import ConvOp, GraphRunner
from .plan import attention_ops, attention_scores, check_state, linear_op, lru_get, rup, wave_batch

__all__ = ["ContentVec", "extract_hubert", "DEFAULT_CONFIG"]

# hubert-base (transformers HubertConfig defaults) with the 10 ms frame shift of preprocess.py:366-368
DEFAULT_CONFIG = dict(
    hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
    conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 1), conv_bias=False,
    feat_extract_norm="group", feat_proj_layer_norm=True, do_stable_layer_norm=False,
    num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, hidden_act="gelu", layer_norm_eps=1e-5,
)
# settings that must hold for the arithmetic here to be HubertModel's (anything else raises rather than half-works)
_FIXED = dict(conv_bias=False, feat_extract_norm="group", feat_proj_layer_norm=True, do_stable_layer_norm=False,
              hidden_act="gelu")
_IGNORED = ("final_proj.", "masked_spec_embed")


def _norm_key(k):
    """both weight-norm spellings of the positional conv -> (g, v): transformers 5.x parametrizations, hub weight_g/v"""
    pre = "encoder.pos_conv_embed.conv."
    for old, new in (("parametrizations.weight.original0", "weight_g"), ("parametrizations.weight.original1", "weight_v")):
        if k == pre + old:
            return pre + new
    return k


class ContentVec:
    """HubertModel.eval() (post-LN encoder, group-norm feature extractor) with exact ragged batching on the GPU."""

    def __init__(self, device="cuda", **config):
        unknown = set(config) - set(DEFAULT_CONFIG)
        if unknown:
            raise TypeError(f"ContentVec: unknown settings {sorted(unknown)}")
        cfg = dict(DEFAULT_CONFIG, **config)
        for k, v in _FIXED.items():
            if cfg[k] != v:
                raise ValueError(f"ContentVec: {k}={cfg[k]!r} is not supported (only {v!r})")
        cfg["conv_dim"], cfg["conv_kernel"], cfg["conv_stride"] = (tuple(int(v) for v in cfg[k])
                                                                  for k in ("conv_dim", "conv_kernel", "conv_stride"))
        if not (len(cfg["conv_dim"]) == len(cfg["conv_kernel"]) == len(cfg["conv_stride"]) >= 1):
            raise ValueError("ContentVec: conv_dim, conv_kernel and conv_stride need one entry per layer")
        if len(set(cfg["conv_dim"])) != 1:
            raise ValueError("ContentVec: the feature convs must all have the same width")
        D, H = cfg["hidden_size"], cfg["num_attention_heads"]
        C = cfg["conv_dim"][0]
        if D % H or C % 4 or D % 4 or cfg["intermediate_size"] % 4 or (D // H) % 4:
            raise ValueError("ContentVec: widths must be multiples of 4 and hidden_size divisible by the heads")
        if cfg["conv_kernel"][0] > 16:
            raise ValueError("ContentVec: layer 0's kernel must be <= 16 taps")
        if max(cfg["conv_kernel"][1:], default=1) > _lib.SRN_MAX_TAPS:
            raise ValueError(f"ContentVec: feature convs 1.. must be <= {_lib.SRN_MAX_TAPS} taps")
        G, K = cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"]
        if D % G or (D // G) % 4 or D // G > 64 or not 1 <= K <= 128:
            raise ValueError("ContentVec: the positional conv needs hidden/groups a multiple of 4 and <= 64, k <= 128")
        self.config = cfg
        self.device = torch.device(device)
        self.eps = float(cfg["layer_norm_eps"])
        self.w = None
        self._plans = {}

    # ------------------------------------------------------------------------------------------------ weights
    def state_shapes(self):
        """{HubertModel state-dict key (hub weight-norm spelling): shape} of this geometry, final_proj excluded"""
        c = self.config
        C, D, FF = c["conv_dim"][0], c["hidden_size"], c["intermediate_size"]
        G, K = c["num_conv_pos_embedding_groups"], c["num_conv_pos_embeddings"]
        fe = "feature_extractor.conv_layers."
        sh = {fe + "0.conv.weight": (C, 1, c["conv_kernel"][0])}
        for i in range(1, len(c["conv_dim"])):
            sh[fe + f"{i}.conv.weight"] = (C, C, c["conv_kernel"][i])
        sh.update({fe + "0.layer_norm.weight": (C,), fe + "0.layer_norm.bias": (C,),
                   "feature_projection.layer_norm.weight": (C,), "feature_projection.layer_norm.bias": (C,),
                   "feature_projection.projection.weight": (D, C), "feature_projection.projection.bias": (D,),
                   "encoder.pos_conv_embed.conv.bias": (D,), "encoder.pos_conv_embed.conv.weight_g": (1, 1, K),
                   "encoder.pos_conv_embed.conv.weight_v": (D, D // G, K), "encoder.layer_norm.weight": (D,),
                   "encoder.layer_norm.bias": (D,)})
        for i in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            for m in ("q_proj", "k_proj", "v_proj", "out_proj"):
                sh[p + f"attention.{m}.weight"], sh[p + f"attention.{m}.bias"] = (D, D), (D,)
            sh.update({p + "layer_norm.weight": (D,), p + "layer_norm.bias": (D,), p + "final_layer_norm.weight": (D,),
                       p + "final_layer_norm.bias": (D,), p + "feed_forward.intermediate_dense.weight": (FF, D),
                       p + "feed_forward.intermediate_dense.bias": (FF,), p + "feed_forward.output_dense.weight": (D, FF),
                       p + "feed_forward.output_dense.bias": (D,)})
        return sh

    @staticmethod
    def map_state_dict(sd):
        """HubertModel / HubertModelWithFinalProj state dict -> {key: fp32 CPU tensor} in the hub spelling (weight_g /
        weight_v for the positional conv), final_proj.* and masked_spec_embed dropped"""
        out = {}
        for k, v in sd.items():
            if any(k.startswith(p) for p in _IGNORED):
                continue
            out[_norm_key(k)] = torch.as_tensor(v).detach().to("cpu", torch.float32)
        return out

    @staticmethod
    def fold_pos_weight(g, v):
        """weight norm with dim=2 (HubertPositionalConvEmbedding): w[:, :, k] = g[k] v[:, :, k] / ||v[:, :, k]||, by
        torch's own _weight_norm (bit-equal to the parametrized conv.weight)"""
        return torch._weight_norm(v.to(torch.float32), g.to(torch.float32), 2)

    @staticmethod
    def pack_pos_weight(pw, groups):
        """grouped Conv1d weight (D, D / groups, K) -> srn_posconv_gelu_res's [g][tap][c in][n out], the output columns
        zero-padded to whole 32-column blocks (32 up to 32 channels per group, else 64)"""
        D, Cg, K = pw.shape
        packed = torch.zeros(groups, K, Cg, 32 if Cg <= 32 else 64)
        packed[..., :Cg] = pw.reshape(groups, Cg, Cg, K).permute(0, 3, 2, 1)
        return packed

    def load_state_dict(self, sd):
        s = self.map_state_dict(sd)
        want = self.state_shapes()
        check_state("ContentVec.load_state_dict", s, want)
        c = self.config
        C, D = c["conv_dim"][0], c["hidden_size"]
        G, K = c["num_conv_pos_embedding_groups"], c["num_conv_pos_embeddings"]
        dev = self.device
        d = lambda t: t.to(dev, torch.float32).contiguous()
        fe = "feature_extractor.conv_layers."
        w = {"c0_w": d(s[fe + "0.conv.weight"].reshape(C, -1)), "gn_w": d(s[fe + "0.layer_norm.weight"]),
             "gn_b": d(s[fe + "0.layer_norm.bias"]),
             "convs": [d(ops.pack_conv_weight(s[fe + f"{i}.conv.weight"])) for i in range(1, len(c["conv_dim"]))],
             "fp_ln_w": d(s["feature_projection.layer_norm.weight"]), "fp_ln_b": d(s["feature_projection.layer_norm.bias"]),
             "fp_w": d(s["feature_projection.projection.weight"]), "fp_b": d(s["feature_projection.projection.bias"]),
             "enc_ln_w": d(s["encoder.layer_norm.weight"]), "enc_ln_b": d(s["encoder.layer_norm.bias"])}
        pw = self.fold_pos_weight(s["encoder.pos_conv_embed.conv.weight_g"], s["encoder.pos_conv_embed.conv.weight_v"])
        w["pos_w"], w["pos_b"] = d(self.pack_pos_weight(pw, G)), d(s["encoder.pos_conv_embed.conv.bias"])
        layers = []
        for i in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            a = p + "attention."
            layers.append({
                "qkv_w": d(torch.cat([s[a + f"{m}_proj.weight"] for m in "qkv"])),
                "qkv_b": d(torch.cat([s[a + f"{m}_proj.bias"] for m in "qkv"])),
                "o_w": d(s[a + "out_proj.weight"]), "o_b": d(s[a + "out_proj.bias"]),
                "ln1_w": d(s[p + "layer_norm.weight"]), "ln1_b": d(s[p + "layer_norm.bias"]),
                "ff1_w": d(s[p + "feed_forward.intermediate_dense.weight"]),
                "ff1_b": d(s[p + "feed_forward.intermediate_dense.bias"]),
                "ff2_w": d(s[p + "feed_forward.output_dense.weight"]), "ff2_b": d(s[p + "feed_forward.output_dense.bias"]),
                "ln2_w": d(s[p + "final_layer_norm.weight"]), "ln2_b": d(s[p + "final_layer_norm.bias"])})
        w["layers"] = layers
        self.w = w
        self._plans = {}
        return self

    # ------------------------------------------------------------------------------------------------ geometry
    def layer_frames(self, n_samples):
        """frames after every feature conv: T_l = floor((T_{l-1} - k_l) / s_l) + 1, T_{-1} = samples (0 if too short)"""
        t, out = int(n_samples), []
        for k, st in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            t = (t - k) // st + 1 if t >= k else 0
            out.append(t)
        return out

    def frames(self, n_samples):
        """output frames of an utterance of n_samples (16 kHz): the length of last_hidden_state"""
        return self.layer_frames(n_samples)[-1]

    # ------------------------------------------------------------------------------------------------ inference
    def forward(self, wave16k, lengths=None):
        """wave16k: (n,) or (B, n) CUDA float32 at 16 kHz (numpy is uploaded).  Returns (B, T', hidden) float32; with
        `lengths` (samples per item) the exact ragged batch and the per-item frame counts (list).  Frames at or past an
        item's count are padding (unspecified values)."""
        if self.w is None:
            raise RuntimeError("ContentVec: load_state_dict first")
        a, lens = wave_batch(wave16k, lengths, self.device, "ContentVec")
        B, n = a.shape
        if min(self.frames(v) for v in lens) < 1:
            raise ValueError(f"ContentVec: an utterance of {min(lens)} samples is shorter than one output frame")
        key = (str(a.device), B, n, tuple(lens))
        plan = lru_get(self._plans, key, 8, lambda: _Plan(self, a.device, B, n, lens))
        plan.wave.copy_(a, non_blocking=True)
        plan.run()
        out = plan.out.clone()
        return (out, [self.frames(v) for v in lens]) if lengths is not None else out

    __call__ = forward


class _Plan:
    """buffers + op list of one (B, n, lengths)"""

    def __init__(self, m, dev, B, n, lens):
        c, w = m.config, m.w
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        i32 = lambda v: torch.tensor(v, device=dev, dtype=torch.int32)
        Ts = m.layer_frames(n)
        per_item = [m.layer_frames(v) for v in lens]
        L = len(Ts)
        self.lens = [i32([p[l] for p in per_item]) for l in range(L)]
        C, D, H, FF = c["conv_dim"][0], c["hidden_size"], c["num_attention_heads"], c["intermediate_size"]
        hd = D // H
        T = Ts[-1]
        eps = m.eps
        self.wave = f(B, n)
        ol = []
        # ---- layer 0: conv + per-channel statistics over each item's valid frames, then GroupNorm(C groups) + GELU
        T0 = Ts[0]
        chunks = _lib.lib().srn_frame_stats_chunks(T0)
        h0 = f(B, T0, C)
        parts = torch.zeros(B, chunks, C, 2, device=dev, dtype=torch.float64)
        stats = f(B, C, 2)
        ol.append(ops.CallOp("srn_cvec_conv0", (self.wave, n, n, self.lens[0], w["c0_w"], h0, parts, B, T0, C,
                                                c["conv_kernel"][0], c["conv_stride"][0])))
        ol.append(ops.CallOp("srn_channel_norm_gelu", (h0, parts, chunks, self.lens[0], w["gn_w"], w["gn_b"], stats, h0,
                                                       B, T0, C, eps)))
        # ---- feature convs 1..: conv (no bias) + GELU in the epilogue.  A valid frame reads only valid frames.
        bufs = [f(B * max(Ts[1::2], default=1) * C), f(B * max(Ts[2::2], default=1) * C)]
        cur = h0
        for l in range(1, L):
            out = bufs[(l - 1) % 2]
            k, st = c["conv_kernel"][l], c["conv_stride"][l]
            ol.append(ConvOp(in0=cur, w=w["convs"][l - 1], out=out, n_batch=B, T_in=Ts[l - 1], T_out=Ts[l], C_in=C, N=C,
                             in0_bs=Ts[l - 1] * C, ld_in0=C, ldw=k * C, out_bs=Ts[l] * C, ld_out=C, taps=range(k),
                             in_stride=st, post=_lib.POST_GELU, precision=_lib.PREC_FP32))
            cur = out
        # ---- feature projection: LayerNorm(C) -> Linear C -> D
        xn = f(B, T, C)
        ol.append(ops.layernorm_op(cur, w["fp_ln_w"], w["fp_ln_b"], xn, B * T, C, eps))
        hA, hB = f(B, T, D), f(B, T, D)
        fp32 = _lib.PREC_FP32
        ol.append(linear_op(xn, B * T, C, w["fp_w"], w["fp_b"], hA, D, precision=fp32))
        # ---- h + GELU(posconv(h)) (rows past an item's length read as zero), then the encoder's LayerNorm
        K = c["num_conv_pos_embeddings"]
        ol.append(ops.CallOp("srn_posconv_gelu_res", (hA, self.lens[-1], w["pos_w"], w["pos_b"], hB, B, T, D,
                                                      c["num_conv_pos_embedding_groups"], K, K // 2)))
        X = hA
        ol.append(ops.layernorm_op(hB, w["enc_ln_w"], w["enc_ln_b"], X, B * T, D, eps))
        # ---- post-LN transformer layers (plan.attention_ops: chunked S, V^T from the QKV epilogue)
        Tp = rup(T, 32)
        qkv = f(B, T, 3 * D)
        Vt = f(B, D, Tp)  # zeroed: the pad columns are never written and must be zero
        S = attention_scores(B, H, T, dev)
        O, G = f(B, T, D), f(B, T, FF)
        ln = self.lens[-1]
        prec = ops.attention_precision()
        for t in w["layers"]:
            ol.append(ConvOp(in0=X, w=t["qkv_w"], out=qkv, n_batch=B, T_in=T, T_out=T, C_in=D, N=3 * D, in0_bs=T * D,
                             ld_in0=D, ldw=D, out_bs=T * 3 * D, ld_out=3 * D, bias=t["qkv_b"], out_tr=Vt,
                             out_tr_col0=2 * D, out_tr_bs=D * Tp, ld_out_tr=Tp, precision=_lib.PREC_FP32))
            ol += attention_ops(qkv, Vt, S, O, ln, B, H, hd, T, prec)
            ol.append(linear_op(O, B * T, D, t["o_w"], t["o_b"], hB, D, precision=fp32, res=X, res_mode=ops.RES_ADD,
                                ld_res=D))
            ol.append(ops.layernorm_op(hB, t["ln1_w"], t["ln1_b"], X, B * T, D, eps))
            ol.append(linear_op(X, B * T, D, t["ff1_w"], t["ff1_b"], G, FF, precision=fp32, post=_lib.POST_GELU))
            ol.append(linear_op(G, B * T, FF, t["ff2_w"], t["ff2_b"], hB, D, precision=fp32, res=X,
                                res_mode=ops.RES_ADD, ld_res=D))
            ol.append(ops.layernorm_op(hB, t["ln2_w"], t["ln2_b"], X, B * T, D, eps))
        self.out = X
        self.ops = ol
        self.Ts = Ts
        self.runner = GraphRunner(lambda: self.ops)

    def run(self):
        self.runner()


def _nearest_index(n_in, scale):
    """torch F.interpolate(mode="nearest", scale_factor=scale) on a length n_in: output length floor(n_in * scale) (in
    double) and source index min(floor(dst * float(1 / scale)), n_in - 1) in float32, as ATen's nearest kernel does"""
    n_out = int(math.floor(n_in * scale))
    inv = np.float32(1.0 / scale)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * inv).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def extract_hubert(model, audio16k, sampling_rate=24000, shiftms=10):
    """preprocess.py:495-503: ContentVec features of one 16 kHz utterance, (#frames, hidden), resampled to the frame
    shift of the acoustic features by nearest interpolation with scale (sr / int(sr * shiftms / 1000)) * (160 / 16000)
    (1.0 for the recipe's 24 kHz / 10 ms)."""
    h = model.forward(audio16k)[0]  # (T', hidden)
    frame_shift = int(sampling_rate * shiftms / 1000)
    scale = (sampling_rate / frame_shift) * (160 / 16000)
    idx = _nearest_index(h.shape[0], scale)
    if len(idx) == h.shape[0] and (idx == np.arange(h.shape[0])).all():
        return h
    return h.index_select(0, torch.from_numpy(idx).to(h.device))
