"""HIP-backed mirror of ``serenade.vocoder``: HiFiGANGenerator, Vocoder, load_vocoder.

    HiFiGANGenerator   serenade/vocoder/models/hifigan.py:21-284 (+ HiFiGANResidualBlock,
                       serenade/vocoder/layers/residual_block.py:143-258)
    Vocoder            serenade/vocoder/vocoder.py:11-75
    load_vocoder       serenade/vocoder/utils.py:14-63

Same constructor kwargs, method signatures and ``state_dict`` layout (with or without weight
norm), so a parallel_wavegan-style checkpoint ``["model"]["generator"]`` loads unchanged.
Everything is computed channels-last by libserenade_hip.so: the transposed convolutions run as one
implicit-GEMM launch per output phase (2 taps each), every residual-stack conv has the LeakyReLU
fused into its input gather and bias / residual / stage-mean fused into its epilogue.

A generator with ``use_causal_conv`` (CausalConv1d / CausalConvTranspose1d, vocoder/layers/causal_conv.py) loads the
reference's causal key names and, besides the calls above, vocodes in chunks: ``HiFiGANGenerator.stream`` /
``Vocoder.stream`` (CausalHiFiGANPlan, HiFiGANStream); with ``ragged=True`` as B independent sessions that start, idle
and end one by one (HiFiGANSessionStream, VocoderSessions).
"""
import logging
import os
import time

import torch
import yaml

from . import _shapes, ops
from .models import _Packed, _fold_wn
from .plan import FUSED_UNIT_CHANNELS  # noqa: F401  (its public name is vocoder.FUSED_UNIT_CHANNELS)
from .plan import (HistoryArena, LeadTable, LengthTable, causal_mrf_stage_ops, causal_stage_buffers,
                   causal_upsample_ops, conv_op, dev_f32, item_lengths, lru_get, masked, mrf_stage_ops,
                   require_cuda as _require_cuda, rup, upsample_ops)

__all__ = ["HiFiGANGenerator", "HiFiGANStream", "HiFiGANSessionStream", "Vocoder", "VocoderStream",
           "VocoderSessionStream", "VocoderSessions", "load_vocoder", "hifigan_state_shapes"]


def hifigan_state_shapes(**params):
    return _shapes.as_meta(_shapes.hifigan_shapes(**params))


RAGGED_BUCKET = 64  # frames: a ragged plan's capacity is the batch maximum rounded up to this


class _Generator(_Packed):
    """what HiFiGANGenerator and SiFiGANGenerator share: the weight-norm fold and how a ragged plan is found and run.
    A generator says where its ragged plans are cached and what makes one (_ragged_slot: cache, key tag, plan class)."""

    def remove_weight_norm(self):
        """hifigan.py:206-217: replace (weight_g, weight_v) by the folded weight."""

        def walk(m):
            if "weight_g" in m._parameters:
                g, v = m._parameters["weight_g"], m._parameters["weight_v"]
                norm = v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
                w = (v * (g / norm)).detach()
                del m._parameters["weight_g"], m._parameters["weight_v"]
                m.register_parameter("weight", torch.nn.Parameter(w, requires_grad=False))
            for c in m.children():
                walk(c)

        walk(self)
        self._invalidate()

    def plan_ragged(self, B, T_max, bucket=None):
        """the ragged plan for B items of at most T_max frames: its capacity is T_max rounded up to `bucket` frames
        (RAGGED_BUCKET), so one plan serves every batch of B whose longest item falls in the same bucket"""
        T_cap = rup(T_max, RAGGED_BUCKET if bucket is None else int(bucket))
        cache, tag, make = self._ragged_slot()
        return lru_get(cache, tag + (B, T_cap, ops.DEFAULT_PRECISION), 4, lambda: make(self, B, T_cap, ragged=True))

    def _run_ragged(self, B, T_max, lengths, fill):
        """run the ragged plan of (B, T_max): `fill(plan)` writes the items into the plan's input buffers (rows past an
        item's end keep whatever an earlier batch left there: they are never read as data); returns the plan, whose
        outputs hold the result until its next run"""
        pl = self.plan_ragged(B, T_max)
        pl.set_lengths(lengths)
        fill(pl)
        pl.run()
        return pl


class HiFiGANGenerator(_Generator):
    def __init__(self, in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilations=[(1, 3, 5), (1, 3, 5), (1, 3, 5)], use_additional_convs=True, bias=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_causal_conv=False, use_weight_norm=True):
        assert kernel_size % 2 == 1, "Kernel size must be odd number."
        assert len(upsample_scales) == len(upsample_kernel_sizes)
        assert len(resblock_dilations) == len(resblock_kernel_sizes)
        assert bias and out_channels == 1 and nonlinear_activation == "LeakyReLU"
        for s, k in zip(upsample_scales, upsample_kernel_sizes):
            assert k == 2 * s
        super().__init__(_shapes.hifigan_shapes(in_channels, out_channels, channels, kernel_size, upsample_scales,
                                                upsample_kernel_sizes, resblock_kernel_sizes,
                                                [tuple(d) for d in resblock_dilations], use_additional_convs,
                                                weight_norm=use_weight_norm, causal=use_causal_conv))
        self.use_causal_conv = bool(use_causal_conv)
        self.in_channels, self.channels, self.kernel_size = in_channels, channels, kernel_size
        self.upsample_scales = tuple(upsample_scales)
        self.upsample_kernel_sizes = tuple(upsample_kernel_sizes)
        self.resblock_kernel_sizes = tuple(resblock_kernel_sizes)
        self.resblock_dilations = [tuple(d) for d in resblock_dilations]
        self.use_additional_convs = use_additional_convs
        self.slope = float(nonlinear_activation_params.get("negative_slope", 0.01))
        self.num_upsamples = len(upsample_kernel_sizes)
        self.num_blocks = len(resblock_kernel_sizes)
        self.hop = 1
        for s in self.upsample_scales:
            self.hop *= s

    # ------------------------------------------------------------------ reference API
    def apply_weight_norm(self):
        raise NotImplementedError("training-only (hifigan.py:219-230)")

    def register_stats(self, stats):
        """hifigan.py:232-247 (".npy" natively; ".h5" through utils.io.read_hdf5)."""
        assert stats.endswith(".h5") or stats.endswith(".npy")
        import numpy as np
        if stats.endswith(".h5"):
            from .utils.io import read_hdf5
            mean, scale = read_hdf5(stats, "mean").reshape(-1), read_hdf5(stats, "scale").reshape(-1)
        else:
            mean, scale = np.load(stats)[0].reshape(-1), np.load(stats)[1].reshape(-1)
        self.register_buffer("mean", torch.from_numpy(mean).float())
        self.register_buffer("scale", torch.from_numpy(scale).float())

    # ------------------------------------------------------------------ packing / plan
    def packed(self):
        if self._packed is None:
            dev = self._device()
            sd = {k: dev_f32(v, dev) for k, v in self._own_state().items() if k not in ("mean", "scale")}
            # the causal classes hold their conv one module deeper (causal_conv.py:27,62); the packed weights are the same
            conv, deconv = (".conv", ".deconv") if self.use_causal_conv else ("", "")
            P = dict(in_w=ops.pack_conv_weight(_fold_wn(sd, "input_conv" + conv)), in_b=sd[f"input_conv{conv}.bias"],
                     ups=[], blocks=[])
            for i, s in enumerate(self.upsample_scales):
                w = _fold_wn(sd, f"upsamples.{i}.1" + deconv)
                phases = (ops.convtranspose_phases_causal(w, s) if self.use_causal_conv
                          else ops.convtranspose_phases(w, s, s // 2 + s % 2))
                P["ups"].append(dict(phases=phases, b=sd[f"upsamples.{i}.1{deconv}.bias"], cin=w.shape[0],
                                     cout=w.shape[1], s=s))
            for bi in range(self.num_upsamples * self.num_blocks):
                j = bi % self.num_blocks
                k, dil = self.resblock_kernel_sizes[j], self.resblock_dilations[j]
                convs = []
                for idx, d in enumerate(dil):
                    p1 = f"blocks.{bi}.convs1.{idx}.1" + conv
                    c = dict(d=d, k=k, w1=ops.pack_conv_weight(_fold_wn(sd, p1)), b1=sd[p1 + ".bias"])
                    if self.use_additional_convs:
                        p2 = f"blocks.{bi}.convs2.{idx}.1" + conv
                        c.update(w2=ops.pack_conv_weight(_fold_wn(sd, p2)), b2=sd[p2 + ".bias"])
                    convs.append(c)
                P["blocks"].append(convs)
            wo = _fold_wn(sd, "output_conv.1" + conv)  # (1, C, k)
            P["out_w"] = wo[0].t().contiguous()  # (k, C)
            P["out_b"] = sd[f"output_conv.1{conv}.bias"]
            self._packed = P
        return self._packed

    def plan(self, B, T):
        key = (B, T, ops.DEFAULT_PRECISION)
        make = CausalHiFiGANPlan if self.use_causal_conv else HiFiGANPlan
        return lru_get(self._plans, key, 4, lambda: make(self, B, T))

    def _ragged_slot(self):
        # the dense plans' LRU, the key tagged.  A causal generator's ragged plan is its dense plan at the bucket's
        # length plus one op that zeroes the tails (CausalHiFiGANPlan)
        return self._plans, ("ragged",), CausalHiFiGANPlan if self.use_causal_conv else HiFiGANPlan

    def stream(self, B, chunk_frames, ragged=False):
        """a HiFiGANStream: B utterances vocoded side by side, at most chunk_frames frames per push().  Causal
        generators only -- ValueError otherwise, and for chunk_frames < 1, before anything is built or launched.
        ragged=True: a HiFiGANSessionStream -- B independent sessions, push(c, lengths, restart)."""
        if not self.use_causal_conv:
            raise ValueError("HiFiGANGenerator.stream: only a generator with use_causal_conv can be run in chunks "
                             "(a non-causal output row depends on later input rows)")
        if int(B) < 1 or int(chunk_frames) < 1:
            raise ValueError(f"HiFiGANGenerator.stream: B = {B}, chunk_frames = {chunk_frames} must be at least 1")
        return (HiFiGANSessionStream if ragged else HiFiGANStream)(self, int(B), int(chunk_frames))

    @torch.no_grad()
    def forward(self, c):
        """(B, in_channels, T) -> (B, 1, T * hop)   (hifigan.py:171-190)."""
        _require_cuda(c, "HiFiGANGenerator.forward")
        return self._run_cl(c.detach().to(torch.float32).transpose(1, 2).contiguous())

    def _run_cl(self, c_cl):
        B, T, _ = c_cl.shape
        pl = self.plan(B, T)
        pl.c_in.copy_(c_cl)
        pl.run()
        return pl.wave.clone().unsqueeze(1)

    @torch.no_grad()
    def inference(self, c, normalize_before=False):
        """(T, in_channels) -> (T * hop, 1)   (hifigan.py:249-265)."""
        if not isinstance(c, torch.Tensor):
            c = torch.tensor(c, dtype=torch.float).to(self._device())
        _require_cuda(c, "HiFiGANGenerator.inference")
        if normalize_before:
            c = (c - self.mean) / self.scale
        y = self._run_cl(c.detach().to(torch.float32).unsqueeze(0).contiguous())
        return y.squeeze(0).transpose(1, 0)

    @torch.no_grad()
    def inference_batch(self, c, normalize_before=False, lengths=None):
        """(B, T, in_channels) -> (B, 1, T * hop)   (hifigan.py:267-284).  lengths (B frame counts in [1, T]): the
        batch is ragged -- item b is vocoded as its own B = 1 call on its first lengths[b] frames (the rows behind
        them may hold anything) and the output is zero past lengths[b] * hop.
        A causal generator runs its dense plan at the longest length and zeroes the output past lengths[b] * hop.  That
        is exact: no output row of a causal generator depends on a later input row, so the first lengths[b] * hop
        samples of item b are what its own B = 1 call gives, whatever the rows behind its end hold."""
        if not isinstance(c, torch.Tensor):
            c = torch.tensor(c, dtype=torch.float).to(self._device())
        _require_cuda(c, "HiFiGANGenerator.inference_batch")
        if lengths is not None:
            lengths = item_lengths(lengths, c.shape[0], c.shape[1], "HiFiGANGenerator.inference_batch")
        if normalize_before:
            c = (c - self.mean) / self.scale
        c = c.detach().to(torch.float32).contiguous()
        if lengths is None:
            return self._run_cl(c)
        pl = self._run_ragged(c.shape[0], c.shape[1], lengths, lambda pl: pl.c_in[:, :c.shape[1]].copy_(c))
        return pl.wave[:, :c.shape[1] * self.hop].clone().unsqueeze(1)

    @torch.no_grad()
    def inference_ragged(self, cs, normalize_before=False):
        """[(T_b, in_channels)] -> [(T_b * hop,)]: utterances of different lengths in ONE call, each computed as its
        own B = 1 inference."""
        cs = [c if isinstance(c, torch.Tensor) else torch.tensor(c, dtype=torch.float).to(self._device()) for c in cs]
        if not cs:
            raise ValueError("HiFiGANGenerator.inference_ragged: no items")
        for c in cs:
            _require_cuda(c, "HiFiGANGenerator.inference_ragged")
        if normalize_before:
            cs = [(c - self.mean) / self.scale for c in cs]
        lengths = item_lengths([c.shape[0] for c in cs], len(cs), max(c.shape[0] for c in cs),
                               "HiFiGANGenerator.inference_ragged")

        def fill(pl):
            for b, c in enumerate(cs):
                pl.c_in[b, :c.shape[0]].copy_(c.detach())
        pl = self._run_ragged(len(cs), max(lengths), lengths, fill)
        return [pl.wave[b, :n * self.hop].clone() for b, n in enumerate(lengths)]


class HiFiGANPlan:
    """Buffers + op list of one generator forward for (B, T).  Input: self.c_in (B, T, in_ch) channels-last;
    output: self.wave (B, T * hop).

    ragged: the lengths are data -- one plan (and one captured graph) for every batch of B items whose longest has at
    most T frames.  Rows of c_in at or past an item's length may hold anything, wave is zero past each item's end, and
    item b is computed as its own B = 1 dense plan of lengths[b] frames computes it.  self.lens (plan.LengthTable: row 0
    for the mel frames, row i + 1 behind upsample i) holds what set_lengths() was given; every conv gets its input
    stage's row as len_in, the fused units and the output stage run their ragged entry points."""

    def __init__(self, gen, B, T, ragged=False):
        P = gen.packed()
        dev = gen._device()
        self.B, self.T = B, T
        lens = [None] * (len(P["ups"]) + 1)
        if ragged:
            table = LengthTable(gen.upsample_scales, B, dev)
            self.lens, self.scales, self.set_lengths, lens = table.lens, table.scales, table.set_lengths, table.rows
        self.c_raw = None  # Vocoder's ragged batch in front of the renormalisation: allocated when first used
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.c_in = f(B, T, gen.in_channels)
        C0 = gen.channels
        h = f(B, T, C0)
        # widest (T_i * C_i) stage decides the ping-pong buffer size
        big, t = 0, T
        for up in P["ups"]:
            t *= up["s"]
            big = max(big, t * up["cout"])
        u, p0, p1, xt, acc = (f(B * big) for _ in range(5))
        self.wave = f(B, t)
        nb = gen.num_blocks
        ol = [conv_op(B, self.c_in, gen.in_channels, T, P["in_w"], P["in_b"], h, C0, T, ops.conv_taps(gen.kernel_size),
                      **masked(lens[0]))]
        cur, ccur, tcur = h, C0, T
        for i, up in enumerate(P["ups"]):
            # the upsample reads `cur` (h, then acc) and writes `u`; the blocks overwrite acc only at their end
            upsample_ops(ol, B, cur, ccur, tcur, up, u, gen.slope, len_in=lens[i])
            cur, ccur, tcur = acc, up["cout"], tcur * up["s"]
            mrf_stage_ops(ol, B, u, p0, p1, xt, acc, P["blocks"][i * nb:(i + 1) * nb], ccur, tcur, gen.slope,
                          lens[i + 1])
        ol.append(ops.out_conv_tanh_op(cur, P["out_w"], P["out_b"], self.wave, B, tcur, ccur, gen.kernel_size, 0.01,
                                       lens=lens[-1]))
        self.ops = ol
        self._runner = ops.GraphRunner(lambda: self.ops)

    def run(self):
        self._runner()


class CausalHiFiGANPlan:
    """Buffers + op list of a causal generator (use_causal_conv) for B items of T frames: ONE builder for the one-shot
    forward and for a stream's chunk.  Input: self.c_in (B, T, in_ch) channels-last; output: self.wave (B, T * hop).

    Every conv reads a [history | chunk] buffer of its own (plan.HistoryArena) as a valid conv; histories of zeros are
    the causal padding, self.lead (plan.LeadTable) tells the fused units and the replication pad of the up-sampling
    how much of an item's utterance lies before this call.  The one-shot plan is this op list run with zero histories
    and every lead 0: nothing it runs writes a history row, so it can be run again and again.  carry=True (a stream's
    plan) appends the ops that move every buffer's last H rows to its front; HiFiGANStream advances the leads.

    carry="ragged" (HiFiGANSessionStream's plan): B independent sessions.  In front, one srn_history_carry_ragged over
    the restart flags zeroes the histories of the items that begin an utterance; behind the compute ops, self.wave is
    zeroed past lengths[b] * hop; last, one srn_history_carry_ragged over the pushed counts moves each item's rows
    [n_b scale, n_b scale + H) to the front (an idle item keeps its state).  set_push() rewrites the counts, the flags
    and the per-item leads in place.

    ragged=True: lengths as data the cheap way -- the dense causal plan at T frames, then self.wave zeroed past
    lengths[b] * hop (set_lengths).  Exact, since no output row depends on a later input row."""

    def __init__(self, gen, B, T, ragged=False, carry=False):
        P = gen.packed()
        dev = gen._device()
        self.B, self.T = B, T
        self.c_raw = None  # Vocoder's ragged batch in front of the renormalisation: allocated when first used
        ks, cin, C0, n_up = gen.kernel_size, gen.in_channels, gen.channels, len(P["ups"])
        nb = gen.num_blocks
        arena = HistoryArena(B, dev)
        arena.add("c", ks - 1, T, cin)
        arena.add("h", 1, T, C0)
        t = T
        for i, up in enumerate(P["ups"]):
            t *= up["s"]
            causal_stage_buffers(arena, i, P["blocks"][i * nb:(i + 1) * nb], up["cout"], t, 1 if i + 1 < n_up else ks - 1)
        arena.allocate()
        self.arena = arena
        self.leads = LeadTable(gen.upsample_scales, B, dev)
        lead = self.leads.rows
        self.c_in = torch.zeros(B, T, cin, device=dev, dtype=torch.float32)
        self.wave = torch.zeros(B, t, device=dev, dtype=torch.float32)
        c, h = arena["c"], arena["h"]
        # c_in stays one contiguous (B, T, in_ch) tensor for its writers (srn_renorm, copy_); its rows go behind the
        # input conv's history here
        ol = [ops.copy_channels_op(self.c_in, T * cin, cin, 0, c.chunk, c.bs, cin, 0, B, T, cin),
              conv_op(B, c.row(0), cin, ks - 1 + T, P["in_w"], P["in_b"], h.chunk, C0, T, range(ks), out_bs=h.bs)]
        cur, tcur = h, T
        for i, up in enumerate(P["ups"]):
            causal_upsample_ops(ol, B, cur, up, arena[f"u{i}"], gen.slope, lead[i])
            tcur *= up["s"]
            causal_mrf_stage_ops(ol, B, arena, i, P["blocks"][i * nb:(i + 1) * nb], up["cout"], tcur, gen.slope,
                                 lead[i + 1])
            cur = arena[f"acc{i}"]
        ol.append(ops.out_conv_tanh_causal_op(cur.row(0), P["out_w"], P["out_b"], self.wave, B, tcur, cur.C, ks, 0.01))
        if ragged:
            self.lens_out = torch.zeros(B, dtype=torch.int32, device=dev)
            self._hop = tcur // T
            ol.append(ops.zero_rows_ragged_op(self.wave, tcur, 1, self.lens_out, B, tcur))
        if carry == "ragged":
            # a stream of B independent sessions: what differs between pushes is self.push (restart, frames pushed and
            # samples valid per item) and the leads, all rewritten in place by set_push() outside the captured graph
            if ragged:
                raise ValueError("CausalHiFiGANPlan: carry='ragged' zeroes the tails itself; ragged=True is the "
                                 "one-shot form")
            self.push = torch.zeros(3, B, dtype=torch.int32, device=dev)
            restart, pushed, valid = self.push.unbind(0)
            self._hop = tcur // T
            ol = (arena.carry_ragged_ops(restart, T) + ol + [ops.zero_rows_ragged_op(self.wave, tcur, 1, valid, B, tcur)]
                  + arena.carry_ragged_ops(pushed, T))
        elif carry:
            ol += arena.carry_ops()
        self.ops = ol
        self._runner = ops.GraphRunner(lambda: self.ops)

    def set_lengths(self, lengths):
        """lengths: B frame counts in [1, T] (validated by the caller, item_lengths); a ragged plan's only"""
        self.lens_out.copy_(torch.tensor([int(n) * self._hop for n in lengths], dtype=torch.int32))

    def set_push(self, lengths, restart, before):
        """a carry="ragged" plan's only, before each run: item b gives lengths[b] frames in [0, T], begins a new
        utterance with them where restart[b], and had `before[b]` frames of this utterance before this run (0 where it
        restarts); all validated by the caller"""
        host = torch.tensor([[-1 if r else 0 for r in restart], [int(n) for n in lengths],
                             [int(n) * self._hop for n in lengths]], dtype=torch.int32)
        self.push.copy_(host)
        self.leads.set_pushed_items(before)

    def restart(self):
        """zero histories, every lead 0: the next run begins B new utterances"""
        self.arena.t.zero_()
        self.leads.set_pushed(0)

    def run(self):
        self._runner()


class HiFiGANStream:
    """B utterances through a causal generator, chunk by chunk: push() takes (B, n <= chunk_frames, in_channels) and
    returns the next (B, n * hop) samples -- together, the chunks' outputs are the one-shot forward of the
    concatenated input (no output row depends on a later input row; the few rows of state per conv live in the plan's
    [history | chunk] buffers).  Every push runs the SAME op list (with graphs on, the same captured graph): what
    differs between chunks is device data -- the carried histories and the leads.

    A chunk shorter than chunk_frames is run padded (the rows behind it keep the previous chunk's) and the surplus
    output dropped, which is exact for the same reason; it ends the stream, since the carried rows then are not the
    utterance's last: push() after it raises until reset().  The stream runs on the generator's one plan for
    (B, chunk_frames): two live streams of the same shape on one generator would share their state."""

    def __init__(self, gen, B, chunk_frames):
        self.gen, self.B, self.chunk_frames = gen, B, chunk_frames
        self._pl = None
        self.frames = 0  # pushed so far
        self._ended = False

    def _plan(self):
        if self._pl is None:
            g = self.gen
            key = ("stream", self.B, self.chunk_frames, ops.DEFAULT_PRECISION)
            self._pl = lru_get(g._plans, key, 4, lambda: CausalHiFiGANPlan(g, self.B, self.chunk_frames, carry=True))
            self._pl.restart()
        return self._pl

    def check(self, c):
        """ValueError unless `c` is a chunk this stream takes; nothing is built or launched"""
        if c.dim() != 3 or c.shape[2] != self.gen.in_channels:
            raise ValueError(f"HiFiGANStream.push: expected (B, n, {self.gen.in_channels}), got {tuple(c.shape)}")
        if c.shape[0] != self.B:
            raise ValueError(f"HiFiGANStream.push: the stream holds {self.B} utterances, the chunk {c.shape[0]}")
        if not 1 <= c.shape[1] <= self.chunk_frames:
            raise ValueError(f"HiFiGANStream.push: a chunk has 1 to {self.chunk_frames} frames, not {c.shape[1]}")
        if self._ended:
            raise ValueError("HiFiGANStream.push: a short chunk ended this stream; reset() begins the next")

    @torch.no_grad()
    def push(self, c):
        self.check(c)
        _require_cuda(c, "HiFiGANStream.push")
        pl, n = self._plan(), c.shape[1]
        pl.c_in[:, :n].copy_(c.detach())
        pl.run()
        y = pl.wave[:, :n * self.gen.hop].clone()
        self.frames += n
        self._ended = n < self.chunk_frames
        pl.leads.set_pushed(self.frames)
        return y

    def reset(self):
        """begin B new utterances"""
        self.frames, self._ended = 0, False
        if self._pl is not None:
            self._pl.restart()


def _per_item(values, B, what, name):
    """B per-item values (tensor, numpy or sequence) as a list; ValueError unless there are B"""
    vals = list(values.tolist() if hasattr(values, "tolist") else values)
    if len(vals) != B:
        raise ValueError(f"{what}: {name} holds {len(vals)} values, the stream {B} sessions")
    return vals


class HiFiGANSessionStream:
    """B independent sessions through a causal generator (HiFiGANGenerator.stream(..., ragged=True)): push(c, lengths,
    restart) takes c (B, n_max <= chunk_frames, in_channels), of which item b gives its first lengths[b] in [0, n_max]
    frames, and returns (B, n_max * hop), zero past lengths[b] * hop.  Item b begins a new utterance with this chunk
    where restart[b]; every slot begins restarted.

    Between two restarts, the concatenation of item b's valid output is the generator's one-shot call on the
    concatenation of its valid input.  Rows of c at or past lengths[b] are never read as data (they may hold NaN), and
    neither is another item's state; an item that gives no frames keeps its state, so a short or empty chunk ends
    nothing.  Every push runs the SAME op list (with graphs on, the same captured graph): the lengths, the restart
    flags and the leads are device data (CausalHiFiGANPlan carry="ragged").  The stream owns its plan -- it is not taken
    from the generator's plan cache -- so two live streams never share state."""

    def __init__(self, gen, B, chunk_frames):
        self.gen, self.B, self.chunk_frames = gen, B, chunk_frames
        self._pl = None
        self.frames = [0] * B  # per session, pushed since its utterance began

    def _plan(self):
        if self._pl is None:
            self._pl = CausalHiFiGANPlan(self.gen, self.B, self.chunk_frames, carry="ragged")
        return self._pl

    def check(self, c, lengths, restart=None):
        """ValueError unless (c, lengths, restart) is a push this stream takes; nothing is built or launched.  Returns
        the lengths as ints and the restart flags as bools."""
        what = "HiFiGANSessionStream.push"
        if c.dim() != 3 or c.shape[2] != self.gen.in_channels:
            raise ValueError(f"{what}: expected (B, n, {self.gen.in_channels}), got {tuple(c.shape)}")
        if c.shape[0] != self.B:
            raise ValueError(f"{what}: the stream holds {self.B} sessions, the chunk {c.shape[0]}")
        if not 1 <= c.shape[1] <= self.chunk_frames:
            raise ValueError(f"{what}: a chunk has 1 to {self.chunk_frames} frames, not {c.shape[1]}")
        lens = [int(n) for n in _per_item(lengths, self.B, what, "lengths")]
        if min(lens) < 0 or max(lens) > c.shape[1]:
            raise ValueError(f"{what}: lengths {tuple(lens)} must lie in [0, {c.shape[1]}]")
        flags = [False] * self.B if restart is None else [bool(r) for r in _per_item(restart, self.B, what, "restart")]
        return lens, flags

    @torch.no_grad()
    def push(self, c, lengths, restart=None):
        lens, flags = self.check(c, lengths, restart)
        _require_cuda(c, "HiFiGANSessionStream.push")
        pl, n_max = self._plan(), c.shape[1]
        before = [0 if r else f for r, f in zip(flags, self.frames)]
        pl.set_push(lens, flags, before)
        pl.c_in[:, :n_max].copy_(c.detach())
        pl.run()
        y = pl.wave[:, :n_max * self.gen.hop].clone()
        self.frames = [f + n for f, n in zip(before, lens)]
        return y


def load_vocoder(checkpoint, config=None, stats=None):
    """serenade/vocoder/utils.py:14-63."""
    if config is None:
        with open(os.path.join(os.path.dirname(checkpoint), "config.yml")) as f:
            config = yaml.load(f, Loader=yaml.Loader)
    generator_type = config.get("generator_type", "HiFiGANGenerator")
    generator_params = {k.replace("upsample_kernal_sizes", "upsample_kernel_sizes"): v
                        for k, v in config["generator_params"].items()}
    model = HiFiGANGenerator(**generator_params)
    model.load_state_dict(torch.load(checkpoint, map_location="cpu")["model"]["generator"])
    if stats is None:
        ext = "h5" if config["format"] == "hdf5" else "npy"
        cand = os.path.join(os.path.dirname(checkpoint), f"stats.{ext}")
        if os.path.exists(cand):
            stats = cand
    if stats is not None and generator_type != "VQVAE":
        model.register_stats(stats)
    return model


class Vocoder(object):
    """serenade/vocoder/vocoder.py:11-75."""

    def __init__(self, checkpoint, config, stats, device, trg_stats=None, take_norm_feat=True):
        with open(config) as f:
            cfg = yaml.load(f, Loader=yaml.Loader)
        model = load_vocoder(checkpoint, cfg)
        logging.info(f"Loaded model parameters from {checkpoint}.")
        from .utils.io import read_feats  # .h5 (h5py) like the reference, or .npz with the same keys
        st = {"mean": read_feats(stats, "mean"), "scale": read_feats(stats, "scale")}
        self._setup(model, cfg, st, device, trg_stats, take_norm_feat)

    @classmethod
    def from_generator(cls, model, config, stats, device, trg_stats=None, take_norm_feat=True):
        """Build from an in-memory generator and stats dict (synthetic runs: no checkpoint files exist offline)."""
        self = cls.__new__(cls)
        self._setup(model, config, stats, device, trg_stats, take_norm_feat)
        return self

    def _setup(self, model, config, stats, device, trg_stats, take_norm_feat):
        self.device = device
        if take_norm_feat:
            assert trg_stats is not None, "trg_stats must be given if take_norm_feat=True"
            self.trg_stats = {k: torch.tensor(trg_stats[k], dtype=torch.float).to(device).contiguous()
                              for k in ("mean", "scale")}
        self.take_norm_feat = take_norm_feat
        self.config = config
        self.model = model
        self.model.remove_weight_norm()
        self.model = self.model.eval().to(device)
        self.stats = {k: torch.tensor(stats[k], dtype=torch.float).to(device).contiguous()
                      for k in ("mean", "scale")}

    def _decode_cl(self, c):
        """c (B, T, 80) normalised mel -> (B, T * hop): both affine maps and the generator on the GPU."""
        _require_cuda(c, "Vocoder.decode")
        pl = self.model.plan(c.shape[0], c.shape[1])
        self._renorm_run(c.detach().to(torch.float32).contiguous(), pl)
        return pl.wave.clone()

    def _renorm_run(self, c, pl):
        """c (B, T, 80) -> pl.c_in in ONE srn_renorm, then the plan"""
        B, T, C = c.shape
        ts = self.trg_stats if self.take_norm_feat else {"scale": None, "mean": None}
        ops.renorm_op(c, ts["scale"], ts["mean"], self.stats["mean"], self.stats["scale"], pl.c_in, B * T, C)()
        pl.run()

    @torch.no_grad()
    def decode(self, c):
        """(T, 80) -> ((T * hop,), sampling_rate)   (vocoder.py:51-62)."""
        start = time.time()
        y = self._decode_cl(c.unsqueeze(0)).view(-1)
        rtf = (time.time() - start) / (len(y) / self.config["sampling_rate"])
        logging.info(f"Finished waveform generation. (RTF = {rtf:.03f}).")
        return y, self.config["sampling_rate"]

    @torch.no_grad()
    def decode_batch(self, c, lengths=None):
        """(B, T, 80) -> (B, T * hop)   (vocoder.py:64-75).  lengths (B frame counts in [1, T]): a ragged batch, as
        HiFiGANGenerator.inference_batch takes it -- zeros past each item's end."""
        if lengths is None:
            return self._decode_cl(c)
        _require_cuda(c, "Vocoder.decode_batch")
        B, T, _ = c.shape
        lengths = item_lengths(lengths, B, T, "Vocoder.decode_batch")
        pl = self._decode_ragged(B, T, lengths, lambda raw: raw[:, :T].copy_(c.detach()))
        return pl.wave[:, :T * self.model.hop].clone()

    @torch.no_grad()
    def decode_ragged(self, mels):
        """[(T_b, 80) normalised mels] -> [(T_b * hop,) waveforms]: one vocoder call for utterances of different
        lengths, each computed as its own decode()."""
        mels = list(mels)
        if not mels:
            raise ValueError("Vocoder.decode_ragged: no items")
        for m in mels:
            _require_cuda(m, "Vocoder.decode_ragged")
        lengths = item_lengths([m.shape[0] for m in mels], len(mels), max(m.shape[0] for m in mels),
                               "Vocoder.decode_ragged")

        def fill(raw):
            for b, m in enumerate(mels):
                raw[b, :m.shape[0]].copy_(m.detach())
        pl = self._decode_ragged(len(mels), max(lengths), lengths, fill)
        return [pl.wave[b, :n * self.model.hop].clone() for b, n in enumerate(lengths)]

    def stream(self, B, chunk_frames, ragged=False):
        """decode_batch in chunks, for a causal generator: a VocoderStream whose push() takes (B, n <= chunk_frames,
        80) normalised mel and returns the next (B, n * hop) samples (HiFiGANGenerator.stream behind both
        renormalisations).  ragged=True: a VocoderSessionStream -- B independent sessions, push(c, lengths, restart)."""
        if ragged:
            return VocoderSessionStream(self, self.model.stream(B, chunk_frames, ragged=True))
        return VocoderStream(self, self.model.stream(B, chunk_frames))

    def _decode_ragged(self, B, T_max, lengths, fill):
        """the padded batch goes through the one srn_renorm (all T_cap rows of every item: the rows past an item's end
        are renormalised leftovers, never read as data), then through the ragged plan"""
        pl = self.model.plan_ragged(B, T_max)
        if pl.c_raw is None:
            pl.c_raw = torch.zeros_like(pl.c_in)
        pl.set_lengths(lengths)
        fill(pl.c_raw)
        self._renorm_run(pl.c_raw, pl)
        return pl


def _renormed(v, c):
    """a chunk (B, n, 80) through the two affine maps of Vocoder `v` (vocoder.py:52-56) in ONE srn_renorm, into a
    tensor of its own"""
    c = c.detach().to(torch.float32).contiguous()
    y = torch.empty_like(c)
    ts = v.trg_stats if v.take_norm_feat else {"scale": None, "mean": None}
    ops.renorm_op(c, ts["scale"], ts["mean"], v.stats["mean"], v.stats["scale"], y, c.shape[0] * c.shape[1], c.shape[2])()
    return y


class VocoderStream:
    """Vocoder.stream: a HiFiGANStream behind the two affine maps of Vocoder.decode (vocoder.py:52-56)"""

    def __init__(self, vocoder, stream):
        self.vocoder, self.stream = vocoder, stream

    @torch.no_grad()
    def push(self, c):
        self.stream.check(c)
        _require_cuda(c, "VocoderStream.push")
        return self.stream.push(_renormed(self.vocoder, c))

    def reset(self):
        self.stream.reset()


class VocoderSessionStream:
    """Vocoder.stream(..., ragged=True): a HiFiGANSessionStream behind the two affine maps of Vocoder.decode
    (vocoder.py:52-56).  Rows of c past an item's length are renormalised like the rest and never read as data."""

    def __init__(self, vocoder, stream):
        self.vocoder, self.stream = vocoder, stream

    @torch.no_grad()
    def push(self, c, lengths, restart=None):
        lens, flags = self.stream.check(c, lengths, restart)
        _require_cuda(c, "VocoderSessionStream.push")
        return self.stream.push(_renormed(self.vocoder, c), lens, flags)


class VocoderSessions:
    """Live sessions over ONE VocoderSessionStream of `slots` items, host bookkeeping only (no threads): open() gives a
    free slot, feed(slot, mel) queues (n, 80) normalised mel frames, step() takes up to chunk_frames queued frames from
    every open slot, runs one push and returns {slot: the next waveform samples} for the slots that gave frames,
    close(slot) frees the slot once its queue is drained.  A reopened slot begins a new utterance."""

    def __init__(self, vocoder, slots, chunk_frames):
        self.stream = vocoder.stream(slots, chunk_frames, ragged=True)
        self.vocoder, self.slots, self.chunk_frames = vocoder, int(slots), int(chunk_frames)
        self._queue = [None] * self.slots    # per slot: its queued (n, 80) pieces; None: the slot is free
        self._fresh = [False] * self.slots   # opened, not pushed yet: its next push restarts it
        self._closing = [False] * self.slots

    def open(self):
        for slot, q in enumerate(self._queue):
            if q is None:
                self._queue[slot], self._fresh[slot], self._closing[slot] = [], True, False
                return slot
        raise RuntimeError(f"VocoderSessions.open: all {self.slots} slots are in use")

    def _live(self, slot, what):
        if not (isinstance(slot, int) and 0 <= slot < self.slots) or self._queue[slot] is None:
            raise ValueError(f"VocoderSessions.{what}: slot {slot} is not open")

    def feed(self, slot, mel):
        self._live(slot, "feed")
        C = self.vocoder.model.in_channels
        if self._closing[slot]:
            raise ValueError(f"VocoderSessions.feed: slot {slot} is closing")
        if mel.dim() != 2 or mel.shape[1] != C:
            raise ValueError(f"VocoderSessions.feed: expected (n, {C}), got {tuple(mel.shape)}")
        if mel.shape[0]:
            self._queue[slot].append(mel.detach())

    def queued(self, slot):
        """frames of `slot` waiting for a step()"""
        self._live(slot, "queued")
        return sum(m.shape[0] for m in self._queue[slot])

    def close(self, slot):
        """no more frames for `slot`: it is freed at once if its queue is empty, else by the step() that drains it"""
        self._live(slot, "close")
        self._closing[slot] = True
        self._release()

    def _release(self):
        for slot, q in enumerate(self._queue):
            if q is not None and self._closing[slot] and not q:
                self._queue[slot], self._closing[slot] = None, False

    def _take(self, slot):
        """up to chunk_frames frames from the front of the slot's queue, as one (n, 80) tensor or None"""
        q, got, n = self._queue[slot], [], 0
        while q and n < self.chunk_frames:
            m = q.pop(0)
            room = self.chunk_frames - n
            if m.shape[0] > room:
                q.insert(0, m[room:])
                m = m[:room]
            got.append(m)
            n += m.shape[0]
        return torch.cat(got) if got else None

    def step(self):
        taken = {slot: self._take(slot) for slot, q in enumerate(self._queue) if q is not None}
        lens = [0 if taken.get(b) is None else taken[b].shape[0] for b in range(self.slots)]
        if max(lens) == 0:
            return {}
        c = torch.zeros(self.slots, max(lens), self.vocoder.model.in_channels, device=self.vocoder.device)
        for b, m in taken.items():
            if m is not None:
                c[b, :m.shape[0]].copy_(m)
        restart = [self._fresh[b] and b in taken for b in range(self.slots)]
        y = self.stream.push(c, lens, restart)
        hop = self.vocoder.model.hop
        for b in taken:
            self._fresh[b] = False
        self._release()
        return {b: y[b, :lens[b] * hop].clone() for b in taken if lens[b]}
