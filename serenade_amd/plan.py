"""What every plan builder shares: the small helpers, the op builders that several plans repeat (batched conv, dense
layer, chunked self-attention, the stages and the length table of the HiFi-GAN / SiFiGAN generators, the height table
of the ragged style encoder) and the input / state-dict checks of the waveform front-ends.  A plan is a list of
prebuilt C-ABI calls (``ops.ConvOp`` / ``ops.CallOp``) over preallocated buffers; nothing here launches anything.
"""
import math

import numpy as np
import torch

from . import ops
from .ops import ConvOp


def rup(x, m):
    return (x + m - 1) // m * m


def require_cuda(t, what):
    """the guard in front of every entry point.  A module binds it under a name of its own (`_require_cuda`): the C-ABI
    emulator of the CPU tests lifts the guard module by module through that name."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")


def dev_f32(t, dev):
    """private fp32 device copy: packed weights never alias a live nn.Parameter, so an in-place reload of the
    parameter (load_state_dict) cannot change -- or be missed by -- anything derived from the packed tensor"""
    r = t.detach().to(device=dev, dtype=torch.float32).contiguous()
    return r.clone() if r.data_ptr() == t.data_ptr() else r


def dev_i32(values, dev):
    """int32 device copy of a sequence of integers (per-item counts, offset tables)"""
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=dev)


def dev_f64(a, dev):
    """float64 device copy of a host table (array-like)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def lru_get(cache, key, capacity, make):
    """dict used as an LRU (insertion order = recency): a hit moves the entry to the back, a miss evicts only the
    least recently used entries beyond `capacity` -- never the plan in use (the B = 1 decode loop sees a new length
    with almost every utterance; GroupNorm runs over the padded length, so lengths cannot be bucketed)."""
    if key in cache:
        cache[key] = cache.pop(key)
    else:
        cache[key] = make()
        while len(cache) > capacity:
            cache.pop(next(iter(cache)))
    return cache[key]


def tensors_of(obj):
    """all tensors inside a nested dict / list / tuple"""
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from tensors_of(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from tensors_of(v)


# ---------------------------------------------------------------------------------------------- contractions
def conv_op(B, inp, cin, T_in, w, b, out, cout, T_out, taps, ld_in=None, **kw):
    """Conv1d over a (B, T_in, cin) channels-last batch into (B, T_out, cout): packed weight `w`, bias `b`, input-row
    offsets `taps`.  ld_in: row length of `inp` when it is wider than cin; in_bs / out_bs / ld_out override the dense
    item strides (a window of a longer buffer)."""
    ld_in = cin if ld_in is None else ld_in
    return ConvOp(in0=inp, w=w, out=out, n_batch=B, T_in=T_in, T_out=T_out, C_in=cin, N=cout,
                  in0_bs=kw.pop("in_bs", T_in * ld_in), ld_in0=ld_in, ldw=w.shape[1], out_bs=kw.pop("out_bs", T_out * cout),
                  ld_out=kw.pop("ld_out", cout), bias=b, taps=taps, **kw)


def linear_op(inp, rows, K, w, b, out, N, **kw):
    """out (rows, N) = inp (rows, K) w^T + b, all rows of a batch as one contraction"""
    return ConvOp(in0=inp, w=w, out=out, n_batch=1, T_in=rows, T_out=rows, C_in=K, N=N, ld_in0=K, ldw=w.shape[1],
                  ld_out=N, bias=b, **kw)


# ---------------------------------------------------------------------------------------------- generator stages
# What the HiFi-GAN and SiFiGAN plans share (vocoder.py, sifigan.py).  Lengths are optional everywhere: None makes the
# dense plan; a (B,) int32 device tensor makes the length data -- a conv reads rows at or past its input's length as the
# zeros an item alone would be padded with (len_in), the fused unit runs its ragged entry point.
FUSED_UNIT_CHANNELS = (32, 64)  # stage widths whose residual units run as one fused launch (srn_hifigan_resunit)


def fused_unit(cv, C):
    """whether the two-conv unit `cv` (packed: k, d, w1, ..., w2) of a C-channel stage runs as one fused launch"""
    return "w2" in cv and C in FUSED_UNIT_CHANNELS and (cv["k"] - 1) * cv["d"] <= 50 and cv["k"] % 2 == 1


def masked(lens, out=False):
    """the length keywords of a conv whose input has `lens` rows per item (out: whose output is cut to them as well,
    stored as 0 behind them); none for the dense plan's None"""
    if lens is None:
        return {}
    return {"len_in": lens, "len_out": lens} if out else {"len_in": lens}


def upsample_ops(ol, B, src, csrc, tsrc, up, out, slope, emb=None, len_in=None):
    """the transposed conv of one stage, LeakyReLU in front: one conv per output phase (2 taps each) from `src`
    (B, tsrc, csrc) into `out` (B, tsrc * s, cout).  up: the packed entry (phases, b, s, cout); emb: a residual
    (B, tsrc * s, cout) added to the result; len_in: the lengths of the stage below, which a phase reads."""
    s, co = up["s"], up["cout"]
    res = {} if emb is None else dict(res=emb, res_mode=ops.RES_ADD, res_bs=tsrc * s * co, ld_res=co)
    for r, (taps, wp) in enumerate(up["phases"]):
        ol.append(conv_op(B, src, csrc, tsrc, wp, up["b"], out, co, tsrc, taps, pro_act=ops.ACT_LEAKY, pro_slope=slope,
                          out_bs=tsrc * s * co, out_t_stride=s, out_t_off=r, **res, **masked(len_in)))


def mrf_stage_ops(ol, B, u, p0, p1, xt, acc, blocks, C, T, slope, lens=None):
    """one multi-receptive-field stage: acc = mean over `blocks` of block(u), all (B, T, C).  blocks: per block its
    packed convs (k, d, w1, b1 and, for the two-conv unit, w2, b2); p0 / p1 ping-pong between a block's units, xt holds
    the middle of an unfused two-conv unit; lens: the stage's lengths."""
    nb = len(blocks)
    for j, convs in enumerate(blocks):
        x = u
        for idx, cv in enumerate(convs):
            last = idx == len(convs) - 1
            dst = acc if last else (p0, p1)[idx % 2]
            fin = {}
            if last:
                # cs += block(c); c = cs / num_blocks  (hifigan.py:183-186), in the reference's order
                if j > 0:
                    fin.update(res2=acc, res2_bs=T * C, ld_res2=C)
                if j == nb - 1:
                    fin.update(post=ops.POST_DIV, post_div=float(nb))
            skip = dict(res=x, res_mode=ops.RES_ADD, res_bs=T * C, ld_res=C, **fin, **masked(lens))
            if fused_unit(cv, C):
                # thin stage: the whole unit in one launch (resunit.hip); stage sum / mean in its epilogue
                ol.append(ops.ResUnitOp(x=x, w1=cv["w1"], b1=cv["b1"], w2=cv["w2"], b2=cv["b2"], out=dst, n_batch=B,
                                        T=T, C=C, k=cv["k"], dilation=cv["d"], slope=slope, res2=fin.get("res2"),
                                        post_div=fin.get("post_div", 0.0), lens=lens))
            elif "w2" in cv:
                # the second LeakyReLU (residual_block.py:252) has one consumer: it runs once per element in
                # conv1's epilogue, not once per element per 32-deep step per column tile in conv2's loop (on
                # the fp32 matrix pipe every vector instruction of the loop is taken from the MFMA stream)
                ol.append(conv_op(B, x, C, T, cv["w1"], cv["b1"], xt, C, T, ops.conv_taps(cv["k"], cv["d"]),
                                  pro_act=ops.ACT_LEAKY, pro_slope=slope, post=ops.POST_LEAKY, post_div=slope,
                                  **masked(lens)))
                ol.append(conv_op(B, xt, C, T, cv["w2"], cv["b2"], dst, C, T, ops.conv_taps(cv["k"], 1), **skip))
            else:
                ol.append(conv_op(B, x, C, T, cv["w1"], cv["b1"], dst, C, T, ops.conv_taps(cv["k"], cv["d"]),
                                  pro_act=ops.ACT_LEAKY, pro_slope=slope, **skip))
            x = dst


# The same stages of a causal generator (use_causal_conv: CausalConv1d / CausalConvTranspose1d, vocoder/layers/
# causal_conv.py).  No output row depends on a later input row, so a stage can run chunk by chunk: every conv reads a
# [history | chunk] buffer of its own -- the last H rows of what it read in the chunk before, then this chunk's rows --
# as a VALID conv (taps 0, d, 2d, ...), and writes into the chunk rows of its consumer's buffer.  Zero history is the
# convs' causal zero padding, so ONE op list is the one-shot plan (zero histories, every lead 0, run once) and the
# streaming plan (the histories carried over after every chunk, HistoryArena.carry_ops).
class HistBuf:
    """one [history | chunk] buffer inside a plan's arena: B items of H + T rows of C floats, items `bs` floats apart"""

    __slots__ = ("arena", "off", "B", "H", "T", "C")

    def __init__(self, arena, off, B, H, T, C):
        self.arena, self.off, self.B, self.H, self.T, self.C = arena, off, B, H, T, C

    @property
    def bs(self):
        return (self.H + self.T) * self.C

    def row(self, r):
        """row r of item 0, counted from the first history row, as ops take an address: (tensor, element offset)"""
        return (self.arena, self.off + r * self.C)

    @property
    def chunk(self):
        """the first row of this call"""
        return self.row(self.H)

    def view(self):
        return self.arena[self.off:self.off + self.B * self.bs].view(self.B, self.H + self.T, self.C)


class HistoryArena:
    """every [history | chunk] buffer of a causal plan, in ONE tensor -- so the carry of a stream (the last H rows of
    each buffer move to its front) is a table of copies inside one tensor: srn_multi_copy, one launch per 160 (buffer,
    item) pairs.  add() the buffers by name, allocate() once (zeros: the causal padding), then look them up."""

    def __init__(self, B, dev):
        self.B, self.dev, self._specs, self._bufs, self.t = B, dev, [], {}, None

    def add(self, name, H, T, C):
        assert self.t is None and name not in dict(self._specs)
        self._specs.append((name, (H, T, C)))

    def allocate(self):
        off = 0
        for name, (H, T, C) in self._specs:
            self._bufs[name] = (off, H, T, C)
            off += rup(self.B * (H + T) * C, 4)  # every buffer 16-byte aligned
        self.t = torch.zeros(off, device=self.dev, dtype=torch.float32)
        self._bufs = {n: HistBuf(self.t, o, self.B, H, T, C) for n, (o, H, T, C) in self._bufs.items()}

    def __getitem__(self, name):
        return self._bufs[name]

    def carry_ops(self):
        """the ops that end a chunk: rows [T, T + H) of every item of every buffer move to rows [0, H).  Where every
        buffer has T >= H the two spans never overlap and the copies run in place; a chunk shorter than some history
        goes through a scratch tensor of the spans (twice the launches), since a copy may not read what another
        workgroup of the same launch writes."""
        spans = []  # (source view, offset of its destination in the arena)
        for hb in self._bufs.values():
            if hb.H:
                v = hb.view()
                spans += [(v[b, hb.T:], hb.off + b * hb.bs) for b in range(self.B)]
        if not spans:
            return []
        if all(hb.T >= hb.H for hb in self._bufs.values()):
            return [ops.MultiCopyOp([v for v, _ in spans], [o for _, o in spans], self.t)]
        at = [0]
        for v, _ in spans:
            at.append(at[-1] + v.numel())
        scratch = torch.zeros(at[-1], device=self.dev, dtype=torch.float32)
        return [ops.MultiCopyOp([v for v, _ in spans], at[:-1], scratch),
                ops.MultiCopyOp([scratch[a:b] for a, b in zip(at[:-1], at[1:])], [o for _, o in spans], self.t)]

    def carry_ragged_ops(self, n, frames):
        """carry_ops with the pushed counts as device data (srn_history_carry_ragged): for item b of every buffer, rows
        [0, H) are zeroed where n[b] < 0, kept where n[b] == 0, and take rows [n[b] scale, n[b] scale + H) where n[b] > 0
        -- scale = T / frames the buffer's rows per input frame, `frames` the plan's chunk length.  n: (B,) int32 device
        tensor, read when the ops run.  One launch per 96 buffers, no scratch: the kernel owns the overlap."""
        assert all(hb.T % frames == 0 for hb in self._bufs.values())
        table = [(hb.off, hb.bs, hb.H, hb.T, hb.C, hb.T // frames) for hb in self._bufs.values() if hb.H]
        return ops.history_carry_ragged_ops(self.t, table, n, self.B) if table else []


def causal_unit_history(cv, C):
    """rows of history in front of the input of causal unit `cv` of a C-channel stage: the fused unit recomputes its
    intermediate from (k - 1)(d + 1) rows of x; the unfused one keeps the intermediate's k - 1 rows in a buffer of
    their own and needs the first conv's (k - 1) d only"""
    return (cv["k"] - 1) * (cv["d"] + 1) if fused_unit(cv, C) else (cv["k"] - 1) * cv["d"]


def causal_stage_buffers(arena, i, blocks, C, T, H_next):
    """the buffers of causal stage i: `u{i}` the up-sampled input, which every block reads (the longest history any of
    them needs), `x{i}.{j}.{idx}` the input of unit idx >= 1 of block j, `t{i}.{j}.{idx}` the middle of an unfused
    two-conv unit, `acc{i}` the stage's mean with the H_next rows its consumer reaches back"""
    arena.add(f"u{i}", max(causal_unit_history(convs[0], C) for convs in blocks), T, C)
    for j, convs in enumerate(blocks):
        for idx, cv in enumerate(convs):
            if idx:
                arena.add(f"x{i}.{j}.{idx}", causal_unit_history(cv, C), T, C)
            if "w2" in cv and not fused_unit(cv, C):
                arena.add(f"t{i}.{j}.{idx}", cv["k"] - 1, T, C)
    arena.add(f"acc{i}", H_next, T, C)


def causal_upsample_ops(ol, B, src, up, out, slope, lead):
    """CausalConvTranspose1d(k = 2 s, stride s), LeakyReLU in front (causal_conv.py:44-77): `src` a HistBuf with ONE
    history row -- the previous chunk's last row, or, where lead[b] <= 0, a copy of this chunk's first
    (ReplicationPad1d((1, 0)); LeakyReLU commutes with the copy) -- and per output phase one conv of two taps into the
    chunk rows of `out`.  up: the packed entry (phases from ops.convtranspose_phases_causal, b, s, cout)."""
    assert src.H == 1
    s, co = up["s"], up["cout"]
    ol.append(ops.replicate_first_row_op(src.row(0), src.bs, src.C, lead, B))
    for r, (taps, wp) in enumerate(up["phases"]):
        ol.append(conv_op(B, src.row(0), src.C, 1 + src.T, wp, up["b"], out.chunk, co, src.T, taps,
                          pro_act=ops.ACT_LEAKY, pro_slope=slope, out_bs=out.bs, out_t_stride=s, out_t_off=r))


def causal_mrf_stage_ops(ol, B, arena, i, blocks, C, T, slope, lead):
    """mrf_stage_ops for causal stage i over the buffers of causal_stage_buffers: acc{i} = mean over `blocks` of
    block(u{i}).  A unit reads a window of its input buffer that begins as many rows before the chunk as it reaches
    back, and writes the chunk rows of the next unit's buffer: nothing a later chunk needs is overwritten (the dense
    plan's ping-pong buffers would be).  lead: the stage's row of the plan's LeadTable, for the fused units."""
    u, acc = arena[f"u{i}"], arena[f"acc{i}"]
    nb = len(blocks)
    for j, convs in enumerate(blocks):
        x = u
        for idx, cv in enumerate(convs):
            last = idx == len(convs) - 1
            dst = acc if last else arena[f"x{i}.{j}.{idx + 1}"]
            k, d = cv["k"], cv["d"]
            fin = {}
            if last:
                # cs += block(c); c = cs / num_blocks  (hifigan.py:183-186), in the reference's order
                if j > 0:
                    fin.update(res2=acc.chunk, res2_bs=acc.bs, ld_res2=C)
                if j == nb - 1:
                    fin.update(post=ops.POST_DIV, post_div=float(nb))
            H = causal_unit_history(cv, C)
            if fused_unit(cv, C):
                ol.append(ops.ResUnitOp(x=x.row(x.H - H), x_bs=x.bs, w1=cv["w1"], b1=cv["b1"], w2=cv["w2"], b2=cv["b2"],
                                        out=dst.chunk, out_bs=dst.bs, n_batch=B, T=T, C=C, k=k, dilation=d, slope=slope,
                                        res2=fin.get("res2"), res2_bs=acc.bs, post_div=fin.get("post_div", 0.0),
                                        lead=lead))
            else:
                skip = dict(res=x.chunk, res_mode=ops.RES_ADD, res_bs=x.bs, ld_res=C, out_bs=dst.bs, **fin)
                first = dict(in_bs=x.bs, pro_act=ops.ACT_LEAKY, pro_slope=slope)
                if "w2" in cv:
                    xt = arena[f"t{i}.{j}.{idx}"]  # its k - 1 history rows: the intermediate of the chunk before
                    ol.append(conv_op(B, x.row(x.H - H), C, H + T, cv["w1"], cv["b1"], xt.chunk, C, T,
                                      range(0, k * d, d), out_bs=xt.bs, post=ops.POST_LEAKY, post_div=slope, **first))
                    ol.append(conv_op(B, xt.row(0), C, k - 1 + T, cv["w2"], cv["b2"], dst.chunk, C, T, range(k), **skip))
                else:
                    ol.append(conv_op(B, x.row(x.H - H), C, H + T, cv["w1"], cv["b1"], dst.chunk, C, T,
                                      range(0, k * d, d), **first, **skip))
            x = dst


class LeadTable:
    """how far each item of a causal plan has come, at every rate: `scales` as LengthTable's, `lead` ONE (n_rates, B)
    int32 device tensor -- row i holds, per item, the rows of its utterance that lie before the next call at rate i
    (capped: the ops clamp it to their own history) -- `rows` its (B,) rows, which the ops read when they run.
    set_pushed() rewrites the tensor in place, outside the captured graph, whose nodes only carry its address."""

    CAP = 1 << 30

    def __init__(self, upsample_scales, B, dev):
        self.scales, self.B = [1], B
        for s in upsample_scales:
            self.scales.append(self.scales[-1] * s)
        self.lead = torch.zeros(len(self.scales), B, dtype=torch.int32, device=dev)
        self.rows = list(self.lead.unbind(0))

    def set_pushed(self, frames):
        """frames: the input frames every item has been given so far"""
        host = torch.tensor([[min(int(frames) * s, self.CAP)] * self.B for s in self.scales], dtype=torch.int32)
        self.lead.copy_(host)

    def set_pushed_items(self, frames):
        """frames: per item, the input frames it has been given since its utterance began (B values)"""
        frames = [int(f) for f in frames]
        assert len(frames) == self.B
        host = torch.tensor([[min(f * s, self.CAP) for f in frames] for s in self.scales], dtype=torch.int32)
        self.lead.copy_(host)


class LengthTable:
    """the lengths of a ragged generator plan at every rate: `scales` the cumulative up-sampling factors (1 for the
    input frames, then one per stage), `lens` ONE (n_rates, B) int32 device tensor, `rows` its (B,) rows, which the ops
    read when they run.  set_lengths() rewrites the tensor in place -- outside the captured graph, whose nodes only
    carry its address."""

    def __init__(self, upsample_scales, B, dev):
        self.scales = [1]
        for s in upsample_scales:
            self.scales.append(self.scales[-1] * s)
        self.lens = torch.zeros(len(self.scales), B, dtype=torch.int32, device=dev)
        self.rows = list(self.lens.unbind(0))

    def set_lengths(self, lengths):
        """lengths: B frame counts in [1, T_cap] (validated by the caller, item_lengths)"""
        host = torch.tensor([[int(n) * s for n in lengths] for s in self.scales], dtype=torch.int32)
        self.lens.copy_(host)


class StridedLengthTable:
    """the heights of a ragged batch through a stack of `n_layers` stride-2 convs (k3, p1: H -> (H - 1) // 2 + 1), kept
    the way LengthTable keeps a generator's: `lens` ONE (n_layers + 1, B) int32 device tensor, row 0 the items' own
    row counts, `rows` its (B,) rows, which the ops read when they run.  set_lengths() rewrites the tensor in place --
    outside the captured graph, whose nodes only carry its address."""

    def __init__(self, n_layers, B, dev):
        self.n_layers, self.B = n_layers, B
        self.lens = torch.zeros(n_layers + 1, B, dtype=torch.int32, device=dev)
        self.rows = list(self.lens.unbind(0))

    def set_lengths(self, lengths):
        """lengths: B row counts in [1, T_cap] (validated by the caller, item_lengths)"""
        table = [[int(n) for n in lengths]]
        assert len(table[0]) == self.B
        for _ in range(self.n_layers):
            table.append([(h - 1) // 2 + 1 for h in table[-1]])
        self.lens.copy_(torch.tensor(table, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- self-attention
S_BUDGET = 320 << 20  # bytes of attention scores in flight (one chunk); see attention_scores


def attention_chunks(B, H, pair_bytes, budget_bytes):
    """[(b0, n_batch, h0, n_head)] covering all (batch, head) pairs in order, each chunk's scores within the budget
    (a single pair is always admitted): runs of whole batch items when one item's H pairs fit, else runs of heads
    inside one batch item."""
    fit = max(1, budget_bytes // max(pair_bytes, 1))
    if fit >= H:
        n = -(-B // (fit // H))  # number of chunks, then even them out
        step = -(-B // n)
        return [(b0, min(step, B - b0), 0, H) for b0 in range(0, B, step)]
    return [(b, 1, h0, min(fit, H - h0)) for b in range(B) for h0 in range(0, H, fit)]


def attention_scores(B, H, T, device):
    """The bounded score buffer of attention_ops for sequences up to T rows.
    Attention scores are produced and consumed in CHUNKS of (batch, head) pairs through this one buffer:
    [Q K^T -> softmax -> P V] per chunk, so S is never materialised whole -- the footprint is S_BUDGET instead of
    B * H * T^2 * 4 B (50 GiB at B=32 x T=4096 before) -- and a chunk stays inside the 256 MiB Infinity Cache
    between its three kernels.  A chunk is a run of whole batch items, or a run of heads of one batch item.
    Not zeroed: Q K^T writes every column below T of a row and srn_softmax_rows rewrites all ld columns of it, masking
    by column < len before it looks at a value."""
    per_pair = T * rup(T, 32) * 4
    return torch.empty(max(1, min(B * H, S_BUDGET // per_pair)) * T * rup(T, 32), device=device, dtype=torch.float32)


def attention_ops(qkv, Vt, S, out, lens, B, H, hd, T, precision):
    """S = Q K^T / sqrt(d) -> softmax over keys < len -> O = P V, chunk by chunk through S (attention_scores).
    qkv (B, T, 3 H hd): q | k row-major, as the QKV projection leaves them; Vt (B, H hd, rup(T, 32)): V^T, which that
    projection's transposed tail wrote (P V then contracts k-major rows like every other GEMM; its pad columns must be
    zero, they meet exact zeros of the softmax); out (B, T, H hd); lens (B,) int32 valid keys per item, or None.
    The training step's attention node runs the same three ops with S holding all B * H pairs (one chunk)."""
    inner = H * hd
    Tp = rup(T, 32)
    ol = []
    for b0, nb, h0, nh in attention_chunks(B, H, T * Tp * 4, S.numel() * 4):
        q_off = b0 * T * 3 * inner + h0 * hd
        ol.append(ConvOp(in0=(qkv, q_off), w=(qkv, q_off + inner), out=S, n_batch=nb, n_head=nh, T_in=T,
                         T_out=T, C_in=hd, N=T, in0_bs=T * 3 * inner, in0_hs=hd, ld_in0=3 * inner,
                         w_bs=T * 3 * inner, w_hs=hd, ldw=3 * inner, out_bs=nh * T * Tp, out_hs=T * Tp,
                         ld_out=Tp, alpha=1.0 / math.sqrt(hd), precision=precision))
        ol.append(ops.softmax_rows_op(S, lens if lens is None else (lens, b0), nb * nh, nh, T, Tp))
        ol.append(ConvOp(in0=S, w=(Vt, b0 * inner * Tp + h0 * hd * Tp), out=(out, b0 * T * inner + h0 * hd),
                         n_batch=nb, n_head=nh, T_in=T, T_out=T, C_in=Tp, N=hd, in0_bs=nh * T * Tp,
                         in0_hs=T * Tp, ld_in0=Tp, w_bs=inner * Tp, w_hs=hd * Tp, ldw=Tp, out_bs=T * inner,
                         out_hs=hd, ld_out=inner, precision=precision))
    return ol


# ---------------------------------------------------------------------------------------------- front-end plumbing
def item_lengths(lengths, B, N, what):
    """the per-item sample counts of a (B, N) batch as a tuple of ints: `lengths` (tensor, numpy or sequence), or N for
    every item when it is None.  ValueError unless there are B values in [1, N]."""
    if lengths is None:
        return (N,) * B
    lens = tuple(int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths))
    if len(lens) != B or min(lens) < 1 or max(lens) > N:
        raise ValueError(f"{what}: lengths {lens} must give {B} sample counts in [1, {N}]")
    return lens


def wave_batch(wave, lengths, device, what, allow_channel_dim=False):
    """(n,) or (B, n) waveform(s) -- (B, 1, n) too with allow_channel_dim -- as a tensor or numpy, and optional
    per-item sample counts -> ((B, n) fp32 tensor on the GPU, [int lengths]).  A CPU input is uploaded to `device`."""
    if not isinstance(wave, torch.Tensor):
        wave = torch.as_tensor(np.asarray(wave, dtype=np.float32))
    a = wave.detach()
    shapes = "(n,), (B, n) or (B, 1, n)" if allow_channel_dim else "(n,) or (B, n)"
    if allow_channel_dim and a.dim() == 3:
        if a.shape[1] != 1:
            raise ValueError(f"{what}: a 3-D wave must be (B, 1, n)")
        a = a[:, 0]
    if a.dim() == 1:
        a = a.unsqueeze(0)
    if a.dim() != 2:
        raise ValueError(f"{what}: wave16k must be {shapes}")
    if not a.is_cuda:
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{what} needs a CUDA (ROCm) device; there is no CPU fallback")
        a = a.to(device)
    a = a.to(torch.float32)
    return a, list(item_lengths(lengths, *a.shape, what))


def check_state(what, state, want, ignored=()):
    """`state` must hold exactly the keys of `want` ({key: shape}) with those shapes, plus any of `ignored`"""
    missing = [k for k in want if k not in state]
    unexpected = sorted(set(state) - set(want) - set(ignored))
    if missing or unexpected:
        raise KeyError(f"{what}: missing {missing[:8]}, unexpected {unexpected[:8]}")
    for k, shp in want.items():
        if tuple(state[k].shape) != shp:
            raise ValueError(f"{what}: {k} has shape {tuple(state[k].shape)}, expected {shp}")
