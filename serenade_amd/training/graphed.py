"""The whole training step captured as a hipGraph."""
import torch


def count_memset_nodes(graph):
    """number of memset nodes in a captured `torch.cuda.CUDAGraph(keep_graph=True)` (hipGraphGetNodes /
    hipGraphNodeGetType on its raw handle).

    Why it matters (profiles/r3_graph_probe.json, tools/experiments/graph_probe.py): on this stack (ROCm 7.2, torch
    2.10+rocm7.0) a hipMemsetAsync captured into a hipGraph fills with the right value on the FIRST replay and with
    garbage from the second replay on, for every size and value tried.  torch's multi-block reductions zero their
    semaphore buffer with exactly that call, so a captured `x.sum()` / `x.norm()` / `x.sum(0)` elects no last block
    and returns stale numbers from replay 2 on (forty reductions in one capture: error 0 on replay 1, 3e17 after).
    Kernels are unaffected.  Anything captured here must therefore hold no memset node."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (ctypes.c_void_p * max(1, n.value))()
    if hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    memsets = 0
    for i in range(n.value):
        kind = ctypes.c_int(-1)
        if hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(kind)) != 0:
            raise RuntimeError("hipGraphNodeGetType failed")
        memsets += kind.value == 2  # hipGraphNodeTypeMemset
    return memsets, n.value


class GraphedStep:
    """One whole-model training step of a fixed (B, L) captured as a hipGraph and replayed.

    At the reference's per-GPU batch (4) the eager step is bound by its ~2500 host-side launches; captured, the same
    kernels run back to back.  Everything step-dependent lives in device memory: the inputs (static buffers the call
    copies into), the infill segment (drawn on the host like the reference, uploaded as two integers), t / z / dropout
    (the device generator, graph-safe), the clip factor and Adam's bias corrections (`AdamW.step_captured`).
    With more than one rank the gradient all-reduce runs between two captured halves (backward | optimizer) on the whole
    flat buffer.  Training batches of varying length need one GraphedStep per length bucket."""

    def __init__(self, model, opt, B, L, in_dim=768, sync=None, warmup=2, tz=None):
        """tz (tests): (t (B,1,1), z (B,out,L)) device tensors used instead of the generator's draws"""
        dev = model.device
        self.model, self.opt, self.sync, self.tz = model, opt, sync, tz
        self.split = sync is not None and (sync.world > 1 or sync.always)
        if self.split and sync._hooks:
            raise ValueError("GraphedStep needs GradSync(..., overlap=False): collectives cannot sit inside the capture")
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.x, self.logmel, self.midi, self.lft = f(B, L, in_dim), f(B, L, model.output_dim), f(B, L, 1), f(B, L, 1)
        self.lens = torch.full((B,), L, device=dev, dtype=torch.int64)
        self.seg = torch.tensor([0, max(1, L // 4)], device=dev, dtype=torch.int64)
        self.L = L
        # warm-up runs real steps (on the zero-filled static inputs): put weights, optimizer state and BatchNorm
        # statistics back afterwards, so constructing a GraphedStep leaves the training state untouched
        keep = (model.flat.clone(), opt.m.clone(), opt.v.clone(), opt.steps, {k: v.clone() for k, v in model.buffers.items()})
        if warmup < 1:
            raise ValueError("GraphedStep needs at least one warm-up step: workspaces, library handles and the autograd "
                             "graph's accumulators must exist before the capture")
        # kept for the lifetime of the graphs: ops.tn_workspace / splitk_workspace key their slabs by the stream's
        # handle, and torch hands a released handle out again
        side = self._side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # library handles, workspaces and autotuning settle outside the capture
            for _ in range(warmup):
                self._fwd_bwd()
                opt.prepare()
                opt.step_captured()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.g1, self.g2 = torch.cuda.CUDAGraph(keep_graph=True), None
        # captured on the warm-up's stream: the leaves' gradient accumulators were created there (the estimator keeps
        # re-laid weights that hold them), and autograd warns -- and synchronises -- when a later backward feeds them
        # from another stream
        if self.split:
            with torch.cuda.graph(self.g1, stream=side):
                self._fwd_bwd()
            self.g2 = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(self.g2, pool=self.g1.pool(), stream=side):
                opt.step_captured()
        else:
            with torch.cuda.graph(self.g1, stream=side):
                self._fwd_bwd()
                opt.step_captured()
        # a captured memset replays with a corrupted fill value on this stack (count_memset_nodes): a torch reduction
        # that goes multi-block at this (B, L), or a library call that clears a flag buffer, would train on stale sums
        # from the second step on -- refuse the bucket instead
        self.nodes = 0
        for g in (self.g1, self.g2):
            if g is not None:
                memsets, total = count_memset_nodes(g)
                self.nodes += total
                if memsets:
                    raise RuntimeError(f"the captured step for B={B}, L={L} holds {memsets} memset node(s) of {total}: "
                                       "hipGraph memset nodes replay wrongly on this ROCm stack (see "
                                       "training.count_memset_nodes); run this bucket eagerly")
        model.flat.copy_(keep[0]), opt.m.copy_(keep[1]), opt.v.copy_(keep[2])
        opt.steps = keep[3]
        for k, v in keep[4].items():
            model.buffers[k].copy_(v)

    def _fwd_bwd(self):
        draws = {"seg": self.seg}
        if self.tz is not None:
            draws.update(t=self.tz[0], z=self.tz[1])
        ret = self.model(self.x, self.lens, self.logmel, self.midi, self.lft, draws=draws)
        self.cfm, self.prior = ret["cfm_loss"].detach(), ret["prior_loss"].detach()
        self.model.store.backward_into_flat(ret["cfm_loss"] + ret["prior_loss"])

    def __call__(self, x, lengths, logmel, midi, lft, segment=None):
        """returns (cfm_loss, prior_loss, grad_norm) as device tensors of the step just replayed"""
        for dst, src in ((self.x, x), (self.logmel, logmel), (self.midi, midi), (self.lft, lft), (self.lens, lengths)):
            dst.copy_(src, non_blocking=True)
        s0, n = self.model.draw_segment(self.L) if segment is None else segment
        self.seg.copy_(torch.tensor([s0, n], dtype=torch.int64))
        self.opt.prepare()
        self.g1.replay()
        if self.split:
            for a, b in self.sync.buckets:
                self.sync.dist.all_reduce(self.model.flat_grad[a:b], group=self.sync.group)
            if self.sync.world > 1:
                self.model.flat_grad.div_(self.sync.world)
            self.g2.replay()
        return self.cfm, self.prior, self.opt.norm
