"""Around the gradients: the all-reduce that replaces DDP, clip + AdamW over the flat buffers, the learning-rate
schedule and the reference's checkpoint format."""
import torch

from ..ops import call as _call
from .. import training as _root  # _root._require_cuda: the guard, bound once at the package root
from ..plan import rup


class GradSync:
    """All-reduce (mean) of `estimator.flat_grad` across the ranks, in buckets of ~`bucket_bytes`.

    The reference wraps the model in DistributedDataParallel over NCCL (bin/ssc_train.py:353-358).  Here the flat
    gradient buffer is cut into contiguous buckets; the parameters are laid out in forward order, so backward
    completes the buckets from the last to the first, and a post-accumulate hook on every parameter launches its
    bucket's asynchronous all-reduce the moment the bucket's last gradient has landed -- the RCCL transfers of the
    late layers overlap the backward GEMMs of the early ones.  xGMI rings are per-link bound, so buckets are large
    (default 64 MiB: 3 collectives for the 44 M-parameter estimator).  `finish()` waits and divides by the world size.
    World size 1 (or no process group) makes every call a no-op unless `always` (single-GPU rehearsal of the RCCL path)."""

    def __init__(self, estimator, bucket_bytes=64 << 20, group=None, always=False, overlap=True):
        import torch.distributed as dist
        self.dist = dist
        self.est = estimator
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.always = bool(always) and dist.is_available() and dist.is_initialized()  # collectives even with one rank
        self.launched = 0  # collectives issued so far (tests / logs)
        per = max(1, bucket_bytes // 4)
        total = estimator.flat.numel()
        self.buckets = []  # (start, end)
        lo = 0
        names = list(estimator.spans)
        for k in names:
            off, n = estimator.spans[k]
            end = off + rup(n, 4)
            if end - lo >= per or k == names[-1]:
                self.buckets.append((lo, total if k == names[-1] else end))
                lo = end
        self.bucket_of = {}
        self.count = [0] * len(self.buckets)
        for k in names:
            off, _ = estimator.spans[k]
            bi = next(i for i, (s, e) in enumerate(self.buckets) if s <= off < e)
            self.bucket_of[k] = bi
            self.count[bi] += 1
        self._left = list(self.count)
        self._work = []
        self._hooks = []
        if (self.world > 1 or self.always) and overlap:  # overlap=False: everything is launched by finish()
            for k, p in estimator.params.items():
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(self.bucket_of[k])))

    def _make_hook(self, bi):
        def hook(_):
            self._left[bi] -= 1
            if self._left[bi] == 0:
                self._launch(bi)
        return hook

    def _launch(self, bi):
        s, e = self.buckets[bi]
        self.launched += 1
        self._work.append(self.dist.all_reduce(self.est.flat_grad[s:e], op=self.dist.ReduceOp.SUM, group=self.group,
                                               async_op=True))

    def finish(self):
        """call after backward(): launches whatever the hooks did not (unused parameters), waits, averages"""
        if self.world == 1 and not self.always:
            return
        for bi, left in enumerate(self._left):
            if left > 0:
                self._launch(bi)
        for w in self._work:
            w.wait()
        self._work = []
        self._left = list(self.count)
        if self.world > 1:
            self.est.flat_grad.div_(self.world)


class AdamW:
    """clip_grad_norm_(max_norm) + torch.optim.AdamW (trainers/ssc.py:90-95; conf/serenade.yaml:62-65: lr 8e-4,
    grad_norm 1.0, torch defaults betas (0.9, 0.999), eps 1e-8, weight_decay 0.01) as ONE kernel over the flat buffers."""

    def __init__(self, estimator, lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0):
        self.est = estimator
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.m = torch.zeros_like(estimator.flat)
        self.v = torch.zeros_like(estimator.flat)
        self.steps = 0
        self.dyn = torch.zeros(4, device=estimator.flat.device, dtype=torch.float32)  # lr, bc1, bc2, grad_scale
        self._ss = torch.zeros(1024, device=estimator.flat.device, dtype=torch.float64)  # srn_sumsq partial sums
        self.norm = torch.zeros((), device=estimator.flat.device, dtype=torch.float64)  # last gradient norm (device)

    def _grad_norm(self):
        """fp64 total gradient norm as a 0-dim device tensor (own kernel + a 1024-element sum: torch's multi-block
        reductions gave wrong results when replayed inside a hipGraph on this stack)"""
        g = self.est.flat_grad
        _call("srn_sumsq", g, g.numel(), self._ss)
        return torch.sqrt(self._ss.sum())

    def prepare(self):
        """host side of `step_captured`: advance the step count and upload {lr, 1 - beta1^t, 1 - beta2^t} (call before
        every replay of a graph that contains `step_captured`)"""
        self.steps += 1
        h = torch.tensor([self.lr, 1.0 - self.betas[0] ** self.steps, 1.0 - self.betas[1] ** self.steps],
                         dtype=torch.float32)
        self.dyn[:3].copy_(h)

    def step_captured(self):
        """the same update with no host synchronisation (gradient norm, clip factor and bias corrections stay on the
        device): identical launches every step, so it can sit inside a captured hipGraph.  `prepare()` first."""
        g = self.est.flat_grad
        with torch.no_grad():
            norm = self._grad_norm()
            self.norm.copy_(norm)
            if self.max_norm and self.max_norm > 0:
                self.dyn[3:4] = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0).to(torch.float32)
            else:
                self.dyn[3:4] = 1.0
            _call("srn_adamw_dyn", self.est.flat, g, self.m, self.v, g.numel(), self.betas[0], self.betas[1], self.eps,
                  self.wd, self.dyn)

    def step(self):
        """returns the gradient norm before clipping (what clip_grad_norm_ returns)"""
        _root._require_cuda(self.est.flat, "AdamW.step")
        g = self.est.flat_grad
        norm = float(self._grad_norm())
        scale = 1.0
        if self.max_norm and self.max_norm > 0:
            scale = min(1.0, self.max_norm / (norm + 1e-6))
        self.steps += 1
        with torch.no_grad():
            _call("srn_adamw", self.est.flat, g, self.m, self.v, g.numel(), self.lr, self.betas[0], self.betas[1],
                  self.eps, self.wd, self.steps, scale)
        return norm


class MultiStepLR:
    """torch.optim.lr_scheduler.MultiStepLR for `AdamW` above (conf/serenade.yaml:66-70: gamma 0.5 at step 100 000):
    call step() once per optimizer step, as trainers/ssc.py:96 does."""

    def __init__(self, opt, milestones, gamma=0.5):
        self.opt, self.milestones, self.gamma = opt, sorted(int(m) for m in milestones), float(gamma)
        self.base_lr, self.last_epoch = opt.lr, 0

    def step(self):
        self.last_epoch += 1
        self.opt.lr = self.base_lr * self.gamma ** sum(1 for m in self.milestones if m <= self.last_epoch)

    def state_dict(self):
        """the entries of torch.optim.lr_scheduler.MultiStepLR.state_dict()"""
        from collections import Counter
        return {"milestones": Counter(self.milestones), "gamma": self.gamma, "base_lrs": [self.base_lr],
                "last_epoch": self.last_epoch, "_step_count": self.last_epoch + 1,
                "_get_lr_called_within_step": False, "_last_lr": [self.opt.lr]}

    def load_state_dict(self, sd):
        ms = sd["milestones"]
        self.milestones = sorted(int(m) for m in (ms.elements() if hasattr(ms, "elements") else ms))
        self.gamma, self.last_epoch = float(sd["gamma"]), int(sd["last_epoch"])
        self.base_lr = float(sd["base_lrs"][0] if "base_lrs" in sd else sd["base_lr"])
        self.opt.lr = self.base_lr * self.gamma ** sum(1 for m in self.milestones if m <= self.last_epoch)


def _torch_adamw_state(model, opt):
    """this optimizer's flat moments as `torch.optim.AdamW.state_dict()` of the reference's optimizer: parameters are
    numbered in `model.parameters()` order, which is the order of the parameter entries of the state_dict the store
    was built from (bin/ssc_train.py:331-343 builds AdamW over model.parameters())."""
    state, ids = {}, []
    for i, (k, (off, n)) in enumerate(model.spans.items()):
        shape = model.params[k].shape
        ids.append(i)
        if opt.steps > 0:
            state[i] = {"step": torch.tensor(float(opt.steps)), "exp_avg": opt.m[off:off + n].view(shape).cpu().clone(),
                        "exp_avg_sq": opt.v[off:off + n].view(shape).cpu().clone()}
    group = {"lr": opt.lr, "betas": tuple(opt.betas), "eps": opt.eps, "weight_decay": opt.wd, "amsgrad": False,
             "foreach": None, "maximize": False, "capturable": False, "differentiable": False, "fused": None,
             "params": ids}
    return {"state": state, "param_groups": [group]}


def _load_torch_adamw_state(o, model, opt):
    names = list(model.spans)
    groups = o["param_groups"]
    ids = [i for g in groups for i in g["params"]]
    if len(ids) != len(names):
        raise ValueError(f"optimizer state holds {len(ids)} parameters, this model has {len(names)}")
    opt.m.zero_(), opt.v.zero_()
    steps = 0
    for pos, i in enumerate(ids):
        st = o["state"].get(i)
        if st is None:
            continue
        off, n = model.spans[names[pos]]
        if st["exp_avg"].numel() != n:
            raise ValueError(f"optimizer state {i} has {st['exp_avg'].numel()} elements, {names[pos]} has {n}")
        opt.m[off:off + n].copy_(st["exp_avg"].reshape(-1))
        opt.v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
        steps = max(steps, int(float(st["step"])))
    opt.steps, opt.lr = steps, float(groups[0]["lr"])


def save_checkpoint(path, model, opt, scheduler=None, steps=0, epochs=0):
    """the reference's checkpoint file (trainers/base.py:91-111): {"model", "optimizer", "scheduler", "steps",
    "epochs"} with "optimizer" / "scheduler" in the layout of `torch.optim.AdamW.state_dict()` /
    `MultiStepLR.state_dict()`, so the reference's trainer resumes from it and vice versa."""
    import os
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"model": {k: v.cpu() for k, v in model.state_dict().items()},
                "optimizer": _torch_adamw_state(model, opt),
                "scheduler": None if scheduler is None else scheduler.state_dict(), "steps": int(steps),
                "epochs": int(epochs)}, path)


def load_checkpoint(path, model, opt=None, scheduler=None, load_only_params=False):
    """trainers/base.py:113-130: restores the weights (and BatchNorm statistics) in place; with an optimizer also its
    moments, step count and learning rate -- from a checkpoint of this package or of the reference's trainer (torch's
    AdamW / MultiStepLR state_dicts).  Returns (steps, epochs)."""
    ck = torch.load(path, map_location="cpu")
    with torch.no_grad():
        for k, v in ck["model"].items():
            if k in model.params:
                model.params[k].copy_(v)
            elif k in getattr(model, "buffers", {}):
                model.buffers[k].copy_(v)
            else:
                raise KeyError(f"checkpoint tensor {k} is not a tensor of this model")
    if load_only_params or opt is None:
        return int(ck.get("steps", 0)), int(ck.get("epochs", 0))
    o = ck["optimizer"]
    if "param_groups" in o and "state" in o:
        with torch.no_grad():
            _load_torch_adamw_state(o, model, opt)
    elif "spans" in o:  # files written by round 2 of this package: flat moment buffers + their layout
        if dict(o["spans"]) != dict(model.spans):
            raise ValueError("optimizer state was saved for a different parameter layout")
        opt.m.copy_(o["m"]), opt.v.copy_(o["v"])
        opt.steps, opt.lr = int(o["steps"]), float(o["lr"])
    else:
        raise ValueError(f"unrecognised optimizer entry (keys {sorted(o)}): expected torch.optim.AdamW.state_dict()")
    if scheduler is not None and ck.get("scheduler") is not None:
        scheduler.load_state_dict(ck["scheduler"])
    return int(ck["steps"]), int(ck["epochs"])
