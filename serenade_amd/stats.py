"""Stage 2 of the recipe and the batch the training step eats, on the GPU: the feature scalers of
serenade/bin/compute_statistics.py:121-144 and FeatsDataset's normalisation (audio_mel_dataset.py:96-110) followed by
SSCCollater (collaters/ssc.py:50-77).

    moments(items, check=True) -> Moments(n, sum, m2, min, max, nonfinite)      per-item numpy arrays
    StandardScaler / MinMaxScaler     .partial_fit(items) .merge(other) .transform(items) .to_sklearn()
    fit_statistics(dumps, score_type="est_lf0_score", logmel_type="logmel", batch=8)
                                      -> {"hubert", "logmel", "score", "loud"}
    save_statistics(scalers, path)                                              joblib.dump: stats.joblib
    Collater(scaler, max_frames=3000, device=None)(dumps) -> {"xs", "lens", "ys", "louds", "scores"}

An item is one utterance's track: (T, C) float32, T >= 1, a numpy array or a tensor on the host or the device.  Items
are PACKED -- their rows one after another in one (R, C) buffer, with the row offsets next to it -- so host items are
uploaded once, nothing is padded and nothing outside an item is read.  There is no CPU path.

Two HIP entry points (serenade_amd/csrc/stats.hip), defined in DESIGN.md 7f:

    srn_col_moments   per item b and column c, n = the item's rows:  sum = sum_r x,  T = sum / n,  d = (double)x - T,
                      m2 = sum_r d^2 - (sum_r d)^2 / n   (sklearn.utils.extmath._incremental_mean_and_var for one
                      batch), min, max (float32), and per item the count of NaN / +-inf.  Every sum is fp64 in an order
                      that depends on n alone, so a list of items gives bit for bit what its items give one at a time.
    srn_scale_collate out[b, t, c] = (x[item order[b]][t, c] - sub[c]) / div[c], +0.0 from the item's end to Tmax.
                      wide: sub / div float64, both operations fp64, one rounding to float32 -- numpy's
                      float32 - float64, / float64 and the collater's .float(); not wide: everything float32 -- numpy's
                      float32 track against MinMaxScaler's float32 data_min_ / span.  Bit for bit numpy.

The scalers fold the per-item results on the host in float64, in item order, by sklearn 1.7's own update formula and
its constant-feature rule, and carry sklearn's attribute names and dtypes for float32 input.

Where this differs from sklearn: an item holding NaN or +-inf is a ValueError naming the item (sklearn would skip NaNs
per column; a dump with NaNs is a broken dump).  transform is FeatsDataset's expression, (x - mean_) / scale_ and
(x - data_min_) / (data_max_ - data_min_) with one rounding, not sklearn's in-place x -= mean_; x /= scale_ and
x * scale_ + min_, which round twice.
"""
import collections

import numpy as np
import torch

from . import ops

__all__ = ["moments", "Moments", "StandardScaler", "MinMaxScaler", "fit_statistics", "save_statistics", "Collater",
           "scale_collate"]

Moments = collections.namedtuple("Moments", "n sum m2 min max nonfinite")
# compute_statistics.py:122-126
ENTRIES = {"hubert": "standard", "logmel": "standard", "score": "minmax", "loud": "minmax"}


# ---------------------------------------------------------------------------------------------------- packing
def _item_list(items):
    if isinstance(items, (list, tuple)):
        return list(items)
    return [items]


def _check_items(items, what):
    """the argument errors of a list of items, before anything touches the device -> (lengths, C)"""
    if not items:
        raise ValueError(f"{what}: no item")
    lens, C = [], None
    for b, v in enumerate(items):
        if not isinstance(v, (torch.Tensor, np.ndarray)):
            raise ValueError(f"{what}: item {b} must be a numpy array or a tensor, got {type(v).__name__}")
        if v.dtype not in (torch.float32, np.float32):
            raise ValueError(f"{what}: item {b} must be float32, got {v.dtype}")
        if len(v.shape) != 2 or v.shape[0] < 1 or v.shape[1] < 1:
            raise ValueError(f"{what}: item {b} must be (T, C) and not empty, got shape {tuple(v.shape)}")
        if C is None:
            C = int(v.shape[1])
        elif int(v.shape[1]) != C:
            raise ValueError(f"{what}: item {b} has {v.shape[1]} columns, item 0 has {C}")
        lens.append(int(v.shape[0]))
    return lens, C


def _device(items, device=None):
    if not torch.cuda.is_available():
        raise RuntimeError("serenade_amd.stats needs a CUDA (ROCm) device; there is no CPU fallback")
    if device is not None:
        return torch.device(device)
    return next((v.device for v in items if isinstance(v, torch.Tensor) and v.is_cuda),
                torch.device("cuda", torch.cuda.current_device()))


class _Packed:
    """the rows of all items one after another on the device, and where each item begins"""

    def __init__(self, items, what, device=None):
        self.lens, self.C = _check_items(items, what)
        dev = _device(items, device)
        if all(isinstance(v, np.ndarray) for v in items):  # packed on the host, uploaded once
            self.x = torch.from_numpy(np.concatenate([np.ascontiguousarray(v) for v in items], axis=0)).to(dev)
        else:
            parts = [torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()
                     for v in items]
            self.x = torch.cat([p.to(dev) for p in parts], dim=0).contiguous()
        self.B, self.R = len(self.lens), int(self.x.shape[0])
        self.row_off = torch.tensor(np.concatenate([[0], np.cumsum(self.lens)]), dtype=torch.int64, device=dev)


# ---------------------------------------------------------------------------------------------------- moments
@torch.no_grad()
def moments(items, check=True):
    """what one partial_fit needs of every item: Moments(n (B,) int64, sum (B, C) float64, m2 (B, C) float64,
    min (B, C) float32, max (B, C) float32, nonfinite (B,) int32) as numpy arrays, one launch for the whole list.
    ValueError before the device is touched for an empty list, an empty item, mixed column counts or a dtype other
    than float32; with `check`, ValueError after the launch naming the first item that holds NaN or +-inf (sklearn
    would skip NaNs per column; a dump with NaNs is a broken dump)."""
    p = _Packed(_item_list(items), "moments")
    dev, B, C = p.x.device, p.B, p.C
    f64 = torch.empty(2, B, C, dtype=torch.float64, device=dev)
    f32 = torch.empty(2, B, C, dtype=torch.float32, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    ops.CallOp("srn_col_moments", (p.x, p.row_off, p.R, f64[0], f64[1], f32[0], f32[1], bad, B, C))()
    f64, f32, bad = f64.cpu().numpy(), f32.cpu().numpy(), bad.cpu().numpy()
    if check and bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"moments: item {b} holds {int(bad[b])} NaN or infinite values: a broken dump")
    return Moments(np.asarray(p.lens, dtype=np.int64), f64[0], f64[1], f32[0], f32[1], bad)


# ---------------------------------------------------------------------------------------------------- collate
@torch.no_grad()
def scale_collate(items, sub, div, order=None, device=None, out=None):
    """(Bout, Tmax, C) float32 on the device: item order[b] of `items` as (x - sub) / div, zeros from its end to
    Tmax = the longest chosen item.  sub / div: (C,) numpy, both float64 (the arithmetic is float64, rounded once) or
    both float32 (the arithmetic is float32), as numpy's own result type would have it.  order: which items, in which
    order (default: all, as given).  out: a contiguous float32 device tensor of that shape to write into; every
    element of it is written."""
    what = "scale_collate"
    items = _item_list(items)
    lens, C = _check_items(items, what)
    order = list(range(len(items))) if order is None else [int(i) for i in order]
    if not order or min(order) < 0 or max(order) >= len(items):
        raise ValueError(f"{what}: order {order} must pick at least one of the {len(items)} items")
    sub, div = np.asarray(sub), np.asarray(div)
    if sub.dtype != div.dtype or sub.dtype not in (np.float32, np.float64):
        raise ValueError(f"{what}: sub and div must both be float32 or both float64, got {sub.dtype} and {div.dtype}")
    if sub.shape != (C,) or div.shape != (C,):
        raise ValueError(f"{what}: sub and div must be ({C},), got {sub.shape} and {div.shape}")
    p = _Packed(items, what, device)
    dev = p.x.device
    Tmax = max(lens[i] for i in order)
    d_order = torch.tensor(order, dtype=torch.int32, device=dev)
    d_sub, d_div = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (sub, div))
    if out is None:
        out = torch.empty(len(order), Tmax, C, dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (len(order), Tmax, C) or out.dtype != torch.float32 or out.device != dev
          or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous float32 {(len(order), Tmax, C)} tensor on {dev}")
    ops.CallOp("srn_scale_collate", (p.x, p.row_off, p.R, d_order, d_sub, d_div, int(sub.dtype == np.float64), out,
                                     Tmax, p.B, len(order), C))()
    return out


def _operands(kind, entry):
    """(sub, div) of FeatsDataset's expression for one scaler entry (datasets._scale), in numpy's result type against
    a float32 track"""
    if kind == "standard":
        sub, div = np.asarray(entry.mean_), np.asarray(entry.scale_)
    else:
        sub = np.asarray(entry.data_min_)
        div = np.asarray(entry.data_max_) - sub
    dtype = np.float64 if np.result_type(np.float32, sub.dtype, div.dtype) == np.float64 else np.float32
    return np.atleast_1d(sub.astype(dtype)), np.atleast_1d(div.astype(dtype))


# ---------------------------------------------------------------------------------------------------- scalers
def _fold(mean, var, count, new_sum, new_m2, new_count):
    """sklearn.utils.extmath._incremental_mean_and_var's update of (mean, var, count) by one batch given as its
    column sums, its corrected sums of squared deviations and its row count; float64 throughout"""
    last_sum = mean * count
    updated_count = count + new_count
    updated_mean = (last_sum + new_sum) / updated_count
    if count == 0:
        m2 = new_m2
    else:
        ratio = count / new_count
        m2 = var * count + new_m2 + ratio / updated_count * np.square(last_sum / ratio - new_sum)
    return updated_mean, m2 / updated_count, updated_count


class _Scaler:
    kind = None

    def _items(self, items, what):
        items = _item_list(items)
        _, C = _check_items(items, what)
        if hasattr(self, "n_features_in_") and C != self.n_features_in_:
            raise ValueError(f"{what}: items have {C} columns, the scaler was fitted on {self.n_features_in_}")
        return items

    def fit(self, items):
        for name in [k for k in vars(self) if k.endswith("_")]:
            delattr(self, name)
        return self.partial_fit(items)

    def partial_fit(self, items):
        """one item or a list: one launch, then the per-item results folded in item order, so a call on a list is bit
        for bit the same items passed one at a time"""
        return self.fold(moments(self._items(items, f"{type(self).__name__}.partial_fit")))

    def fold(self, m):
        """the host half of partial_fit: fold the per-item results `m` of moments() in item order"""
        if hasattr(self, "n_features_in_") and m.sum.shape[1] != self.n_features_in_:
            raise ValueError(f"{type(self).__name__}.fold: {m.sum.shape[1]} columns against {self.n_features_in_}")
        for b in range(len(m.n)):
            self._update(m, b)
        return self

    @torch.no_grad()
    def transform(self, items):
        """FeatsDataset's normalisation of every item: a list of (T, C) float32 device tensors (one tensor for one
        item), bit for bit datasets._scale followed by .astype(float32)"""
        if not hasattr(self, "n_samples_seen_"):
            raise ValueError(f"{type(self).__name__}.transform: the scaler is not fitted")
        listed = isinstance(items, (list, tuple))
        items = self._items(items, f"{type(self).__name__}.transform")
        out = scale_collate(items, *_operands(self.kind, self))
        out = [out[b, :len(v)] for b, v in enumerate(items)]
        return out if listed else out[0]

    def to_sklearn(self):
        """the sklearn object with these attributes (what stats.joblib holds in the reference)"""
        import sklearn.preprocessing
        sk = getattr(sklearn.preprocessing, type(self).__name__)()
        for name, v in vars(self).items():
            if name.endswith("_"):
                setattr(sk, name, v.copy() if isinstance(v, np.ndarray) else v)
        return sk


class StandardScaler(_Scaler):
    """sklearn.preprocessing.StandardScaler for float32 items: mean_, var_, scale_ (float64), n_samples_seen_"""
    kind = "standard"

    def _update(self, m, b):
        self._absorb(m.sum[b], m.m2[b], m.n[b], m.sum.shape[1])

    def _absorb(self, new_sum, new_m2, new_count, C):
        if not hasattr(self, "n_samples_seen_"):
            self.n_features_in_ = int(C)
            self.mean_, self.var_, self.n_samples_seen_ = np.zeros(C), np.zeros(C), np.int64(0)
        self.mean_, self.var_, self.n_samples_seen_ = _fold(self.mean_, self.var_, self.n_samples_seen_, new_sum,
                                                            new_m2, np.int64(new_count))
        # sklearn.preprocessing._data._is_constant_feature and _handle_zeros_in_scale
        n, eps = self.n_samples_seen_, np.finfo(np.float64).eps
        constant = self.var_ <= n * eps * self.var_ + np.square(n * self.mean_ * eps)
        self.scale_ = np.sqrt(self.var_)
        self.scale_[constant] = 1.0

    def merge(self, other):
        """fold another fitted StandardScaler (one shard of a dump) into this one by the same update"""
        if hasattr(other, "n_samples_seen_"):
            if hasattr(self, "n_features_in_") and len(other.mean_) != self.n_features_in_:
                raise ValueError(f"StandardScaler.merge: {len(other.mean_)} columns against {self.n_features_in_}")
            n = np.int64(other.n_samples_seen_)
            self._absorb(np.asarray(other.mean_) * n, np.asarray(other.var_) * n, n, len(other.mean_))
        return self


class MinMaxScaler(_Scaler):
    """sklearn.preprocessing.MinMaxScaler(feature_range=(0, 1)) for float32 items: data_min_, data_max_, data_range_,
    scale_, min_ (float32), n_samples_seen_"""
    kind = "minmax"
    feature_range = (0, 1)

    def _update(self, m, b):
        self._absorb(m.min[b], m.max[b], int(m.n[b]))

    def _absorb(self, lo, hi, count):
        lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
        if hasattr(self, "n_samples_seen_"):
            lo, hi = np.minimum(self.data_min_, lo), np.maximum(self.data_max_, hi)
            self.n_samples_seen_ += count
        else:
            self.n_features_in_, self.n_samples_seen_ = len(lo), count
        span = hi - lo
        divisor = span.copy()
        divisor[divisor < 10 * np.finfo(np.float32).eps] = 1.0  # _handle_zeros_in_scale
        lo_range, hi_range = (np.float32(v) for v in self.feature_range)
        self.scale_ = (hi_range - lo_range) / divisor
        self.min_ = lo_range - lo * self.scale_
        self.data_min_, self.data_max_, self.data_range_ = lo.copy(), hi.copy(), span

    def merge(self, other):
        """fold another fitted MinMaxScaler (one shard of a dump) into this one"""
        if hasattr(other, "n_samples_seen_"):
            if hasattr(self, "n_features_in_") and len(other.data_min_) != self.n_features_in_:
                raise ValueError(f"MinMaxScaler.merge: {len(other.data_min_)} columns against {self.n_features_in_}")
            self._absorb(other.data_min_, other.data_max_, int(other.n_samples_seen_))
        return self


# ---------------------------------------------------------------------------------------------------- stage 2
def _tracks(dump, score_type, logmel_type):
    """the four tracks of one dump dict, as extract_features returns it (stored names) or as FeatsDataset yields it
    (item keys)"""
    return {"hubert": dump["hubert"], "logmel": dump["logmel"] if "logmel" in dump else dump[logmel_type],
            "score": dump["score"] if "score" in dump else dump[score_type], "loud": dump["loud"]}


def fit_statistics(items, score_type="est_lf0_score", logmel_type="logmel", batch=8):
    """compute_statistics.py:121-141: StandardScaler on hubert and logmel, MinMaxScaler on score and loud, one
    partial_fit per utterance in the order given.  items: any iterable of dump dicts, as extract_features returns them
    or as FeatsDataset(scaler=None) yields them; None entries are skipped.  `batch` utterances share one launch per
    track, which changes no bit of the result."""
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"fit_statistics: batch={batch!r} must be a positive integer")
    scalers = {k: StandardScaler() if kind == "standard" else MinMaxScaler() for k, kind in ENTRIES.items()}
    pending = []

    def flush():
        for k, s in scalers.items():
            s.partial_fit([t[k] for t in pending])
        pending.clear()

    for dump in items:
        if dump is None:
            continue
        pending.append(_tracks(dump, score_type, logmel_type))
        if len(pending) == batch:
            flush()
    if pending:
        flush()
    if not hasattr(scalers["hubert"], "n_samples_seen_"):
        raise ValueError("fit_statistics: no utterance")
    return scalers


def save_statistics(scalers, path):
    """compute_statistics.py:144: joblib.dump of the dict, as sklearn objects where sklearn imports and as this
    module's own otherwise; ssc_decode and FeatsDataset read either (mean_, scale_, data_min_, data_max_)"""
    import joblib
    try:
        import sklearn.preprocessing  # noqa: F401
        scalers = {k: s.to_sklearn() if isinstance(s, _Scaler) else s for k, s in scalers.items()}
    except ImportError:
        pass
    joblib.dump(scalers, path)


# ---------------------------------------------------------------------------------------------------- the batch
class Collater:
    """FeatsDataset's normalisation and SSCCollater in one: called on a list of raw dump dicts (extract_features'
    or FeatsDataset(scaler=None)'s), sorts them by hubert length, longest first and stable, drops those of max_frames
    frames or more, and returns {"xs" (hubert), "lens", "ys" (logmel), "louds", "scores"}: normalised, zero-padded,
    contiguous float32 tensors on the device and int64 lens, as training.TrainSerenade takes them.  scaler: the dict
    of stats.joblib (sklearn's objects or this module's)."""

    def __init__(self, scaler, max_frames=3000, device=None, score_type="est_lf0_score", logmel_type="logmel"):
        missing = [k for k in ENTRIES if k not in scaler]
        if missing:
            raise ValueError(f"Collater: the scaler lacks {missing}")
        self.operands = {k: _operands(kind, scaler[k]) for k, kind in ENTRIES.items()}
        self.max_frames, self.device = int(max_frames), device
        self.score_type, self.logmel_type = score_type, logmel_type

    def __call__(self, batch):
        tracks = [_tracks(d, self.score_type, self.logmel_type) for d in batch if d is not None]
        order = sorted(range(len(tracks)), key=lambda i: -len(tracks[i]["hubert"]))
        order = [i for i in order if len(tracks[i]["hubert"]) < self.max_frames]
        if not order:
            raise ValueError(f"Collater: no utterance of fewer than {self.max_frames} frames in the batch")
        kept = sorted(order)  # only these are uploaded, in the order given
        where = {i: j for j, i in enumerate(kept)}
        picks = [where[i] for i in order]
        out = {}
        for name, key in (("xs", "hubert"), ("ys", "logmel"), ("louds", "loud"), ("scores", "score")):
            out[name] = scale_collate([tracks[i][key] for i in kept], *self.operands[key], order=picks,
                                      device=self.device)
        out["lens"] = torch.tensor([len(tracks[i]["hubert"]) for i in order], dtype=torch.int64,
                                   device=out["xs"].device)
        return out
