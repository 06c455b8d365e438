"""Float64 numpy restatement of serenade_amd/csrc/stats.hip and of the scalers' fold, every sum a plain
loop in the kernel's order.  No GPU, no sklearn: tests/test_stats_host.py pins it against scikit-learn, and
tests/test_hip_stats.py holds the kernels to it.

    col_moments(x)                      one item -> (sum, m2, min, max, nonfinite)
    StandardRef / MinMaxRef             .partial_fit(item) / .merge(other): sklearn's update formula, restated
    scale_collate(items, order, sub, div)   the padded, normalised batch of one track
    reference_chain(dumps, scaler, max_frames)   FeatsDataset's datasets._scale + a literal SSCCollater
"""
import numpy as np

from serenade_amd.datasets import _scale

WAVES = 4  # the kernel's row split: wave w adds the rows w, w + 4, ... in turn, then (s0 + s1) + s2 + s3
EPS = np.finfo(np.float64).eps


def _wave_sum(rows):
    """sum over axis 0 of a float64 (n, C) array in the kernel's order"""
    total = None
    for w in range(WAVES):
        acc = np.zeros(rows.shape[1], dtype=np.float64)
        for r in range(w, rows.shape[0], WAVES):
            acc = acc + rows[r]
        total = acc if total is None else total + acc
    return total


def col_moments(x):
    """srn_col_moments of one item x (n, C) float32"""
    assert x.dtype == np.float32 and x.ndim == 2
    n = x.shape[0]
    xd = x.astype(np.float64)
    s = _wave_sum(xd)
    d = xd - s / float(n)
    corr = _wave_sum(d)
    m2 = _wave_sum(d * d) - corr * corr / float(n)
    return s, m2, x.min(axis=0), x.max(axis=0), int((~np.isfinite(x)).sum())


class StandardRef:
    """StandardScaler.partial_fit, one item per call: the fold of sklearn.utils.extmath._incremental_mean_and_var on
    col_moments' sums, _is_constant_feature and _handle_zeros_in_scale"""

    def __init__(self):
        self.n_samples_seen_ = 0

    def _absorb(self, new_sum, new_m2, n_new):
        n_last = self.n_samples_seen_
        n = n_last + n_new
        if n_last == 0:
            self.mean_ = (0.0 + new_sum) / n
            m2 = new_m2
        else:
            last_sum = self.mean_ * n_last
            self.mean_ = (last_sum + new_sum) / n
            ratio = n_last / n_new
            m2 = self.var_ * n_last + new_m2 + ratio / n * (last_sum / ratio - new_sum) ** 2
        self.var_ = m2 / n
        self.n_samples_seen_ = n
        constant = self.var_ <= n * EPS * self.var_ + (n * self.mean_ * EPS) ** 2
        self.scale_ = np.where(constant, 1.0, np.sqrt(self.var_))

    def partial_fit(self, x):
        s, m2, _, _, _ = col_moments(x)
        self._absorb(s, m2, x.shape[0])
        return self

    def merge(self, other):
        n = other.n_samples_seen_
        self._absorb(other.mean_ * n, other.var_ * n, n)
        return self


class MinMaxRef:
    """MinMaxScaler(feature_range=(0, 1)).partial_fit, one item per call, float32 as sklearn keeps it"""

    def __init__(self):
        self.n_samples_seen_ = 0

    def _absorb(self, lo, hi, n_new):
        if self.n_samples_seen_:
            lo, hi = np.minimum(self.data_min_, lo), np.maximum(self.data_max_, hi)
        self.n_samples_seen_ += n_new
        self.data_min_, self.data_max_, self.data_range_ = lo, hi, hi - lo
        divisor = np.where(self.data_range_ < 10 * np.finfo(np.float32).eps, np.float32(1), self.data_range_)
        self.scale_ = np.float32(1) / divisor
        self.min_ = np.float32(0) - lo * self.scale_

    def partial_fit(self, x):
        _, _, lo, hi, _ = col_moments(x)
        self._absorb(lo, hi, x.shape[0])
        return self

    def merge(self, other):
        self._absorb(other.data_min_, other.data_max_, other.n_samples_seen_)
        return self


def scale_collate(items, order, sub, div):
    """srn_scale_collate: (len(order), Tmax, C) float32.  sub / div float64: the arithmetic is float64 and rounded
    once; float32: the arithmetic is float32."""
    assert sub.dtype == div.dtype and sub.dtype in (np.float32, np.float64)
    tmax = max(len(items[i]) for i in order)
    out = np.zeros((len(order), tmax, items[0].shape[1]), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b, i in enumerate(order):
            x = items[i].astype(sub.dtype)
            out[b, :len(x)] = ((x - sub) / div).astype(np.float32)
    return out


def operands(kind, entry):
    """(sub, div) of datasets._scale for a scaler entry, in the dtype numpy gives a float32 track against it"""
    if kind == "standard":
        sub, div = entry.mean_, entry.scale_
    else:
        sub, div = entry.data_min_, entry.data_max_ - entry.data_min_
    dtype = np.result_type(np.float32, sub.dtype, div.dtype)
    return sub.astype(dtype), div.astype(dtype)


KINDS = {"hubert": "standard", "logmel": "standard", "loud": "minmax", "score": "minmax"}
NAMES = {"xs": "hubert", "ys": "logmel", "louds": "loud", "scores": "score"}


def reference_chain(dumps, scaler, max_frames=3000, score_type="est_lf0_score"):
    """what the reference hands the training step: FeatsDataset.__getitem__'s normalisation (datasets._scale, numpy on
    the host) and SSCCollater written out literally -- sorted(key=-len(hubert)), the length filter, .float(), zero
    padding"""
    with np.errstate(divide="ignore", invalid="ignore"):
        items = [{"hubert": _scale(d["hubert"], scaler["hubert"], "standard"),
                  "logmel": _scale(d["logmel"], scaler["logmel"], "standard"),
                  "loud": _scale(d["loud"], scaler["loud"], "minmax"),
                  "score": _scale(d[score_type], scaler["score"], "minmax")} for d in dumps]
    batch = sorted(items, key=lambda x: -x["hubert"].shape[0])
    batch = [b for b in batch if len(b["hubert"]) < max_frames]
    out = {"lens": np.array([b["hubert"].shape[0] for b in batch], dtype=np.int64)}
    for name, key in NAMES.items():
        xs = [b[key].astype(np.float32) for b in batch]
        pad = np.zeros((len(xs), max(len(x) for x in xs)) + xs[0].shape[1:], dtype=np.float32)
        for i, x in enumerate(xs):
            pad[i, :len(x)] = x
        out[name] = pad
    return out


# ---------------------------------------------------------------------------------------------------- test data
def track(kind, n, seed, constant_column=None):
    """float32 (n, C): "logmel" N(-4, 2) C = 80, "hubert" N(0.1, 0.4) C = 768, "loud" / "score" C = 1"""
    rng = np.random.default_rng([seed, n, sorted(SHAPES).index(kind)])
    mean, std, C = SHAPES[kind]
    x = (mean + std * rng.standard_normal((n, C))).astype(np.float32)
    if constant_column is not None:
        x[:, constant_column] = np.float32(0.1)
    return x


SHAPES = {"logmel": (-4.0, 2.0, 80), "hubert": (0.1, 0.4, 768), "loud": (-30.0, 8.0, 1), "score": (5.5, 0.4, 1)}


def dumps(lengths, seed=0):
    """synthetic dump dicts with the tracks the scalers and the collater read"""
    return [{"hubert": track("hubert", n, seed + i), "logmel": track("logmel", n, seed + i),
             "loud": track("loud", n, seed + i), "est_lf0_score": track("score", n, seed + i)}
            for i, n in enumerate(lengths)]
