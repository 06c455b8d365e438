"""The feature scalers and the training batch on the MI355X (serenade_amd/stats.py + csrc/stats.hip) against the float64
restatement tests/_stats_ref.py and, where it is installed, scikit-learn: srn_col_moments at row counts on both sides
of the four-wave row split and of a 64-row edge and at column counts below, across and at multiples of the 64-column
tile, exact ragged batching, srn_scale_collate bit for bit against numpy for both arithmetic widths, fit_statistics,
the Collater against FeatsDataset's normalisation + a literal SSCCollater, and the stage-2 CLI.

Bounds as in tests/test_stats_host.py: sums within 1e-12 of sum|x| (the restatement follows the kernel's order, so
the measured differences are 0), min / max and everything srn_scale_collate writes bitwise."""
import numpy as np
import pytest
import torch

from serenade_amd import stats as S
from serenade_amd.bin import compute_statistics
from serenade_amd.datasets import FeatsDataset, _scale

from . import _stats_ref as R
from .test_stats_host import BOUND, _check_minmax, _check_standard

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 257)
COLUMNS = (1, 3, 65, 80, 768)
DUMP_LENGTHS = (5, 70, 3, 64, 69, 12, 64, 1)  # a tie, and one item at max_frames = 70
_CASES = {}


def _case(C):
    """(items, their restated moments), made once per column count"""
    if C not in _CASES:
        rng = np.random.default_rng(C)
        items = [(-4.0 + 2.0 * rng.standard_normal((n, C))).astype(np.float32) for n in LENGTHS]
        _CASES[C] = (items, [R.col_moments(x) for x in items])
    return _CASES[C]


def _same(a, b):
    return all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("C", COLUMNS)
def test_col_moments_against_the_restatement(C):
    items, ref = _case(C)
    m = S.moments(items)
    assert m.n.tolist() == list(LENGTHS) and m.sum.shape == m.m2.shape == m.min.shape == m.max.shape == (len(items), C)
    assert m.sum.dtype == m.m2.dtype == np.float64 and m.min.dtype == m.max.dtype == np.float32
    assert m.nonfinite.dtype == np.int32 and not m.nonfinite.any()
    worst = [0.0, 0.0]
    for b, (x, (s, m2, lo, hi, _)) in enumerate(zip(items, ref)):
        e_sum, e_m2 = np.abs(m.sum[b] - s), np.abs(m.m2[b] - m2)
        worst = [max(worst[0], (e_sum / np.abs(x).sum(axis=0)).max()), max(worst[1], (e_m2 / np.where(m2 > 0, m2, 1.0)).max())]
        assert (e_sum <= BOUND * np.abs(x).sum(axis=0)).all(), (C, b)
        assert (e_m2 <= BOUND * m2).all(), (C, b)
        assert m.min[b].tobytes() == lo.tobytes() and m.max[b].tobytes() == hi.tobytes(), (C, b)
    print(f"C={C}: sum {worst[0]:.2e} of sum|x|, m2 {worst[1]:.2e} relative")


@pytest.mark.parametrize("C", (1, 80))
def test_nonfinite_values_are_counted_in_their_item(C):
    items = [x.copy() for x in _case(C)[0]]
    items[2][0, 0], items[2][2, C - 1] = np.nan, np.inf
    m = S.moments(items, check=False)
    assert m.nonfinite.tolist() == [0, 0, 2] + [0] * (len(items) - 3)
    clean = S.moments(_case(C)[0])
    for b in range(len(items)):
        if b != 2:
            assert _same([v[b] for v in m[:5]], [v[b] for v in clean[:5]])
    with pytest.raises(ValueError, match="item 2 holds 2"):
        S.moments(items)
    with pytest.raises(ValueError, match="item 2"):
        S.StandardScaler().partial_fit(items)


@pytest.mark.parametrize("C", COLUMNS)
def test_a_batch_is_bit_for_bit_its_items(C):
    items = _case(C)[0]
    m = S.moments(items)
    for b, x in enumerate(items):
        one = S.moments([x])
        assert _same([v[b:b + 1] for v in m], one), (C, b)
    back = S.moments(items[::-1])
    assert _same([v[::-1] for v in back], m)
    mixed = [torch.from_numpy(x).to("cuda:0") if b % 2 else x for b, x in enumerate(items)]  # device and host items
    assert _same(S.moments(mixed), m)


@pytest.mark.parametrize("wide", (1, 0), ids=("f64", "f32"))
@pytest.mark.parametrize("C", COLUMNS)
def test_scale_collate_is_numpy_bit_for_bit(C, wide):
    items = _case(C)[0]
    order = [8, 3, 0, 7, 5, 1, 6, 2]  # item 4 is dropped
    rng = np.random.default_rng(100 + C)
    dtype = np.float64 if wide else np.float32
    sub, div = (-4.0 + rng.standard_normal(C)).astype(dtype), (0.5 + rng.random(C)).astype(dtype)
    want = R.scale_collate(items, order, sub, div)
    out = torch.full(want.shape, float("nan"), dtype=torch.float32, device="cuda:0")
    got = S.scale_collate(items, sub, div, order=order, out=out)
    assert got is out and got.is_contiguous()
    got = got.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    for b, i in enumerate(order):
        tail = got[b, LENGTHS[i]:]
        assert not tail.any() and not np.signbit(tail).any()  # exact +0.0
    assert S.scale_collate(items[3], sub, div).cpu().numpy().tobytes() == want[1:2, :LENGTHS[3]].tobytes()


@pytest.mark.parametrize("wide", (1, 0), ids=("f64", "f32"))
def test_a_zero_span_gives_numpys_inf_and_nan(wide):
    dtype = np.float64 if wide else np.float32
    items = [x.copy() for x in _case(3)[0][3:6]]
    sub, div = np.array([-4.0, 0.25, -4.0], dtype=dtype), np.array([2.0, 0.0, 2.0], dtype=dtype)
    for x in items:
        x[::2, 1] = 0.25  # 0 / 0 on every other row, +-inf on the rest
    want = R.scale_collate(items, [2, 0, 1], sub, div)
    got = S.scale_collate(items, sub, div, order=[2, 0, 1]).cpu().numpy()
    assert np.isnan(want).any() and np.isinf(want).any()
    assert (np.isnan(got) == np.isnan(want)).all()
    keep = ~np.isnan(want)
    assert got[keep].tobytes() == want[keep].tobytes()


def _reference_scalers(dumps):
    """sklearn's four scalers fed one partial_fit per dump, or the restatement's where sklearn is absent"""
    try:
        from sklearn.preprocessing import MinMaxScaler, StandardScaler
    except ImportError:
        StandardScaler, MinMaxScaler = R.StandardRef, R.MinMaxRef
    ref = {"hubert": StandardScaler(), "logmel": StandardScaler(), "score": MinMaxScaler(), "loud": MinMaxScaler()}
    for d in dumps:
        for k, s in ref.items():
            s.partial_fit(d["est_lf0_score" if k == "score" else k])
    return ref


@pytest.fixture(scope="module")
def dumps():
    d = R.dumps(DUMP_LENGTHS)
    return d, _reference_scalers(d)


def test_fit_statistics(dumps):
    dumps, ref = dumps
    got = S.fit_statistics(dumps)
    assert sorted(got) == ["hubert", "logmel", "loud", "score"]
    for k in ("hubert", "logmel"):
        _check_standard(got[k], ref[k], [d[k] for d in dumps], None, k)
    _check_minmax(got["score"], ref["score"])
    _check_minmax(got["loud"], ref["loud"])
    # None entries are skipped, FeatsDataset's item keys are read too, and the launch grouping changes no bit
    as_items = [None] + [{"hubert": d["hubert"], "logmel": d["logmel"], "loud": d["loud"], "score": d["est_lf0_score"]}
                         for d in dumps]
    again = S.fit_statistics(iter(as_items), batch=3)
    for k in ("hubert", "logmel"):
        assert _same([again[k].mean_, again[k].var_, again[k].scale_], [got[k].mean_, got[k].var_, got[k].scale_])
    _check_minmax(again["loud"], got["loud"])
    one, many = S.StandardScaler(), S.StandardScaler().partial_fit([d["logmel"] for d in dumps])
    for d in dumps:
        one.partial_fit(d["logmel"])
    assert _same([one.mean_, one.var_, one.scale_], [many.mean_, many.var_, many.scale_])
    assert _same([many.mean_, many.var_], [got["logmel"].mean_, got["logmel"].var_])
    x = dumps[3]["logmel"]
    want = _scale(x, got["logmel"], "standard").astype(np.float32)
    assert got["logmel"].transform(x).cpu().numpy().tobytes() == want.tobytes()
    want = _scale(dumps[4]["loud"], got["loud"], "minmax")
    assert want.dtype == np.float32
    assert got["loud"].transform([dumps[3]["loud"], dumps[4]["loud"]])[1].cpu().numpy().tobytes() == want.tobytes()


def test_collater_is_the_reference_chain(dumps):
    dumps, ref = dumps
    want = R.reference_chain(dumps, ref, max_frames=70)
    got = S.Collater(ref, max_frames=70)(dumps)
    assert sorted(got) == ["lens", "louds", "scores", "xs", "ys"]
    assert got["lens"].dtype == torch.int64 and got["lens"].tolist() == want["lens"].tolist() == [69, 64, 64, 12, 5, 3, 1]
    for name, width in (("xs", 768), ("ys", 80), ("louds", 1), ("scores", 1)):
        t = got[name]
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (7, 69, width)
        assert t.cpu().numpy().tobytes() == want[name].tobytes(), name
    mine = S.Collater(S.fit_statistics(dumps), max_frames=70)(dumps + [None])  # this module's own scalers serve too
    assert mine["lens"].tolist() == want["lens"].tolist() and tuple(mine["xs"].shape) == (7, 69, 768)
    assert mine["louds"].cpu().numpy().tobytes() == want["louds"].tobytes()  # min / max are bitwise sklearn's


def test_cli_writes_stats_that_the_dataset_reads(dumps, tmp_path):
    import joblib
    dumps, ref = dumps
    root = tmp_path / "raw"
    root.mkdir()
    for i, d in enumerate(dumps):
        n = len(d["hubert"])
        np.savez(root / f"utt{i}.npz", wave=np.zeros(8, np.float32), f0=np.zeros((n, 1), np.float32),
                 midi=np.zeros((n, 1), np.float32), **d)
    config = tmp_path / "conf.yaml"
    config.write_text("sampling_rate: 24000\n")
    compute_statistics.main(["--rootdir", str(root), "--config", str(config), "--dumpdir", str(tmp_path / "out"),
                             "--verbose", "0"])
    scaler = joblib.load(tmp_path / "out" / "stats.joblib")
    direct = S.fit_statistics(dumps)  # utt0 .. utt7 sort as they were written
    for k in ("hubert", "logmel"):
        assert _same([scaler[k].mean_, scaler[k].scale_], [direct[k].mean_, direct[k].scale_])
    for k in ("score", "loud"):
        assert _same([scaler[k].data_min_, scaler[k].data_max_], [direct[k].data_min_, direct[k].data_max_])
    item = FeatsDataset(str(root), scaler=scaler, return_utt_id=True)[3]
    assert item["utt_id"] == "utt3"
    assert item["logmel"].tobytes() == _scale(dumps[3]["logmel"], direct["logmel"], "standard").tobytes()
    assert item["loud"].tobytes() == _scale(dumps[3]["loud"], ref["loud"], "minmax").tobytes()
