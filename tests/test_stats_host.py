"""Host side of serenade_amd/stats.py and the restatement tests/_stats_ref.py, no GPU: the restatement pinned against
scikit-learn fed the same items one partial_fit each, the scalers' fold and merge on restated moments, to_sklearn
through joblib, the collate restatement against datasets._scale and a literal SSCCollater, and the argument errors.

Bounds.  mean_ within 1e-12 x mean|x| and var_ within 1e-12 relative: a sum of n <= 4500 terms of one sign is, over
any order, within about n 2^-53 = 5e-13 of the truth, doubled for the fold.  Measured with the kernel's order
(wave w adds rows w, w + 4, ..., then (s0 + s1) + s2 + s3) against scikit-learn 1.7.2: mean_ 0 on every track (sums of
float32 values in fp64 are exact here; 2.2e-16 after a merge), var_ at most 3.1e-15 relative.  min / max
are the input's own values: bitwise.
"""
import numpy as np
import pytest

from serenade_amd import stats as S
from serenade_amd.bin import compute_statistics

from . import _stats_ref as R

LENGTHS = (1, 2, 63, 64, 65, 257, 1000, 2999)
BOUND = 1e-12
CONSTANT = {"logmel": 7, "hubert": 700, "loud": None, "score": None}


@pytest.fixture(scope="module")
def sk():
    return pytest.importorskip("sklearn.preprocessing")


@pytest.fixture(scope="module")
def tracks():
    """kind -> the eight items, one column of the wide tracks constant"""
    return {k: [R.track(k, n, seed=3, constant_column=CONSTANT[k]) for n in LENGTHS] for k in R.SHAPES}


def _restated_moments(items):
    cols = list(zip(*[R.col_moments(x) for x in items]))
    return S.Moments(np.array([len(x) for x in items], dtype=np.int64), np.stack(cols[0]), np.stack(cols[1]),
                     np.stack(cols[2]), np.stack(cols[3]), np.array(cols[4], dtype=np.int32))


def _check_standard(got, want, items, constant, label):
    """got against want (sklearn's or another statement's attributes) to the bounds of the module docstring"""
    assert int(got.n_samples_seen_) == int(want.n_samples_seen_)
    assert got.mean_.dtype == got.var_.dtype == got.scale_.dtype == np.float64
    scale = np.abs(np.concatenate(items)).mean(axis=0)
    e_mean = (np.abs(got.mean_ - want.mean_) / scale).max()
    live = np.ones(len(scale), dtype=bool)
    if constant is not None:
        live[constant] = False
        assert got.scale_[constant] == 1.0 and want.scale_[constant] == 1.0
    e_var = np.abs(got.var_ - want.var_)[live]
    rel = (e_var / np.where(want.var_[live] > 0, want.var_[live], 1.0)).max()
    print(f"{label}: n {int(got.n_samples_seen_)}, mean_ {e_mean:.2e} of mean|x|, var_ {rel:.2e} relative")
    assert e_mean <= BOUND
    assert (e_var <= BOUND * want.var_[live]).all()
    assert (np.abs(got.scale_ - want.scale_)[live] <= BOUND * want.scale_[live]).all()


def _check_minmax(got, want):
    assert int(got.n_samples_seen_) == int(want.n_samples_seen_)
    for name in ("data_min_", "data_max_", "data_range_", "scale_", "min_"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
def test_restatement_against_sklearn(sk, tracks, kind):
    items = tracks[kind]
    std, mm, rstd, rmm = sk.StandardScaler(), sk.MinMaxScaler(), R.StandardRef(), R.MinMaxRef()
    for i, x in enumerate(items):  # one partial_fit each, compared after every one
        std.partial_fit(x), mm.partial_fit(x), rstd.partial_fit(x), rmm.partial_fit(x)
        _check_standard(rstd, std, items[:i + 1], CONSTANT[kind], f"{kind} after {i + 1}")
        _check_minmax(rmm, mm)


@pytest.mark.parametrize("kind", sorted(R.SHAPES))
def test_the_scalers_fold_as_sklearn_does(sk, tracks, kind):
    """stats.StandardScaler / MinMaxScaler on the restated moments: sklearn's attributes, names and dtypes; a list is bit
    for bit its items one at a time; two statements of one formula agree bit for bit"""
    items = tracks[kind]
    m = _restated_moments(items)
    std, mm = S.StandardScaler().fold(m), S.MinMaxScaler().fold(m)
    sstd, smm = sk.StandardScaler(), sk.MinMaxScaler()
    rstd, rmm = R.StandardRef(), R.MinMaxRef()
    one_std, one_mm = S.StandardScaler(), S.MinMaxScaler()
    for b, x in enumerate(items):
        sstd.partial_fit(x), smm.partial_fit(x), rstd.partial_fit(x), rmm.partial_fit(x)
        single = S.Moments(*[v[b:b + 1] for v in m])
        one_std.fold(single), one_mm.fold(single)
    _check_standard(std, sstd, items, CONSTANT[kind], kind)
    _check_minmax(mm, smm)
    assert type(std.n_samples_seen_) is type(sstd.n_samples_seen_) and type(mm.n_samples_seen_) is type(smm.n_samples_seen_)
    assert std.n_features_in_ == sstd.n_features_in_ == items[0].shape[1] and mm.feature_range == smm.feature_range
    for name in ("mean_", "var_", "scale_"):
        assert getattr(std, name).tobytes() == getattr(one_std, name).tobytes() == getattr(rstd, name).tobytes(), name
    _check_minmax(mm, one_mm)
    _check_minmax(mm, rmm)


@pytest.mark.parametrize("kind", ["logmel", "loud"])
def test_merge_of_two_halves_is_the_whole(sk, tracks, kind):
    items = tracks[kind]
    whole_std, whole_mm = sk.StandardScaler(), sk.MinMaxScaler()
    for x in items:
        whole_std.partial_fit(x), whole_mm.partial_fit(x)
    for first in (3, 5):
        a, b = _restated_moments(items[:first]), _restated_moments(items[first:])
        std = S.StandardScaler().fold(a).merge(S.StandardScaler().fold(b))
        mm = S.MinMaxScaler().fold(a).merge(S.MinMaxScaler().fold(b))
        _check_standard(std, whole_std, items, CONSTANT[kind], f"{kind} merged at {first}")
        _check_minmax(mm, whole_mm)
        rstd = R.StandardRef()
        for x in items[:first]:
            rstd.partial_fit(x)
        other = R.StandardRef()
        for x in items[first:]:
            other.partial_fit(x)
        _check_standard(rstd.merge(other), whole_std, items, CONSTANT[kind], f"{kind} restated merge at {first}")
    # an sklearn-fitted shard merges too, and an unfitted one changes nothing
    std = S.StandardScaler().fold(_restated_moments(items[:3]))
    rest = sk.StandardScaler()
    for x in items[3:]:
        rest.partial_fit(x)
    before = std.mean_.copy()
    assert std.merge(S.StandardScaler()).mean_.tobytes() == before.tobytes()
    _check_standard(std.merge(rest), whole_std, items, CONSTANT[kind], f"{kind} merged with sklearn's")


def test_to_sklearn_round_trips_through_joblib(sk, tracks, tmp_path):
    """sklearn's own transform rounds twice (x -= mean_; x /= scale_ in float32, and x * scale_ + min_), FeatsDataset's
    expression once, so they agree to the roundings between them, each 2^-24 relative: three on the standard side, and
    on the min-max side two each on x scale_ and on min_ and three on the result."""
    import joblib
    ours = {"logmel": S.StandardScaler().fold(_restated_moments(tracks["logmel"])),
            "loud": S.MinMaxScaler().fold(_restated_moments(tracks["loud"]))}
    path = tmp_path / "stats.joblib"
    S.save_statistics(ours, path)
    back = joblib.load(path)
    assert isinstance(back["logmel"], sk.StandardScaler) and isinstance(back["loud"], sk.MinMaxScaler)
    for k, names in (("logmel", ("mean_", "var_", "scale_")), ("loud", ("data_min_", "data_max_", "data_range_", "scale_", "min_"))):
        assert int(back[k].n_samples_seen_) == int(ours[k].n_samples_seen_)
        for name in names:
            a, b = getattr(back[k], name), getattr(ours[k], name)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (k, name)
    x = tracks["logmel"][4]
    mine = R.scale_collate([x], [0], *R.operands("standard", back["logmel"]))[0]
    assert (np.abs(back["logmel"].transform(x) - mine) <= 2.0 ** -22 * np.abs(mine)).all()
    x = tracks["loud"][4]
    entry = back["loud"]
    mine = R.scale_collate([x], [0], *R.operands("minmax", entry))[0]
    bound = 2.0 ** -22 * ((np.abs(x) + np.abs(entry.data_min_)) / entry.data_range_ + np.abs(mine))
    assert (np.abs(entry.transform(x) - mine) <= bound).all()
    # this module's own objects pickle too (what is written where sklearn is absent) and carry what the readers read
    joblib.dump(ours, path)
    again = joblib.load(path)
    assert again["logmel"].mean_.tobytes() == ours["logmel"].mean_.tobytes()
    assert again["loud"].data_max_.tobytes() == ours["loud"].data_max_.tobytes()


def test_collate_restatement_is_the_reference_chain(sk):
    """datasets._scale (numpy on the host) + a literal SSCCollater against the restatement of srn_scale_collate, bit for
    bit, for sklearn-fitted scalers: float64 operands for hubert / logmel, float32 for loud / score; a tie in length
    keeps the given order, an item of max_frames frames is dropped"""
    lengths = (5, 70, 3, 64, 69, 12, 64, 1)
    dumps = R.dumps(lengths)
    scaler = {"hubert": sk.StandardScaler(), "logmel": sk.StandardScaler(), "score": sk.MinMaxScaler(),
              "loud": sk.MinMaxScaler()}
    for d in dumps:
        for k, s in scaler.items():
            s.partial_fit(d["est_lf0_score" if k == "score" else k])
    want = R.reference_chain(dumps, scaler, max_frames=70)
    order = [4, 3, 6, 5, 0, 2, 7]
    assert want["lens"].tolist() == [lengths[i] for i in order]
    for name, key in R.NAMES.items():
        sub, div = R.operands(R.KINDS[key], scaler[key])
        assert sub.dtype == div.dtype == (np.float64 if R.KINDS[key] == "standard" else np.float32)
        mine = S._operands(R.KINDS[key], scaler[key])
        assert mine[0].dtype == sub.dtype and mine[0].tobytes() == sub.tobytes() and mine[1].tobytes() == div.tobytes()
        items = [d["est_lf0_score" if key == "score" else key] for d in dumps]
        got = R.scale_collate(items, order, sub, div)
        assert got.dtype == want[name].dtype == np.float32 and got.shape == want[name].shape
        assert got.tobytes() == want[name].tobytes(), name


def test_argument_errors_need_no_device(tracks):
    x = tracks["logmel"][3]
    for bad, word in (([], "no item"), ([x, x[:0]], "not empty"), ([x, x[:, :3]], "columns"),
                      ([x.astype(np.float64)], "float32"), ([x[:, 0]], r"\(T, C\)"), ([[1.0, 2.0]], "numpy array")):
        with pytest.raises(ValueError, match=word):
            S.moments(bad)
        with pytest.raises(ValueError, match=word):
            S.StandardScaler().partial_fit(bad)
    sub = np.zeros(80)
    for kw, word in ((dict(sub=sub, div=sub.astype(np.float32)), "both"), (dict(sub=sub[:3], div=sub[:3]), r"\(80,\)"),
                     (dict(sub=sub, div=sub, order=[1]), "order"), (dict(sub=sub, div=sub, order=[]), "order"),
                     (dict(sub=sub.astype(np.int64), div=sub.astype(np.int64)), "both")):
        with pytest.raises(ValueError, match=word):
            S.scale_collate([x], **kw)
    fitted = S.StandardScaler().fold(_restated_moments(tracks["logmel"]))
    with pytest.raises(ValueError, match="columns"):
        fitted.partial_fit(tracks["hubert"][0])
    with pytest.raises(ValueError, match="columns"):
        fitted.merge(S.StandardScaler().fold(_restated_moments(tracks["loud"])))
    with pytest.raises(ValueError, match="not fitted"):
        S.MinMaxScaler().transform(x)
    with pytest.raises(ValueError, match="batch"):
        S.fit_statistics([], batch=0)
    with pytest.raises(ValueError, match="no utterance"):
        S.fit_statistics([None, None])
    scaler = {"hubert": S.StandardScaler().fold(_restated_moments(tracks["hubert"])), "logmel": fitted,
              "score": S.MinMaxScaler().fold(_restated_moments(tracks["score"])),
              "loud": S.MinMaxScaler().fold(_restated_moments(tracks["loud"]))}
    with pytest.raises(ValueError, match="lacks"):
        S.Collater({"hubert": fitted})
    with pytest.raises(ValueError, match="fewer than 3 frames"):
        S.Collater(scaler, max_frames=3)(R.dumps((3, 7)))


def test_cli_refuses_feats_scp(tmp_path):
    config = tmp_path / "c.yaml"
    config.write_text("sampling_rate: 24000\n")
    for extra in (["--feats-scp", "feats.scp"], ["--feats-scp", "feats.scp", "--rootdir", str(tmp_path)], []):
        with pytest.raises(ValueError, match="Please specify either --rootdir or --feats-scp."):
            compute_statistics.main(["--config", str(config), "--dumpdir", str(tmp_path / "out")] + extra)
