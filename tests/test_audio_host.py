"""Host side of serenade_amd/audio.py and the restatement tests/_audio_ref.py, no GPU: the filter geometry, the
restatement against scipy's independent polyphase implementation and against the analytic truth of band-limited
signals, trim on known answers, the window against np.pad, and the argument errors.

Recorded values of the committed restatement (the gates are twice these):
  truth, largest error away from the ends   24 -> 16 kHz 3.4e-7, 44.1 -> 24 3.0e-7, 16 -> 24 3.5e-7, 48 -> 24 2.6e-7,
                                            22.05 -> 24 3.1e-7
  stop band, unit sine at 1.05 new Nyquist  24 -> 16 kHz 1.1e-7, 44.1 -> 24 1.7e-7, 48 -> 24 0.9e-7
"""
import numpy as np
import pytest
import scipy.signal

from serenade_amd import audio as A

from . import _audio_ref as R

GEOMETRY = {(24000, 16000): (2, 3, 270), (44100, 24000): (80, 147, 13187), (48000, 24000): (1, 2, 180),
            (22050, 24000): (160, 147, 14354)}
TRUTH = {(24000, 16000): 3.4e-7, (44100, 24000): 3.0e-7, (16000, 24000): 3.5e-7, (48000, 24000): 2.6e-7,
         (22050, 24000): 3.1e-7}
STOPBAND = {(24000, 16000): 1.1e-7, (44100, 24000): 1.7e-7, (48000, 24000): 0.9e-7}
# frame_length 2048, hop 512, top_db 60, by hand from the rule.  The tone spans [3333, 8333) of 12433 samples and its
# second sample already carries more than the threshold, so the first frame with a tone sample is t = 5
# (512 t + 1024 > 3334) and the last t = 18 (512 t - 1024 <= 8332).  Exact zeros throughout: every frame sits at amin^2,
# the reference level too, and amin^2 > 1e-6 amin^2 -- the rule keeps the whole item, as amplitude_to_db(ref=np.max)
# does with a zero reference; (0, 0) needs a threshold no frame can pass, top_db = 0.
TRIM_BY_HAND = {"zeros_tone_zeros": (2560, 9728), "floor_tone_floor": (2560, 9728), "silent": (0, 6000),
                "loud": (0, 7001), "short": (0, 300)}


@pytest.mark.parametrize("rates", sorted(GEOMETRY))
def test_geometry(rates):
    assert A.resample_geometry(*rates) == GEOMETRY[rates] == R.geometry(*rates)[:3]
    h = A.resample_taps(*rates)
    L, M, half = GEOMETRY[rates]
    assert h.dtype == np.float64 and len(h) == 2 * half + 1
    assert np.abs(h - R.taps(*rates)).max() <= 1e-15  # two statements of one formula: a few ulp of h[0] = 2 fc L < 1
    assert abs(h.sum() / L - 1.0) <= 1e-6
    for n in (M, 7 * M, 1000 * M):
        for v in (n - 1, n, n + 1):
            assert A.resample_length(v, *rates) == int(np.ceil(v * (rates[1] / rates[0]))) == R.out_length(v, *rates)


@pytest.mark.parametrize("rates", sorted(GEOMETRY))
def test_polyphase_table_holds_every_tap_once(rates):
    L, M, half = GEOMETRY[rates]
    K, q_lo = A._table_shape(L, half)
    tab, h = A.polyphase_table(*rates), R.taps(*rates)
    assert tab.shape == (K, L)
    for p in sorted({0, 1 % L, L // 2, L - 1}):
        arg = p - (np.arange(K) - q_lo) * L
        inside = np.abs(arg) <= half
        assert np.abs(tab[inside, p] - h[arg[inside] + half]).max() <= 1e-15 and not tab[~inside, p].any()
        assert inside.sum() == np.count_nonzero((np.arange(-half, half + 1) - p) % L == 0)
    assert np.count_nonzero(tab) <= len(h) and np.isclose(tab.sum(), h.sum(), rtol=1e-12)


@pytest.mark.parametrize("rates", [(24000, 16000), (44100, 24000), (16000, 24000)])
def test_restatement_against_scipy(rates):
    L, M, half = R.geometry(*rates)[:3]
    x = np.random.default_rng(3).standard_normal(3001)
    ref = scipy.signal.resample_poly(x, L, M, window=R.taps(*rates) / L)
    got = R.resample(x, *rates)
    assert len(got) == len(ref)
    err = np.abs(got - ref).max()
    print(f"{rates}: restatement - scipy {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("rates", sorted(TRUTH))
def test_restatement_against_the_truth(rates):
    y = R.resample(R.sines(rates[0], *rates), *rates)
    assert len(y) == len(R.sines(rates[1], *rates))
    err = R.truth_error(y, *rates)
    print(f"{rates}: truth {err:.2e} (recorded {TRUTH[rates]:.1e})")
    assert err <= 2 * TRUTH[rates]


@pytest.mark.parametrize("rates", sorted(STOPBAND))
def test_restatement_stop_band(rates):
    level = R.stopband_level(R.resample(R.stopband_tone(*rates), *rates), *rates)
    print(f"{rates}: stop band {level:.2e} (recorded {STOPBAND[rates]:.1e})")
    assert level <= 2 * STOPBAND[rates]


@pytest.mark.parametrize("name", sorted(TRIM_BY_HAND))
def test_trim_known_answers(name):
    x = R.trim_signals()[name]
    bounds, near = R.trim(x)
    assert bounds == TRIM_BY_HAND[name]
    assert len(near) == 0
    assert A.trim_frames(len(x), 512) == 1 + len(x) // 512
    assert len(R.trim(x, frame_length=1000, hop=300)[1]) == 0  # the GPU file's other framing: no near-tie either
    assert R.trim(x, top_db=0)[0] == (0, 0)  # nothing lies above the loudest frame itself


def test_window_equals_numpy_pad():
    x = np.random.default_rng(4).standard_normal(700)
    for s, e, pad in ((0, 700, 512), (37, 640, 512), (37, 640, 602), (100, 102, 1), (5, 6, 0)):
        assert np.array_equal(R.window(x, s, e - s, pad), np.pad(x[s:e], (0, pad), "reflect"))
    assert np.array_equal(R.window(x, 3, 10, 4, width=20), np.concatenate([np.pad(x[3:13], (0, 4), "reflect"), np.zeros(6)]))


def test_argument_errors_come_before_the_device():
    x = np.zeros(100, dtype=np.float32)
    for bad in ((22050.5, 16000), (24000, 0), (24000, "16000"), (-8000, 16000)):
        with pytest.raises(ValueError):
            A.resample(x, *bad)
    with pytest.raises(ValueError, match="table"):
        A.resample(x, 24000, 23999)
    with pytest.raises(ValueError, match="tile"):
        A.resample(x, 192000, 8000)
    for empty in (np.zeros(0, np.float32), np.zeros((2, 0), np.float64)):
        with pytest.raises(ValueError):
            A.resample(empty, 24000, 16000)
        with pytest.raises(ValueError):
            A.trim(empty)
    with pytest.raises(ValueError):
        A.resample(np.zeros((2, 50)), 24000, 16000, lengths=[50, 0])
    with pytest.raises(ValueError):
        A.resample(np.zeros(100, np.int16), 24000, 16000)
    for pad in (100, 101, -1, 2.5):
        with pytest.raises(ValueError):
            A.pad_tail(x, pad)
    with pytest.raises(ValueError):
        A.pad_tail(np.zeros((2, 100)), 60, lengths=[100, 60])
    with pytest.raises(ValueError):
        A.trim(x, hop_length=0)
    config = {"sampling_rate": 24000, "trim_silence": False, "fft_size": 64}
    with pytest.raises(ValueError, match="16 bit PCM"):
        A.prepare([np.full(400, 1.5)], 24000, config)
    with pytest.raises(ValueError, match="16 bit PCM"):
        A.prepare([np.zeros(400), np.stack([np.full(400, 1.5), np.full(400, 0.9)], axis=1)], [24000, 44100], config)
    with pytest.raises(ValueError):
        A.prepare([np.zeros(400)], 24000.5, config)
