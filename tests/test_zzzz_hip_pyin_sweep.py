"""The pYIN kernels on the MI355X (csrc/pyin.hip through serenade_amd/pitch.py) at the edge cases of
tests/_pyin_cases.py against the float64 restatement tests/_pyin_ref.py: more than 1024 bins and 2048 states, bands of
one bin and of nearly all bins, switch probabilities 0 and 1 (the exact-tie scan), threshold counts around the 64-lane
stride and other priors, the shortest period range and the largest geometry the LDS budget admits, hundreds of troughs
per frame, other fills, no centring, an explicit window, loud and quiet input, items of 1 / 319 / 320 / 321 samples,
silence, a strided batch.  tests/test_pyin_cases_host.py proves on the CPU that each case is decided and reaches the
branch it is named for.

Per case two comparisons: the observation kernel's matrix and voiced probability straight from the plan (1e-12
absolute; a probability in a bin that loses the Viterbi is invisible in the decoded path), then the decoded states, f0
and flags (identical off the near-tie frames, tests/test_hip_pyin.py's rule).  The kernel's header claims every rounding
is the restatement's, so each case also prints its largest difference and whether it was bit-equal.

The file is named to sort after every other test file (like the test_zz_ / test_zzz_ files before it), so that the
suite that was there before runs in the order and from the state it ran in without it."""
import numpy as np
import pytest
import torch

from serenade_amd import _lib, pitch
from tests import _pyin_cases as C
from tests import _pyin_ref as R
from tests.test_hip_pyin import _compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(waves, fill=1e4):
    """padded batch; the tail holds large values that no valid frame may read"""
    lens = [len(w) for w in waves]
    x = torch.full((len(waves), max(lens)), fill, dtype=torch.float32)
    for i, w in enumerate(waves):
        x[i, :len(w)] = torch.from_numpy(np.array(w))
    return x.to(DEV), lens


def _run(names, x, lens):
    """one pyin call on the batch x of the cases `names` (which share their keywords), then the observation kernel once
    more on its own into cleared buffers: the plan's obs and vp are what it wrote.  Compares every item."""
    kw = C.BY_NAME[names[0]].kw
    f0, flag, vp, frames = pitch.pyin(x, lens, **kw)
    plan = next(reversed(pitch._PLANS.values()))  # the plan of this call: the most recently used
    assert (plan.B, plan.N) == tuple(x.shape) and plan.frames.tolist() == frames.tolist()
    states = plan.states.cpu().numpy()
    plan.obs.fill_(float("nan"))
    plan.vp.fill_(float("nan"))
    plan.observe(x, None)
    torch.cuda.synchronize()
    obs, ovp = plan.obs.cpu().numpy(), plan.vp.cpu().numpy()
    f0, flag, vp = f0.cpu().numpy(), flag.cpu().numpy(), vp.cpu().numpy()
    fill = kw.get("fill_na", np.nan)
    for i, name in enumerate(names):
        case = C.BY_NAME[name]
        rf0, rflag, rvp, near, st = C.ref(case)
        n = int(frames[i])
        assert n == len(rf0), name
        e_obs = np.abs(obs[i, :n] - st["voiced"]).max()
        e_vp = max(np.abs(ovp[i, :n] - rvp).max(), np.abs(vp[i, :n] - rvp).max())
        exact = np.array_equal(obs[i, :n], st["voiced"]) and np.array_equal(ovp[i, :n], rvp)
        print(f"{name}: observations {e_obs:.2e}, voiced_prob {e_vp:.2e} over {n} frames x {st['voiced'].shape[1]} bins"
              f" ({'bit-equal' if exact else 'not bit-equal'})")
        assert e_obs <= C.TOL and e_vp <= C.TOL, name
        assert (ovp[i, n:] == 0).all() and (vp[i, n:] == 0).all() and not flag[i, n:].any(), name
        past = f0[i, n:]
        assert (past == 0.0).all() if fill is None else np.array_equal(past, np.full(len(past), fill), equal_nan=True)
        if case.absolute:  # known without the restatement; its near flag (set on every such frame) excuses nothing
            assert not obs[i, :n].any() and not ovp[i, :n].any() and not vp[i, :n].any() and not flag[i, :n].any()
            assert np.isnan(f0[i, :n]).all() and (states[i, :n] >= st["voiced"].shape[1]).all(), name
            continue
        _compare(name, (f0[i, :n], flag[i, :n], vp[i, :n]), (rf0, rflag, rvp, near))
        assert np.array_equal(states[i, :n][~near], st["states"][~near]), name
        assert (states[i, n:] == -1).all()


@pytest.mark.parametrize("name", C.SINGLE)
def test_case_against_the_restatement(name):
    x, lens = _batch([C.BY_NAME[name].y])
    _run([name], x, lens)


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
def test_ragged_batch_of_frame_count_edges(strided):
    """1, 319, 320 and 321 samples (hop 320), silence and a 4000-sample item in one call, the tail filled with 1e4;
    strided: the same batch as the view wide[:, :N] of a wider tensor, so that the row stride exceeds N"""
    x, lens = _batch([C.BY_NAME[k].y for k in C.RAGGED])
    if strided:
        wide = torch.full((x.shape[0], x.shape[1] + 37), -7e3, dtype=torch.float32, device=DEV)
        wide[:, :x.shape[1]] = x
        x = wide[:, :x.shape[1]]
        assert x.stride(0) > x.shape[1] and not x.is_contiguous()
    _run(C.RAGGED, x, lens)


def test_fill_none_past_the_item_is_zero_and_unvoiced_frames_carry_their_bin():
    waves = [C.BY_NAME["fill-none"].y, C.BY_NAME["len4000"].y]
    x, lens = _batch(waves)
    kw = C.BY_NAME["fill-none"].kw
    f0, flag, vp, frames = pitch.pyin(x, lens, **kw)
    f0, flag = f0.cpu().numpy(), flag.cpu().numpy()
    rf0, rflag, _, near, _ = C.ref(C.BY_NAME["fill-none"])
    assert (~rflag).any() and (rf0[~rflag] > 0).all()
    assert np.array_equal(f0[0][~near], rf0[~near]) and np.array_equal(flag[0][~near], rflag[~near])
    n1 = int(frames[1])
    assert n1 < f0.shape[1] and (f0[1, n1:] == 0.0).all() and (f0[1, :n1] > 0).all()
    z0 = pitch.pyin(x, lens, **dict(kw, fill_na=0.0))[0].cpu().numpy()
    assert np.array_equal(z0, np.where(flag, f0, 0.0))


def test_viterbi_alone_beyond_1024_bins_takes_an_out_of_band_leap():
    """1203 bins, 2406 states: the second trip of the kernel's loop over bins and of its argmax over states; a leap of
    600 bins inside a run of certain frames, a run without observations, ragged frame counts"""
    voiced, vp, frames, ref = C.synthetic_leap()
    B, T, n = voiced.shape
    w, s = 181, 0.01
    d = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    p_init = np.zeros(2 * n)
    p_init[n:] = 1 / n
    band, lpi = d(pitch.log_band(n, w, s)), d(np.log(p_init + R.TINY))
    obs, vpd, fr = d(voiced), d(vp), torch.tensor(frames, dtype=torch.int32, device=DEV)
    ptr = torch.empty(B, T, 2 * n, dtype=torch.int16, device=DEV)
    states = torch.empty(B, T, dtype=torch.int32, device=DEV)
    f0 = torch.empty(B, T, dtype=torch.float64, device=DEV)
    flag = torch.empty(B, T, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().srn_pyin_viterbi(
        obs.data_ptr(), vpd.data_ptr(), fr.data_ptr(), band.data_ptr(), lpi.data_ptr(),
        d(np.arange(2 * n, dtype=np.float64)).data_ptr(), float(np.log(R.TINY)), float("nan"), 1, ptr.data_ptr(),
        states.data_ptr(), f0.data_ptr(), flag.data_ptr(), B, T, n, w, None), "viterbi")
    torch.cuda.synchronize()
    st = states.cpu().numpy()
    for b in range(B):
        assert np.array_equal(st[b, :frames[b]], ref[b]), b
        assert (st[b, frames[b]:] == -1).all()
    assert list(st[0, 3:11]) == [100] * 4 + [700] * 4


def test_limits_are_refused_before_any_launch():
    x = torch.zeros(1, 3000, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="1339 periods"):
        pitch.pyin(x, fmin=32.7, fmax=4000, sr=44100, frame_length=4096)
    with pytest.raises(ValueError, match="shorter than frame_length"):
        pitch.pyin(x, [3000], fmin=65, fmax=2093, sr=16000, frame_length=4096, center=False)
    with pytest.raises(ValueError, match="transition width"):
        pitch.pyin(x, fmin=100, fmax=800, sr=8000, frame_length=512, win_length=300, hop_length=700)


@pytest.mark.parametrize("fill", [1e4, float("nan")], ids=["1e4", "nan"])
def test_ragged_items_equal_their_own_calls_bit_for_bit(fill):
    waves = [C.BY_NAME[k].y for k in C.EXACT]
    x, lens = _batch(waves, fill)
    f0, flag, vp, frames = (t.cpu() for t in pitch.pyin(x, lens, **C.TRANS))
    nn = lambda t: torch.nan_to_num(t, nan=-1.0)
    for i, w in enumerate(waves):
        f1, fl1, vp1, fr1 = pitch.pyin(torch.from_numpy(np.array(w)).to(DEV), **C.TRANS)
        n = int(fr1[0])
        assert n == int(frames[i])
        assert torch.equal(nn(f0[i, :n]), nn(f1.cpu())) and torch.equal(flag[i, :n], fl1.cpu()), C.EXACT[i]
        assert torch.equal(vp[i, :n], vp1.cpu()), C.EXACT[i]
        assert np.isnan(f0[i, n:].numpy()).all() and not flag[i, n:].any() and not vp[i, n:].any()
