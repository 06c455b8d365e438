"""GPU feature front-end: the log-mel spectrogram and A-weighted loudness the reference computes with librosa on the
CPU before the hot path.

    logmelfilterbank(audio, sampling_rate, fft_size, hop_size, win_length, window, num_mels, fmin, fmax, eps,
                     log_base)                       serenade/bin/preprocess.py:140-203
    loudness_extract(audio, sampling_rate, hop_length)   serenade/bin/preprocess.py:126-137

Same names, arguments and return shapes ((#frames, num_mels) and (#frames,)); `audio` may also be a (B, n) batch of
equal-length signals, which adds a leading batch axis to the result.  With `lengths=` (B sample counts) the batch is a
padded one of unequal utterances, as audio.prepare returns it: each item is padded, analysed and -- for the loudness
floor -- normalised on its own, frames at or past an item's own 1 + n_b // hop are exactly 0 and the call returns
(tensor, [frames per item]), the convention of ContentVec and TranscriptionModel.  Inputs are CUDA tensors (numpy arrays
are uploaded); everything runs in libserenade_hip.so: the STFT is a strided implicit GEMM (`srn_conv_gemm`, exact-fp32
MFMA) over the padded signal viewed as rows of 16 samples with window x DFT basis weights, followed by `srn_logmel` /
`srn_loudness` (`srn_logmel_ragged` / `srn_loudness_ragged` with lengths).  The constant tables (window x DFT basis,
Slaney mel filterbank, A-weighting) are built on the host in float64 once per process and device (`_table`), whatever
(B, n) the plans that use them have.  There is no CPU path.

Parity: librosa is not vendored by the reference and not installed here, so this row is pinned to the restatement
in oracle/features_oracle.py only ("parity unpinned").
"""
import math

import numpy as np
import torch

from . import _lib, ops
from .plan import item_lengths, lru_get, require_cuda as _require_cuda, rup

__all__ = ["logmelfilterbank", "loudness_extract"]

_PLANS = {}
_TABLES = {}  # (device, what, what it depends on) -> device tensor: one copy per process, shared by every plan


# ---------------------------------------------------------------------------------------------- constant tables
def _hann_padded(n_fft, win_length):
    n = np.arange(win_length, dtype=np.float64)
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)  # periodic Hann, centred in the frame
    return w


def _dft_basis(n_fft, win_length, n_pad):
    """(n_pad, n_fft): rows [0, nb) = w cos, rows [nb, 2 nb) = -w sin (rfft sign), zero rows up to n_pad"""
    nb = 1 + n_fft // 2
    w = _hann_padded(n_fft, win_length)
    ang = 2.0 * np.pi * np.outer(np.arange(nb), np.arange(n_fft)) / n_fft
    basis = np.zeros((n_pad, n_fft))
    basis[:nb] = np.cos(ang) * w
    basis[nb:2 * nb] = -np.sin(ang) * w
    return basis.astype(np.float32)


def _slaney_mel(sr, n_fft, n_mels, fmin, fmax):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    to_mel = lambda f: min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp
    mels = np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2)
    hz = np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)), f_sp * mels)
    fft_f = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    ramps = hz[:, None] - fft_f[None, :]
    d = np.diff(hz)
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / d[:-1, None], ramps[2:] / d[1:, None]))
    return w * (2.0 / (hz[2:] - hz[:-2]))[:, None]  # Slaney area normalisation


def _a_weight_db(freqs, min_db=-80.0):
    f2 = np.asarray(freqs, dtype=np.float64) ** 2
    c = np.array([12194.217, 20.598997, 107.65265, 737.86223]) ** 2
    with np.errstate(divide="ignore"):
        w = 2.0 + 20.0 * (np.log10(c[0]) + 2 * np.log10(f2) - np.log10(f2 + c[0]) - np.log10(f2 + c[1])
                          - 0.5 * np.log10(f2 + c[2]) - 0.5 * np.log10(f2 + c[3]))
    return np.maximum(min_db, w)


def _table(dev, key, make):
    """the per-process device copy of a constant table: built (host, float64 -> float32) on first use only"""
    k = (str(dev),) + key
    if k not in _TABLES:
        _TABLES[k] = torch.from_numpy(np.ascontiguousarray(make(), dtype=np.float32)).to(dev)
    return _TABLES[k]


def _basis_table(dev, n_fft, win_length, n_pad):
    return _table(dev, ("basis", n_fft, win_length, n_pad), lambda: _dft_basis(n_fft, win_length, n_pad))


def _mel_table(dev, sr, n_fft, n_mels, fmin, fmax):
    """(n_bins, n_mels): the filterbank transposed, as srn_logmel reads it"""
    return _table(dev, ("mel", sr, n_fft, n_mels, fmin, fmax), lambda: _slaney_mel(sr, n_fft, n_mels, fmin, fmax).T)


def _a_weight_table(dev, sr, n_bins):
    return _table(dev, ("a_weight", sr, n_bins), lambda: _a_weight_db(np.linspace(0.0, sr / 2.0, n_bins)))


# ---------------------------------------------------------------------------------------------- STFT plan
class _Stft:
    """reflect pad + strided implicit-GEMM STFT of (B, n) signals -> self.spec (B, frames, ld) = [re | im | 0]"""

    def __init__(self, dev, B, n, n_fft, hop, win_length, pad_mode="reflect", lens=None, audio=None):
        """lens: per-item sample counts (CUDA int32) -- each item is padded at its own end (srn_pad_ragged mirrors
        there, srn_pad_ragged_zero puts zeros); audio: a (B, n) buffer of the caller's to read the signal from, instead
        of one of the plan's own"""
        if pad_mode not in ("reflect", "constant"):
            raise ValueError(f"pad_mode {pad_mode!r}: 'reflect' or 'constant'")
        c = math.gcd(math.gcd(n_fft, hop), 16)
        if c < 4:
            raise ValueError(f"fft_size {n_fft} and hop_size {hop} must share a factor of 4 (rows of the signal view)")
        self.B, self.n, self.nb = B, n, 1 + n_fft // 2
        self.frames = 1 + n // hop
        pad = n_fft // 2
        rows = -(-(n + 2 * pad) // c) + n_fft // c + 2  # the last frame's taps stay inside the buffer
        self.ld_sig = rows * c
        self.ld = rup(2 * self.nb, 4)
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        self.audio = f(B, n) if audio is None else audio
        self.sig, self.spec = f(B, self.ld_sig), f(B, self.frames, self.ld)
        self.basis = _basis_table(dev, n_fft, win_length, self.ld)
        if lens is None:
            self.ops = [ops.CallOp("srn_pad_signal", (self.audio, self.sig, B, n, pad, self.ld_sig,
                                                      int(pad_mode == "constant")))]
        else:
            entry = "srn_pad_ragged" if pad_mode == "reflect" else "srn_pad_ragged_zero"
            self.ops = [ops.CallOp(entry, (self.audio, n, lens, self.sig, B, n, pad, self.ld_sig))]
        # A frame is a contraction over n_fft samples = taps of `cw` samples each.  The signal is viewed as rows that START
        # every c samples (row stride c, so any frame start is a row) but are cw = 32 samples WIDE (overlapping rows are
        # fine for a read-only operand): 32-channel taps take the fast contraction kernel, 16-wide ones the generic one
        # (loudness, n_fft 2048: 5.6 -> 0.9 ms per 8 x 1024 frames).
        cw = 32 if (c == 16 and n_fft % 32 == 0) else c
        step = cw // c
        taps_all = n_fft // cw
        for g0 in range(0, taps_all, _lib.SRN_MAX_TAPS):
            taps = [step * j for j in range(g0, min(g0 + _lib.SRN_MAX_TAPS, taps_all))]
            more = dict(res=self.spec, res_mode=ops.RES_ADD, res_bs=self.frames * self.ld, ld_res=self.ld) if g0 else {}
            self.ops.append(ops.ConvOp(in0=self.sig, w=(self.basis, g0 * cw), out=self.spec, n_batch=B, T_in=rows - step,
                                       T_out=self.frames, C_in=cw, N=self.ld, in0_bs=self.ld_sig, ld_in0=c, ldw=n_fft,
                                       out_bs=self.frames * self.ld, ld_out=self.ld, taps=taps, in_stride=hop // c,
                                       precision=_lib.PREC_FP32, **more))

    def load(self, audio):
        self.audio.copy_(audio.reshape(self.B, self.n), non_blocking=True)


def _as_batch(audio):
    if not isinstance(audio, torch.Tensor):  # numpy input, as the reference's callers pass: uploaded
        if not torch.cuda.is_available():
            raise RuntimeError("serenade_amd.features needs a CUDA (ROCm) device; there is no CPU fallback")
        audio = torch.as_tensor(np.asarray(audio, dtype=np.float32)).cuda()
    _require_cuda(audio, "serenade_amd.features")
    a = audio.detach().to(torch.float32)
    return (a.unsqueeze(0), True) if a.dim() == 1 else (a, False)


def _item_frames(lengths, B, n, hop, what, reflect_pad=None):
    """the checked per-item sample counts of a padded (B, n) batch and their frame counts 1 + n_b // hop.
    reflect_pad: the reflect padding each item must be longer than (numpy.pad's own condition, srn_pad_signal's check
    for the dense call)."""
    lens = item_lengths(lengths, B, n, what)
    if reflect_pad is not None:
        for b, v in enumerate(lens):
            if v <= reflect_pad:
                raise ValueError(f"{what}: item {b} has {v} samples, reflect padding of {reflect_pad} needs more")
    return lens, [1 + v // hop for v in lens]


class _Ragged:
    """what a plan with per-item lengths adds: `counts` (2, B) device int32 = [samples | frames], refilled by every
    call (the plan depends on (B, n) only, not on the lengths)"""

    def __init__(self, dev, B):
        self.counts = torch.zeros(2, B, device=dev, dtype=torch.int32)
        self.samples, self.frames = self.counts[0], self.counts[1]

    def load(self, lens, frames):
        self.counts.copy_(torch.tensor([lens, frames], dtype=torch.int32))


def _run(plan, a, lens, frames, single):
    st, rg, out, ol = plan
    st.load(a)
    if rg is not None:
        rg.load(lens, frames)
    for op in ol:
        op()
    res = out.clone()
    res = res[0] if single else res
    return res if rg is None else (res, frames)


def logmelfilterbank(audio, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80,
                     fmin=None, fmax=None, eps=1e-10, log_base=10.0, lengths=None):
    """preprocess.py:140-203: (#frames, num_mels) log-mel spectrogram (leading batch axis for (B, n) input).

    lengths: the sample counts n_b of a padded (B, n) batch, each in (fft_size // 2, n].  The result is then
    ((B, 1 + n // hop_size, num_mels), [1 + n_b // hop_size]): item b's own frames are what its B = 1 call on
    audio[b, :n_b] computes, up to the fp32 summation order of the STFT (audio[b, n_b:] is never read), the frames
    past them are 0."""
    if window != "hann":
        raise ValueError("only the recipe's Hann window is implemented")
    if log_base not in (None, 10.0, 2.0):
        raise ValueError(f"{log_base} is not supported.")
    a, single = _as_batch(audio)
    B, n = a.shape
    win_length = fft_size if win_length is None else win_length
    fmin = 0 if fmin is None else fmin
    fmax = sampling_rate / 2 if fmax is None else fmax
    key = ("mel", str(a.device), B, n, sampling_rate, fft_size, hop_size, win_length, num_mels, fmin, fmax, eps, log_base)
    lens = frames = None
    if lengths is not None:
        lens, frames = _item_frames(lengths, B, n, hop_size, "logmelfilterbank", reflect_pad=fft_size // 2)
        key += ("ragged",)

    def make():
        rg = None if lengths is None else _Ragged(a.device, B)
        st = _Stft(a.device, B, n, fft_size, hop_size, win_length, lens=None if rg is None else rg.samples)
        mel_t = _mel_table(a.device, sampling_rate, fft_size, num_mels, fmin, fmax)
        out = torch.zeros(B, st.frames, num_mels, device=a.device, dtype=torch.float32)
        mode = 0 if log_base is None else int(log_base)
        if rg is None:
            op = ops.CallOp("srn_logmel", (st.spec, mel_t, out, B * st.frames, st.nb, st.ld, num_mels, float(eps),
                                           mode))
        else:
            op = ops.CallOp("srn_logmel_ragged", (st.spec, mel_t, rg.frames, out, B, st.frames, st.nb, st.ld, num_mels,
                                                  float(eps), mode))
        return st, rg, out, st.ops + [op]

    return _run(lru_get(_PLANS, key, 8, make), a, lens, frames, single)


def loudness_extract(audio, sampling_rate, hop_length, pad_mode="constant", lengths=None):
    """preprocess.py:126-137: (#frames,) log mean A-weighted amplitude (librosa defaults: n_fft 2048, Hann,
    power_to_db top_db 80 relative to the utterance's loudest bin).

    pad_mode: the reference calls `librosa.stft(audio, hop_length=hop_length)` without a pad_mode, so the edge frames
    depend on the installed librosa: "constant" (zeros) since librosa 0.10 -- the default here --, "reflect" before
    (setup.cfg only asks for librosa >= 0.8.0).  Use the mode the `lft` features of a checkpoint were extracted with;
    about n_fft / 2 / hop frames at each end of an utterance differ between the two.

    lengths: the sample counts n_b of a padded (B, n) batch, each in [1, n] ((1024, n] with pad_mode "reflect").  The
    result is then ((B, 1 + n // hop_length), [1 + n_b // hop_length]): item b's own frames are what its B = 1 call
    on audio[b, :n_b] computes, up to the fp32 summation order of the STFT -- the top_db floor is relative to the
    item's own loudest bin, audio[b, n_b:] is never read --, the frames past them are 0."""
    n_fft = 2048
    if pad_mode not in ("reflect", "constant"):
        raise ValueError(f"pad_mode {pad_mode!r}: 'reflect' or 'constant'")
    a, single = _as_batch(audio)
    B, n = a.shape
    key = ("loud", str(a.device), B, n, sampling_rate, hop_length, pad_mode)
    lens = frames = None
    if lengths is not None:
        lens, frames = _item_frames(lengths, B, n, hop_length, "loudness_extract",
                                    reflect_pad=n_fft // 2 if pad_mode == "reflect" else None)
        key += ("ragged",)

    def make():
        rg = None if lengths is None else _Ragged(a.device, B)
        st = _Stft(a.device, B, n, n_fft, hop_length, n_fft, pad_mode, lens=None if rg is None else rg.samples)
        aw = _a_weight_table(a.device, sampling_rate, st.nb)
        ws = torch.zeros(B, device=a.device, dtype=torch.int32)
        out = torch.zeros(B, st.frames, device=a.device, dtype=torch.float32)
        if rg is None:
            op = ops.CallOp("srn_loudness", (st.spec, aw, ws, out, B, st.frames, st.nb, st.ld, 1e-10, 80.0, 1e-5))
        else:
            op = ops.CallOp("srn_loudness_ragged", (st.spec, aw, rg.frames, ws, out, B, st.frames, st.nb, st.ld, 1e-10,
                                                    80.0, 1e-5))
        return st, rg, out, st.ops + [op]  # (the op pins ws)

    return _run(lru_get(_PLANS, key, 8, make), a, lens, frames, single)
