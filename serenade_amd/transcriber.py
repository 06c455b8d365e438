"""Phoneme-informed MIDI note transcriber on the GPU: the `est_lf0_score` track of a dump (the F0 input of
Serenade.inference), computed by the reference in serenade/bin/preprocess.py:374-383,506-528 with TranscriptionModel
(serenade/modules/phoneme_midi/model.py, phonerec_model.py, subnetworks.py, feature.py), one utterance at a time, then
FramewiseDecoder (decoding.py) on the host.

    TranscriptionModel(config)          the checkpoint's ckpt["config"]; DEFAULT_CONFIG is an assumed geometry
      .load_state_dict(sd)              ckpt["model_state_dict"] keys; BN folded, W_hh transposed, feat_ext buffers
                                        ignored (a mel_basis of the right shape among them is used)
      .forward(wave16k, lengths)        (B, T, 3) onset / offset / activation logits of every item on its own
      .frames(n_samples)                T = 1 + n // hop_length
    FramewiseDecoder(config).decode(logits_item, f0)      decoding.py, on the host
      .decode_batch(logits, frames, f0, f0_frames)        the same for a ragged batch in one launch on the GPU
                                                          (srn_note_decode): (counts, intervals, pitches) tensors
    reference_f0(wave16k, lengths, config)                decoding.py:36-45's librosa.pyin call, on the GPU
                                                          (pitch.pyin): one f0 contour per item for decode(f0=...)
    reference_f0_device(wave16k, lengths, config)         the same contours left on the GPU for decode_batch
    estimate_score(pitches, intervals, n_samples, ...)    preprocess.py:510-528: (midi frames, est_lf0_score)
    estimate_score_batch(counts, intervals, pitches, ...) the same for a ragged batch on the GPU (srn_note_frames)

The network, per item (B = 1, eval mode):
    pitch = DilatedConvStack(dB-mel(x)) -> BiLSTM                          (pitch_conv_stack, pitch_rnn)
    phon  = Linear(BiLSTM(ConvStack(dB-mel'(x))), 39)                       (lang_model: raw logits, no softmax)
    lang  = DilatedConvStack(phon) -> BiLSTM                                (lang_conv_stack, lang_rnn)
    out   = Linear(BiLSTM(cat(pitch, lang)), 3)                             (combined_rnn, combined_fc)
A conv stack is conv3x3 + BN + ReLU, conv3x3 + BN + ReLU, MaxPool(1, 2), conv3x3 + BN + ReLU, MaxPool(1, 2), flatten
(channel-major) and Linear; the dilated form has time dilation 2 in its first conv.  BiLSTM.forward's 512-frame chunks
with carried (h, c) equal one unchunked bidirectional pass, which is what runs here.

Every item of a padded batch gets exactly what its own B = 1 call gets (`lengths`): the STFT reflects at the item's own
end, the top_db clamp of AmplitudeToDB takes the item's own maximum over its valid frames (torchaudio would take one
maximum over a whole (B, F, T) batch), the convs read frames past the item's length as zero and the reverse LSTM starts
at the item's last frame.

Arithmetic is exact fp32, all of it in libserenade_hip.so: the ragged reflect pad (srn_pad_ragged), the STFT, conv
layers 1-2, the flatten + Linear layers and the LSTM input projections (srn_conv_gemm), the mel power + dB + per-item
clamp (srn_mel_db), layer 0 (srn_trans_conv0), the pooling (srn_trans_pool) and the LSTM recurrence (srn_bilstm_recur).
Plans are cached per (B, samples, lengths) and replayed through ops.GraphRunner; no torch arithmetic runs inside a plan
and there is no CPU path.

Parity: the network from the dB-mel image onward is pinned to the reference's own modules
(tests/golden/transcriber_small.npz); nnAudio and torchaudio are not installed, so the front-end is pinned to float64
restatements of them only ("parity unpinned", like the log-mel row).
"""
import copy

import numpy as np
import torch

from . import _lib, ops, pitch
from .features import _slaney_mel, _Stft
from .ops import ConvOp, GraphRunner
from .plan import check_state, dev_i32, linear_op, lru_get, rup, wave_batch

__all__ = ["TranscriptionModel", "FramewiseDecoder", "estimate_score", "estimate_score_batch", "reference_f0",
           "reference_f0_device", "DEFAULT_CONFIG", "NOTE_MAX_FRAMES"]

# ASSUMED geometry: no transcriber checkpoint is available to read ckpt["config"] from.  The front-end follows the
# reference's 16 kHz input (preprocess.py:495,506); model_complexity 48 (model_size 768, LSTM hidden 384) and the
# decoder settings are assumptions.  Pass the checkpoint's own config for real use.
_FRONT = dict(sample_rate=16000, win_length=1024, hop_length=320, n_mels=128, fmin=30, fmax=8000)
DEFAULT_CONFIG = dict(
    _FRONT, model_complexity=48, pitch_sum="weighted_median", onset_threshold=0.5, offset_threshold=0.5,
    lang_model_config=dict(_FRONT, model_complexity=48, num_lbl=40),
)
N_PHONEMES = 39  # PhonemeRecognitionModel.output_features
NOTE_MAX_FRAMES = 8192  # SRN_NOTE_MAX_FRAMES of serenade_hip.h: frames per item of decode_batch
PITCH_SUM = {"median": 0, "weighted_mean": 1, "weighted_median": 2}  # srn_note_decode's pitch_sum
TOP_DB, AMIN, BN_EPS = 80.0, 1e-10, 1e-5
_CONVS = ((0, 1), (3, 4), (8, 9))  # (conv, BatchNorm) indices inside a stack's nn.Sequential


def _stack_shapes(pre, F, m):
    c0, c2 = m // 16, m // 8
    sh = {}
    for (ci, bi), (co, cin) in zip(_CONVS, ((c0, 1), (c0, c0), (c2, c0))):
        sh[f"{pre}cnn.{ci}.weight"], sh[f"{pre}cnn.{ci}.bias"] = (co, cin, 3, 3), (co,)
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{pre}cnn.{bi}.{k}"] = (co,)
    sh[f"{pre}fc.0.weight"], sh[f"{pre}fc.0.bias"] = (m, c2 * (F // 4)), (m,)
    return sh


def _lstm_shapes(pre, I, H):
    sh = {}
    for sfx in ("", "_reverse"):
        sh.update({f"{pre}rnn.weight_ih_l0{sfx}": (4 * H, I), f"{pre}rnn.weight_hh_l0{sfx}": (4 * H, H),
                   f"{pre}rnn.bias_ih_l0{sfx}": (4 * H,), f"{pre}rnn.bias_hh_l0{sfx}": (4 * H,)})
    return sh


def fold_bn(w, b, gamma, beta, mean, var, eps=BN_EPS):
    """Conv2d + BatchNorm2d (running statistics) -> one conv, in float64: w' = w s, b' = (b - mean) s + beta with
    s = gamma / sqrt(var + eps)"""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s.view(-1, 1, 1, 1), (b.double() - mean.double()) * s + beta.double()


def lstm_w_hh_t(w_hh, w_hh_rev):
    """(4H, H) W_hh of both directions -> (2, H, H, 4) [d][k][j][gate], srn_bilstm_recur's layout"""
    H = w_hh.shape[1]
    return torch.stack([w.reshape(4, H, H).permute(2, 1, 0) for w in (w_hh, w_hh_rev)]).contiguous()


class TranscriptionModel:
    """TranscriptionModel.eval() (pitch + phoneme branches, three BiLSTMs) with exact ragged batching on the GPU."""

    def __init__(self, config=None, device="cuda"):
        cfg = copy.deepcopy(DEFAULT_CONFIG if config is None else dict(config))
        lc = cfg["lang_model_config"]
        for c, what in ((cfg, "config"), (lc, "lang_model_config")):
            missing = [k for k in ("sample_rate", "win_length", "hop_length", "n_mels", "fmin", "fmax",
                                   "model_complexity") if k not in c]
            if missing:
                raise KeyError(f"TranscriptionModel: {what} lacks {missing}")
        if int(lc.get("num_lbl", N_PHONEMES + 1)) != N_PHONEMES + 1:
            raise ValueError(f"TranscriptionModel: lang_model_config num_lbl must be {N_PHONEMES + 1}")
        if cfg["hop_length"] != lc["hop_length"]:
            raise ValueError("TranscriptionModel: both front-ends need the same hop_length (their frames are concatenated)")
        self.m, self.m_lang = 16 * int(cfg["model_complexity"]), 16 * int(lc["model_complexity"])
        for m in (self.m, self.m_lang):
            if not (32 <= m // 2 <= 512 and (m // 2) % 8 == 0):
                raise ValueError(f"TranscriptionModel: LSTM hidden size {m // 2} must be a multiple of 8 in [32, 512]")
        for c in (cfg, lc):
            if c["n_mels"] < 4 or c["win_length"] < 2:
                raise ValueError("TranscriptionModel: n_mels >= 4 and win_length >= 2 needed")
        self.config = cfg
        self.device = torch.device(device)
        self.w = None
        self._plans = {}

    # ------------------------------------------------------------------------------------------------ weights
    def state_shapes(self):
        """{network state-dict key: shape} of this geometry (feature-extractor buffers and num_batches_tracked excluded)"""
        c, lc = self.config, self.config["lang_model_config"]
        m, ml = self.m, self.m_lang
        sh = {}
        sh.update(_stack_shapes("lang_model.conv_stack.", lc["n_mels"], ml))
        sh.update(_lstm_shapes("lang_model.rnn.", ml, ml // 2))
        sh["lang_model.fc.weight"], sh["lang_model.fc.bias"] = (N_PHONEMES, ml), (N_PHONEMES,)
        sh.update(_stack_shapes("pitch_conv_stack.", c["n_mels"], m))
        sh.update(_stack_shapes("lang_conv_stack.", N_PHONEMES, m))
        sh.update(_lstm_shapes("pitch_rnn.", m, m // 2))
        sh.update(_lstm_shapes("lang_rnn.", m, m // 2))
        sh.update(_lstm_shapes("combined_rnn.", 2 * m, m // 2))
        sh["combined_fc.weight"], sh["combined_fc.bias"] = (3, m), (3,)
        return sh

    @staticmethod
    def _ignored(k):
        return "feat_ext." in k or k.endswith("num_batches_tracked")

    def mel_matrix(self, which, sd=None):
        """(n_mels, n_fft // 2 + 1) float64 mel matrix of front-end `which` ("pitch" or "lang"): the checkpoint's
        nnAudio mel_basis when `sd` holds one of the right shape, else the Slaney filterbank built from the config"""
        c = self.config if which == "pitch" else self.config["lang_model_config"]
        key = "pitch_feat_ext.feat.mel_basis" if which == "pitch" else "lang_model.feat_ext.feat.mel_basis"
        shape = (c["n_mels"], c["win_length"] // 2 + 1)
        if sd is not None and key in sd and tuple(sd[key].shape) == shape:
            return torch.as_tensor(sd[key]).detach().cpu().double().numpy()
        return _slaney_mel(c["sample_rate"], c["win_length"], c["n_mels"], c["fmin"], c["fmax"])

    def _pack_stack(self, s, pre, F, m, d):
        c0, c2 = m // 16, m // 8
        p0, p2 = rup(c0, 4), rup(c2, 4)
        convs = []
        for (ci, bi), (co, cin, cop, cip) in zip(_CONVS, ((c0, 1, p0, 1), (c0, c0, p0, p0), (c2, c0, p2, p0))):
            bn = [s[f"{pre}cnn.{bi}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")]
            w, b = fold_bn(s[f"{pre}cnn.{ci}.weight"], s[f"{pre}cnn.{ci}.bias"], *bn)
            bp = torch.zeros(cop, dtype=torch.float64)
            bp[:co] = b
            if ci == 0:
                wp = torch.zeros(cop, 9, dtype=torch.float64)
                wp[:co] = w.reshape(co, 9)
            else:  # [N_pad][9 taps][C_in_pad], taps in (dt, df) order, zero rows / columns in the padding
                wp = torch.zeros(cop, 9, cip, dtype=torch.float64)
                wp[:co, :, :cin] = w.reshape(co, cin, 9).permute(0, 2, 1)
                wp = wp.reshape(cop, 9 * cip)
            convs.append((d(wp), d(bp)))
        K = c2 * (F // 4)
        fw = torch.zeros(m, rup(K, 4))
        fw[:, :K] = s[f"{pre}fc.0.weight"]
        return {"convs": convs, "fc_w": d(fw), "fc_b": d(s[f"{pre}fc.0.bias"]), "F": F, "m": m, "c2": c2}

    @staticmethod
    def _pack_lstm(s, pre, d):
        r = pre + "rnn."
        w_ih = torch.cat([s[r + "weight_ih_l0"], s[r + "weight_ih_l0_reverse"]])
        b = torch.cat([s[r + "bias_ih_l0"].double() + s[r + "bias_hh_l0"].double(),
                       s[r + "bias_ih_l0_reverse"].double() + s[r + "bias_hh_l0_reverse"].double()])
        H = s[r + "weight_hh_l0"].shape[1]
        return {"w_ih": d(w_ih), "b": d(b), "w_hh_t": d(lstm_w_hh_t(s[r + "weight_hh_l0"], s[r + "weight_hh_l0_reverse"])),
                "H": H, "I": w_ih.shape[1]}

    def load_state_dict(self, sd):
        s = {k: torch.as_tensor(v).detach().cpu() for k, v in sd.items()}
        want = self.state_shapes()
        check_state("TranscriptionModel.load_state_dict", s, want, ignored=[k for k in s if self._ignored(k)])
        c, lc = self.config, self.config["lang_model_config"]
        dev = self.device
        d = lambda t: t.to(dev, torch.float32).contiguous()
        w = {"phon_stack": self._pack_stack(s, "lang_model.conv_stack.", lc["n_mels"], self.m_lang, d),
             "phon_rnn": self._pack_lstm(s, "lang_model.rnn.", d),
             "pitch_stack": self._pack_stack(s, "pitch_conv_stack.", c["n_mels"], self.m, d),
             "lang_stack": self._pack_stack(s, "lang_conv_stack.", N_PHONEMES, self.m, d),
             "pitch_rnn": self._pack_lstm(s, "pitch_rnn.", d), "lang_rnn": self._pack_lstm(s, "lang_rnn.", d),
             "comb_rnn": self._pack_lstm(s, "combined_rnn.", d)}
        pw = torch.zeros(N_PHONEMES + 1, self.m_lang)  # 40 output columns: column 39 is a zero row of the weight
        pb = torch.zeros(N_PHONEMES + 1)
        pw[:N_PHONEMES], pb[:N_PHONEMES] = s["lang_model.fc.weight"], s["lang_model.fc.bias"]
        w["phon_fc"] = (d(pw), d(pb))
        cw, cb = torch.zeros(4, self.m), torch.zeros(4)
        cw[:3], cb[:3] = s["combined_fc.weight"], s["combined_fc.bias"]
        w["comb_fc"] = (d(cw), d(cb))
        w["mel_pitch"] = d(torch.from_numpy(self.mel_matrix("pitch", s).T.copy()))
        w["mel_lang"] = d(torch.from_numpy(self.mel_matrix("lang", s).T.copy()))
        self.w = w
        self._plans = {}
        return self

    # ------------------------------------------------------------------------------------------------ geometry
    def frames(self, n_samples):
        """frames of an utterance of n_samples (16 kHz): nnAudio's 1 + n // hop_length (center=True)"""
        return 1 + int(n_samples) // int(self.config["hop_length"])

    # ------------------------------------------------------------------------------------------------ inference
    def forward(self, wave16k, lengths=None, with_phonemes=False):
        """wave16k: (n,), (B, n) or (B, 1, n) CUDA float32 at 16 kHz (numpy is uploaded).  Returns the logits (B, T, 3)
        (onset, offset, activation) and the per-item frame counts; with_phonemes=True also the phoneme model's raw
        logits (B, T, 39).  Frames at or past an item's count are padding (unspecified values)."""
        if self.w is None:
            raise RuntimeError("TranscriptionModel: load_state_dict first")
        a, lens = wave_batch(wave16k, lengths, self.device, "TranscriptionModel", allow_channel_dim=True)
        B, n = a.shape
        pad = max(self.config["win_length"], self.config["lang_model_config"]["win_length"]) // 2
        if min(lens) <= pad:
            raise ValueError(f"TranscriptionModel: an utterance of {min(lens)} samples is too short for the reflect "
                             f"padding of {pad}")
        key = (str(a.device), B, n, tuple(lens))
        plan = lru_get(self._plans, key, 8, lambda: _Plan(self, a.device, B, n, lens))
        plan.wave.copy_(a, non_blocking=True)
        plan.run()
        T = [self.frames(v) for v in lens]
        out = plan.logits[..., :3].clone()
        if with_phonemes:
            return out, T, plan.phon[..., :N_PHONEMES].clone()
        return out, T

    __call__ = forward


class _Plan:
    """buffers + op list of one (B, n, lengths)"""

    def __init__(self, m, dev, B, n, lens):
        c, lc, w = m.config, m.config["lang_model_config"], m.w
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        i32 = lambda v: torch.tensor(v, device=dev, dtype=torch.int32)
        T = m.frames(n)
        tl = [m.frames(v) for v in lens]
        self.T, self.B = T, B
        self.lens = i32(tl)
        self.wave = f(B, n)
        self._lens_cache = {}
        ol = []
        # ---- front-ends: one STFT per distinct (n_fft, hop), then mel power -> dB -> per-item top_db clamp
        samples = i32(lens)
        stfts = {}
        imgs = {}
        gmax = torch.zeros(B, device=dev, dtype=torch.int32)
        for which, cc, mel_t in (("pitch", c, w["mel_pitch"]), ("lang", lc, w["mel_lang"])):
            sk = (cc["win_length"], cc["hop_length"])
            if sk not in stfts:
                st = _Stft(dev, B, n, cc["win_length"], cc["hop_length"], cc["win_length"], lens=samples,
                           audio=self.wave)
                ol.extend(st.ops)
                stfts[sk] = st
            st = stfts[sk]
            assert st.frames == T
            img = f(B, T, cc["n_mels"])
            ol.append(ops.CallOp("srn_mel_db", (st.spec, st.ld, st.nb, mel_t, self.lens, gmax, img, cc["n_mels"], B, T,
                                                cc["n_mels"], AMIN, TOP_DB)))
            imgs[which] = img
        # ---- phoneme model: ConvStack -> BiLSTM -> Linear(39) (40 columns, the last one zero)
        x, _ = self._stack(ol, f, imgs["lang"], lc["n_mels"], lc["n_mels"], w["phon_stack"], 1)
        h = f(B, T, m.m_lang)
        self._bilstm(ol, f, x, w["phon_rnn"], h, 0, m.m_lang)
        self.phon = f(B, T, N_PHONEMES + 1)
        ol.append(linear_op(h, B * T, m.m_lang, *w["phon_fc"], self.phon, N_PHONEMES + 1, precision=_lib.PREC_FP32))
        # ---- lang and pitch branches into the two halves of the combined BiLSTM's input
        cat = f(B, T, 2 * m.m)
        x, _ = self._stack(ol, f, self.phon, N_PHONEMES + 1, N_PHONEMES, w["lang_stack"], 2)
        self._bilstm(ol, f, x, w["lang_rnn"], cat, m.m, 2 * m.m)
        x, _ = self._stack(ol, f, imgs["pitch"], c["n_mels"], c["n_mels"], w["pitch_stack"], 2)
        self._bilstm(ol, f, x, w["pitch_rnn"], cat, 0, 2 * m.m)
        comb = f(B, T, m.m)
        self._bilstm(ol, f, cat, w["comb_rnn"], comb, 0, m.m)
        self.logits = f(B, T, 4)
        ol.append(linear_op(comb, B * T, m.m, *w["comb_fc"], self.logits, 4, precision=_lib.PREC_FP32))
        self.ops = ol
        self.runner = GraphRunner(lambda: self.ops)

    def _lens_times(self, k):
        if k not in self._lens_cache:
            self._lens_cache[k] = (self.lens * k).contiguous()
        return self._lens_cache[k]

    def _conv3x3(self, inp, wb, out, F, cin, cout):
        """3x3 conv (padding 1) + folded BN + ReLU on a bordered channels-last image (B, T, F + 2, cin): the rows of an
        item are (t, column) pairs, so the 9 taps are row offsets dt (F + 2) + df and the zero border columns supply the
        frequency padding; rows at or past len (F + 2) read as zero (the time padding)."""
        B, T, Wd = self.B, self.T, F + 2
        taps = [dt * Wd + df for dt in (-1, 0, 1) for df in (-1, 0, 1)]
        return ConvOp(in0=inp, w=wb[0], out=out, n_batch=B, T_in=T * Wd, T_out=T * Wd, C_in=cin, N=cout,
                      in0_bs=T * Wd * cin, ld_in0=cin, ldw=9 * cin, out_bs=T * Wd * cout, ld_out=cout, taps=taps,
                      bias=wb[1], len_in=self._lens_times(Wd), post=_lib.POST_RELU, precision=_lib.PREC_FP32)

    def _stack(self, ol, f, img, ld_img, F, sw, dil):
        """(Dilated)ConvStack on img (B, T, ld_img) with F valid columns -> (B, T, m)"""
        B, T = self.B, self.T
        (w0, b0), c1, c2w = sw["convs"]
        p0, p2 = w0.shape[0], c2w[0].shape[0]
        F2, F4 = F // 2, F // 4
        a0, a1 = f(B, T, F + 2, p0), f(B, T, F + 2, p0)
        q1, a2 = f(B, T, F2 + 2, p0), f(B, T, F2 + 2, p2)
        K = sw["c2"] * F4
        flat = f(B, T, rup(K, 4))
        out = f(B, T, sw["m"])
        ol.append(ops.CallOp("srn_trans_conv0", (img, T * ld_img, ld_img, self.lens, w0, b0, a0, B, T, F, p0, dil)))
        ol.append(self._conv3x3(a0, c1, a1, F, p0, p0))
        ol.append(ops.CallOp("srn_trans_pool", (a1, self.lens, q1, B, T, F, p0, p0, 0, 0)))
        ol.append(self._conv3x3(q1, c2w, a2, F2, p0, p2))
        ol.append(ops.CallOp("srn_trans_pool", (a2, self.lens, flat, B, T, F2, p2, sw["c2"], 1, rup(K, 4))))
        ol.append(linear_op(flat, B * T, rup(K, 4), sw["fc_w"], sw["fc_b"], out, sw["m"], precision=_lib.PREC_FP32))
        return out, sw["m"]

    def _bilstm(self, ol, f, x, lw, out, col0, ld_out):
        """BiLSTM(x) -> out[:, :, col0 : col0 + 2H] (row length ld_out)"""
        B, T, H, I = self.B, self.T, lw["H"], lw["I"]
        g = f(B, T, 8 * H)
        ol.append(linear_op(x, B * T, I, lw["w_ih"], lw["b"], g, 8 * H, precision=_lib.PREC_FP32))
        ol.append(ops.CallOp("srn_bilstm_recur", (g, T * 8 * H, 8 * H, self.lens, lw["w_hh_t"], (out, col0), T * ld_out,
                                                  ld_out, B, T, H)))

    def run(self):
        self.runner()


# ---------------------------------------------------------------------------------------------- host decoding
def _hz_to_midi(f):
    """librosa.hz_to_midi"""
    return 12 * (np.log2(np.asanyarray(f)) - np.log2(440.0)) + 69


def _midi_to_hz_librosa(notes):
    """librosa.midi_to_hz"""
    return 440.0 * (2.0 ** ((np.asanyarray(notes) - 69.0) / 12.0))


def weighted_median(data, weights):
    """wquantiles.median of 1-D data: the weighted 0.5-quantile by linear interpolation of the sorted data over the
    centred cumulative weights (S_n - w_n / 2) / S_N"""
    data, weights = np.asarray(data), np.asarray(weights)
    order = np.argsort(data)
    d, wt = data[order], weights[order]
    cum = np.cumsum(wt)
    return np.interp(0.5, (cum - 0.5 * wt) / cum[-1], d)


def _peaks(p, threshold):
    """decoding.py's peak picking on one activation curve: inside each run above the threshold the first strict
    maximum is kept; the index 0 doubles as "no run open", so a peak at frame 0 is never emitted (and a later run whose
    values do not exceed p[0] keeps pointing at it), and a run still open at the end is dropped"""
    out = torch.zeros_like(p)
    v = p.numpy()
    best = 0
    for i in range(len(v)):
        if v[i] > threshold:
            if v[i] > v[best]:
                best = i
        elif best != 0:
            out[best] = p[best]
            best = 0
    return out


def _rises(x):
    """1.0 where x rose against the previous frame (the first frame compares against 0)"""
    return (torch.cat([x[:1], x[1:] - x[:-1]]) > 0).float()


class FramewiseDecoder:
    """decoding.py's FramewiseDecoder on the host: sigmoid, peak picking of onsets / offsets, note segmentation and one
    pitch per note from the f0 contour (`pitch_sum`: median, weighted_mean or weighted_median)."""

    def __init__(self, config):
        self.sr, self.win_length, self.hop_length = config["sample_rate"], config["win_length"], config["hop_length"]
        self.onset_threshold, self.offset_threshold = config["onset_threshold"], config["offset_threshold"]
        self.pitch_sum = config["pitch_sum"]
        if self.pitch_sum not in ("median", "weighted_mean", "weighted_median"):
            raise ValueError(f"FramewiseDecoder: pitch_sum {self.pitch_sum!r}")

    def pyin(self, audio):
        """the reference's f0: librosa.pyin(fmin 65, fmax 2093, frame = win_length, hop = hop_length, NaN unvoiced)"""
        try:
            import librosa
        except ImportError as e:
            raise RuntimeError("FramewiseDecoder: f0 not given and librosa is not installed (pass the pyin contour)") from e
        a = audio.detach().cpu().numpy() if isinstance(audio, torch.Tensor) else np.asarray(audio)
        f0, _, _ = librosa.pyin(a, fmin=65, fmax=2093, sr=self.sr, frame_length=self.win_length,
                                hop_length=self.hop_length, fill_na=np.nan, center=True)
        return f0

    def decode(self, logits, f0=None, audio=None):
        """logits (T, 3) or (1, T, 3) of one item (its valid frames); f0: the pyin contour (Hz, NaN unvoiced), or None to
        run pyin on `audio`.  Returns (pitches, intervals) as the reference does: a list of floats and a list of
        [onset frame, offset frame + 1]."""
        p = torch.as_tensor(logits).detach().to("cpu", torch.float32).reshape(-1, 3)
        act = torch.sigmoid(p)
        on, off, frames = act[:, 0].contiguous(), act[:, 1].contiguous(), act[:, 2].contiguous()
        if f0 is None:
            if audio is None:
                raise ValueError("Either audio or f0 should not be None.")
            f0 = self.pyin(audio)
        f0 = torch.as_tensor(np.asarray(f0.detach().cpu() if isinstance(f0, torch.Tensor) else f0)).float()
        return self._notes(_peaks(on, self.onset_threshold), f0, _peaks(off, self.offset_threshold), frames)

    @torch.no_grad()
    def decode_batch(self, logits, frames, f0, f0_frames):
        """decode() of every item of a ragged batch in one launch (srn_note_decode; notes.hip states the semantics).
        logits (B, Tmax, 3) float32 on the GPU with `frames` valid frames per item, as TranscriptionModel.forward
        returns them; f0 (B, Fmax) float64 on the GPU with `f0_frames` frames per item, as pitch.pyin and
        reference_f0_device return them.  Returns device tensors: counts (B,) int32 notes per item, intervals
        (B, Tmax, 2) int32 [onset frame, offset frame + 1] and pitches (B, Tmax) float64, zeros past an item's count.
        The arithmetic from the contour on is float64 (decode() follows the reference's float32), and the sigmoid is
        the GPU's: decisions agree with decode() wherever no activation lies within an fp32 rounding of a threshold
        or of another activation.  An item may have at most NOTE_MAX_FRAMES frames: ValueError beyond, no truncation."""
        _require_cuda(logits, "decode_batch: logits")
        if not (logits.dtype == torch.float32 and logits.ndim == 3 and logits.shape[2] == 3):
            raise RuntimeError("decode_batch: logits must be a (B, Tmax, 3) float32 tensor")
        if not (isinstance(f0, torch.Tensor) and f0.device == logits.device and f0.dtype == torch.float64
                and f0.ndim == 2 and f0.shape[0] == logits.shape[0]):
            raise RuntimeError("decode_batch: f0 must be a (B, Fmax) float64 tensor on the logits' device")
        B, Tmax, _ = logits.shape
        Fmax = f0.shape[1]
        nt, nf = _counts(frames, B, Tmax, "frames"), _counts(f0_frames, B, Fmax, "f0_frames")
        if B == 0 or Tmax == 0 or Fmax == 0:
            raise ValueError(f"decode_batch: empty batch (logits {tuple(logits.shape)}, f0 {tuple(f0.shape)})")
        if Tmax > NOTE_MAX_FRAMES:
            raise ValueError(f"decode_batch: {Tmax} frames per item exceed the kernel's limit of {NOTE_MAX_FRAMES}")
        dev = logits.device
        e = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device=dev)
        counts, intervals = e(B, dtype=torch.int32), e(B, Tmax, 2, dtype=torch.int32)
        pitches = e(B, Tmax, dtype=torch.float64)
        ops.call("srn_note_decode", logits.contiguous(), dev_i32(nt, dev), f0.contiguous(), dev_i32(nf, dev), B, Tmax,
                 Fmax, float(self.onset_threshold), float(self.offset_threshold), PITCH_SUM[self.pitch_sum],
                 float(np.log2(440.0)), e(B, 5, Tmax, dtype=torch.float32), e(B, 4, Tmax, dtype=torch.float64),
                 e(B, 2, Tmax, dtype=torch.int32), counts, intervals, pitches)
        return counts, intervals, pitches

    def _notes(self, onsets, f0, offsets, frames):
        midi = torch.from_numpy(_hz_to_midi(f0).squeeze())
        on_idx = [int(i) for i in _rises(onsets).nonzero()[:, 0]]
        off_rise = _rises(offsets)
        fq = (frames >= 0.5).float()
        fall = (torch.cat([fq[:-1] - fq[1:], fq[-1:]]) == 1).float()  # last active frame of a run (or of the curve)
        n = onsets.shape[0]
        pitches, intervals = [], []
        for k, onset in enumerate(on_idx):
            nxt = on_idx[k + 1] if k + 1 < len(on_idx) else n - 1
            offset, off_conf, fr_conf = None, 0, 0
            for i in range(onset + 2, nxt):
                if off_rise[i] == 1 and off_conf < offsets[i]:
                    off_conf, offset = offsets[i], i
                if fall[i] == 1:
                    conf, j = 0, i + 1
                    while frames[j] < 0.5 and j < nxt:  # the deepest dip before the frames rise again
                        conf = max(1 - frames[j], conf)
                        j += 1
                    if fr_conf < conf:
                        fr_conf, offset = conf, i
            if offset is None:
                offset = nxt - 1
            seg = midi[onset:offset + 1]
            pitch = self._pitch(seg)
            if pitch != pitch:
                pitch = 0
            if offset > onset:
                pitches.append(pitch)
                intervals.append([onset, offset + 1])
        return pitches, intervals

    def _pitch(self, seg):
        nan = seg.isnan()
        if self.pitch_sum == "median":
            return seg[~nan].median().item()  # torch's lower median
        win = torch.hann_window(seg.shape[0])
        if self.pitch_sum == "weighted_mean":
            ws = seg * win
            keep = ~ws.isnan()
            return (ws[keep].sum() / win[keep].sum()).item()
        win[nan] = 0
        win /= win.sum()
        return weighted_median(seg.cpu().numpy(), win.cpu().numpy())


def reference_f0(wave16k, lengths=None, config=None):
    """the f0 contours FramewiseDecoder.decode(pred, audio=x) computes with librosa (decoding.py:36-45:
    librosa.pyin(audio, fmin=65, fmax=2093, sr, frame_length=win_length, hop_length, fill_na=nan, center=True)), for
    every item of wave16k (B, N) or (N,) on the GPU (pitch.pyin).  A list of numpy float64 contours, one per item over
    its own frames (NaN where unvoiced), each ready for decode(logits, f0=...)."""
    cfg = DEFAULT_CONFIG if config is None else config
    x = wave16k.reshape(1, -1) if wave16k.ndim == 1 else wave16k
    f0, _, _, frames = pitch.pyin(x, lengths, fmin=65, fmax=2093, sr=cfg["sample_rate"],
                                  frame_length=cfg["win_length"], hop_length=cfg["hop_length"], fill_na=np.nan,
                                  center=True)
    f0 = f0.cpu().numpy()
    return [f0[b, :int(n)].copy() for b, n in enumerate(frames)]


def reference_f0_device(wave16k, lengths=None, config=None):
    """reference_f0 without the visit to the host: (f0 (B, T) float64 on the GPU, NaN where unvoiced and past an
    item's frames; frames per item as a list), ready for FramewiseDecoder.decode_batch"""
    cfg = DEFAULT_CONFIG if config is None else config
    x = wave16k.reshape(1, -1) if wave16k.ndim == 1 else wave16k
    f0, _, _, frames = pitch.pyin(x, lengths, fmin=65, fmax=2093, sr=cfg["sample_rate"],
                                  frame_length=cfg["win_length"], hop_length=cfg["hop_length"], fill_na=np.nan,
                                  center=True)
    return f0, [int(n) for n in frames]


def _require_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what} must be a CUDA (ROCm) tensor; there is no CPU path (decode / estimate_score are "
                           "the host forms)")


def _counts(values, B, limit, what):
    """B per-item counts in [0, limit] as a list of ints"""
    v = [int(n) for n in (values.tolist() if hasattr(values, "tolist") else values)]
    if len(v) != B or (B and (min(v) < 0 or max(v) > limit)):
        raise ValueError(f"{what} {v} must give {B} counts in [0, {limit}]")
    return v


def midi_to_frames(midi_values, time_intervals, T, shift_ms=10):
    """preprocess.py midi_to_frames: notes (pitch, [start s, end s]) on a frame grid of shift_ms, ceil(T / shift) frames,
    floor(start / shift) .. ceil(end / shift) (clipped), later notes overwriting earlier ones; int32"""
    shift = shift_ms / 1000.0
    n = int(np.ceil(T / shift))
    out = np.zeros(n, dtype=np.int32)
    for v, (s, e) in zip(midi_values, time_intervals):
        out[int(np.floor(s / shift)):min(int(np.ceil(e / shift)), n)] = v
    return out


def midi_to_log_hz(midi):
    """preprocess.py _midi_to_hz(x, log_f0=True) on the int32 midi frames: log(Hz) where x > 0, else 0.  The result
    keeps the dtype of x (np.zeros_like), so every value is truncated to an integer twice -- Hz, then its log -- as the
    reference does."""
    z = np.zeros_like(midi)
    keep = midi > 0
    z[keep] = _midi_to_hz_librosa(midi[keep])
    z[keep] = np.log(z[keep])
    return z


def estimate_score(pitches, intervals, n_samples, config=None, sampling_rate=24000, shiftms=10):
    """preprocess.py:510-528: the decoded notes of one utterance of n_samples samples at `sampling_rate` (the acoustic
    features' rate, 24 kHz in the recipe) -> (midi (frames,) int32, est_lf0_score (frames, 1)).  Intervals are frames of
    the transcriber (hop_length / sample_rate of `config`); pitches are rounded half to even (Python round)."""
    cfg = DEFAULT_CONFIG if config is None else config
    scale = cfg["hop_length"] / cfg["sample_rate"]
    time = (np.array(intervals) * scale).reshape(-1, 2)
    midi = np.array([round(p) for p in pitches])
    midi = midi_to_frames(midi, time, n_samples / sampling_rate, shift_ms=shiftms)
    return midi, np.expand_dims(midi_to_log_hz(midi), axis=-1)


@torch.no_grad()
def estimate_score_batch(counts, intervals, pitches, n_samples, config=None, sampling_rate=24000, shiftms=10):
    """estimate_score of every item of a ragged batch in one launch (srn_note_frames).  counts (B,) int32, intervals
    (B, cap, 2) int32 and pitches (B, cap) float64 on the GPU, as decode_batch returns them (or any caller-supplied
    notes of that layout); n_samples: samples per item at `sampling_rate`.  Returns (midi (B, Nmax) int32,
    est_lf0_score (B, Nmax) int32, frames per item as a list): item b holds its track in [:frames[b]] and zeros
    behind, bit for bit estimate_score's (the two IEEE operations of every frame index are numpy's, in its order, and
    the log-Hz value per MIDI number is midi_to_log_hz's own).  ValueError when a rounded pitch lies outside 0..127."""
    cfg = DEFAULT_CONFIG if config is None else config
    _require_cuda(counts, "estimate_score_batch: counts")
    if not (counts.dtype == torch.int32 and counts.ndim == 1):
        raise RuntimeError("estimate_score_batch: counts must be a (B,) int32 tensor")
    B, dev = counts.shape[0], counts.device
    if not (intervals.dtype == torch.int32 and intervals.ndim == 3 and intervals.shape[0] == B
            and intervals.shape[2] == 2 and pitches.dtype == torch.float64
            and tuple(pitches.shape) == tuple(intervals.shape[:2]) and intervals.device == dev == pitches.device):
        raise RuntimeError("estimate_score_batch: intervals (B, cap, 2) int32 and pitches (B, cap) float64 on the "
                           "device of counts are needed")
    cap = intervals.shape[1]
    ns = _counts(n_samples, B, 2 ** 31 - 1, "estimate_score_batch: n_samples")
    if B == 0 or cap == 0:
        raise ValueError("estimate_score_batch: empty batch")
    scale, shift = cfg["hop_length"] / cfg["sample_rate"], shiftms / 1000.0
    frames = [int(np.ceil((n / sampling_rate) / shift)) for n in ns]
    Nmax = max(max(frames), 1)
    table = midi_to_log_hz(np.arange(128, dtype=np.int32))
    e = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    midi, lf0, n_frames, bad = e(B, Nmax), e(B, Nmax), e(B), e(1)
    ops.call("srn_note_frames", counts, intervals.contiguous(), pitches.contiguous(), B, cap, dev_i32(ns, dev),
             float(scale), float(shift), float(sampling_rate), dev_i32(table, dev), e(B, cap, 3), midi, lf0, Nmax,
             n_frames, bad)
    if int(bad.item()):
        raise ValueError("estimate_score_batch: a note's rounded pitch lies outside the MIDI numbers 0..127 (or an "
                         "interval is negative)")
    return midi, lf0, frames
