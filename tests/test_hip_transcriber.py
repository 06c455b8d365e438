"""The MIDI note transcriber on the MI355X (serenade_amd/transcriber.py + transcriber.hip): the reduced fixture against
the reference's own modules, DEFAULT_CONFIG geometry against a float64 torch restatement, exact ragged batching, graph
replay, and unit checks of the BiLSTM recurrence, the layer-0 conv and the per-item top_db clamp."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from serenade_amd import ops
from serenade_amd.transcriber import FramewiseDecoder, TranscriptionModel, lstm_w_hh_t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("median", "weighted_mean", "weighted_median")


def _gate(out, ref, what, mx_tol=1e-4, rms_tol=1e-5):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape, what
    m = np.abs(ref).max()
    err = np.abs(out - ref)
    mx, rms = err.max() / m, np.sqrt((err ** 2).mean()) / m
    assert mx <= mx_tol and rms <= rms_tol, f"{what}: max {mx:.2e} rms {rms:.2e} of max|ref|"


@pytest.fixture(scope="module")
def small(golden):
    d = golden("transcriber_small")
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    return TranscriptionModel(cfg, device=DEV).load_state_dict(sd), d, cfg


def _ragged(d):
    n0, n1 = len(d["wave0"]), len(d["wave1"])
    x = torch.full((2, n0), 5.0)  # padding never reaches a valid frame
    x[0] = torch.from_numpy(d["wave0"])
    x[1, :n1] = torch.from_numpy(d["wave1"])
    return x, [n0, n1]


def test_fixture_ragged_batch_against_the_reference(small):
    m, d, _ = small
    x, lens = _ragged(d)
    out, T, phon = m(x.to(DEV).unsqueeze(1), lengths=lens, with_phonemes=True)
    torch.cuda.synchronize()
    assert T == [d["ref0"].shape[0], d["ref1"].shape[0]]
    for i in range(2):
        _gate(out[i, :T[i]].cpu().numpy(), d[f"ref{i}"], f"logits item {i}")
        _gate(phon[i, :T[i]].cpu().numpy(), d[f"phon{i}"], f"phoneme logits item {i}")


def test_decoder_on_device_logits_gives_the_fixture_notes(small):
    m, d, cfg = small
    x, lens = _ragged(d)
    out, T = m(x.to(DEV), lengths=lens)
    torch.cuda.synchronize()
    for mode in MODES:
        dec = FramewiseDecoder(dict(cfg, pitch_sum=mode))
        for i in range(2):
            p, iv = dec.decode(out[i, :T[i]], f0=d[f"f0_{i}"])
            assert np.asarray(iv).reshape(-1, 2).tolist() == d[f"intervals{i}_{mode}"].tolist(), (mode, i)
            assert np.array_equal(np.asarray(p, np.float64), d[f"pitches{i}_{mode}"]), (mode, i)


def test_graph_replay_equals_eager(small):
    m, d, _ = small
    x, lens = _ragged(d)
    x = x.to(DEV)
    eager = m(x, lengths=lens)[0].clone()
    ops.set_graphs(True)
    try:
        m._plans.clear()
        first = m(x, lengths=lens)[0].clone()  # eager warm-up
        second = m(x, lengths=lens)[0].clone()  # capture + replay
        third = m(x, lengths=lens)[0].clone()  # replay
    finally:
        ops.set_graphs(False)
        m._plans.clear()
    torch.cuda.synchronize()
    assert torch.equal(first, eager) and torch.equal(second, eager) and torch.equal(third, eager)


# ------------------------------------------------------------------------------------------------ full geometry
def _seeded_state(m, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in m.state_shapes().items():
        r = torch.randn(shp, generator=g)
        if len(shp) == 4:
            sd[k] = r * math.sqrt(2.0 / (shp[1] * 9))
        elif ".rnn." in k or k.startswith("lang_model.rnn"):
            sd[k] = r / math.sqrt(shp[-1] if len(shp) == 2 else 64)
        elif len(shp) == 2:
            sd[k] = r / math.sqrt(shp[1])
        elif k.endswith("running_var"):
            sd[k] = (400.0 if k.endswith("cnn.1.running_var") else 0.5) * (1 + torch.rand(shp, generator=g))
        elif k.endswith("running_mean"):
            sd[k] = (20.0 if k.endswith("cnn.1.running_mean") else 0.2) * r
        elif "cnn" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.2 * r
        else:
            sd[k] = 0.1 * r
    return sd


def _front64(x, c, mel):
    n_fft, hop = c["win_length"], c["hop_length"]
    y = F.pad(x.view(1, 1, -1), (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    fr = y.unfold(-1, n_fft, hop)
    win = 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(n_fft, dtype=torch.float64) / n_fft)
    s = torch.fft.rfft(fr * win, dim=-1)
    db = 10.0 * torch.log10(torch.clamp((s.real ** 2 + s.imag ** 2) @ torch.from_numpy(mel).T, min=1e-10))
    return torch.max(db, db.max() - 80.0)  # (T, n_mels)


def _stack64(img, sd, pre, dil):
    x = img[None, None]
    for ci, bi, pad in ((0, 1, (dil, 1)), (3, 4, (1, 1)), (8, 9, (1, 1))):
        g = lambda k: sd[f"{pre}cnn.{k}"].double()
        x = F.conv2d(x, g(f"{ci}.weight"), g(f"{ci}.bias"), padding=pad, dilation=(dil if ci == 0 else 1, 1))
        x = F.relu(F.batch_norm(x, g(f"{bi}.running_mean"), g(f"{bi}.running_var"), g(f"{bi}.weight"),
                                g(f"{bi}.bias"), False, 0.0, 1e-5))
        if ci:
            x = F.max_pool2d(x, (1, 2))
    x = x.transpose(1, 2).flatten(-2)
    return F.linear(x, sd[f"{pre}fc.0.weight"].double(), sd[f"{pre}fc.0.bias"].double())


def _lstm64(x, sd, pre):
    H = sd[pre + "weight_hh_l0"].shape[1]
    rnn = torch.nn.LSTM(x.shape[-1], H, batch_first=True, bidirectional=True).double()
    rnn.load_state_dict({k[len(pre):]: v.double() for k, v in sd.items() if k.startswith(pre)})
    with torch.no_grad():
        return rnn(x)[0]


def _torch_forward64(m, sd, wave):
    """TranscriptionModel.eval() of one item restated with torch nn functions in float64"""
    c, lc = m.config, m.config["lang_model_config"]
    x = wave.double()
    with torch.no_grad():
        lang_img = _front64(x, lc, m.mel_matrix("lang"))
        ph = _lstm64(_stack64(lang_img, sd, "lang_model.conv_stack.", 1), sd, "lang_model.rnn.rnn.")
        ph = F.linear(ph, sd["lang_model.fc.weight"].double(), sd["lang_model.fc.bias"].double())
        lang = _lstm64(_stack64(ph[0], sd, "lang_conv_stack.", 2), sd, "lang_rnn.rnn.")
        pitch = _lstm64(_stack64(_front64(x, c, m.mel_matrix("pitch")), sd, "pitch_conv_stack.", 2), sd,
                        "pitch_rnn.rnn.")
        comb = _lstm64(torch.cat([pitch, lang], -1), sd, "combined_rnn.rnn.")
        return F.linear(comb, sd["combined_fc.weight"].double(), sd["combined_fc.bias"].double())[0]


@pytest.fixture(scope="module")
def base():
    m = TranscriptionModel(device=DEV)
    sd = _seeded_state(m, 3)
    return m.load_state_dict(sd), sd


def _waves(lens, seed):
    g = torch.Generator().manual_seed(seed)
    n = max(lens)
    t = torch.arange(n) / 16000.0
    x = torch.zeros(len(lens), n)
    for i, L in enumerate(lens):
        f0 = 150.0 * (1 + 0.25 * i)
        x[i, :L] = (0.3 * torch.sin(2 * math.pi * f0 * t[:L]) * torch.sin(math.pi * 3 * t[:L]) ** 2
                    + 0.02 * torch.randn(L, generator=g)) * (0.01 if i == 1 else 1.0)
    return x


def test_default_geometry_against_torch_fp64(base):
    m, sd = base
    lens = [48000, 170000, 100000]  # 151, 532, 313 frames
    x = _waves(lens, 5)
    out, T = m(x.to(DEV), lengths=lens)
    torch.cuda.synchronize()
    assert max(T) > 512
    for i, L in enumerate(lens):
        ref = _torch_forward64(m, sd, x[i, :L])
        _gate(out[i, :T[i]].cpu().numpy(), ref.numpy(), f"item {i}")


def test_ragged_batch_equals_single_calls(base):
    m, _ = base
    lens = [48000, 170000, 100000]
    x = _waves(lens, 6)
    splitk = ops.SPLITK
    ops.SPLITK = False
    try:
        m._plans.clear()
        out, T = m(x.to(DEV), lengths=lens)
        ones = [m(x[i, :L].to(DEV))[0][0] for i, L in enumerate(lens)]
    finally:
        ops.SPLITK = splitk
        m._plans.clear()
    torch.cuda.synchronize()
    for i, one in enumerate(ones):
        a, b = out[i, :T[i]].double(), one.double()
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 2e-6 * b.abs().max().item(), f"item {i}"


# ------------------------------------------------------------------------------------------------ unit checks
@pytest.mark.parametrize("H", [32, 40, 384, 512])
def test_bilstm_recurrence_against_nn_lstm(H):
    g = torch.Generator().manual_seed(H)
    B, T, I = 3, 530, 24
    lens = [530, 317, 1]
    rnn = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / math.sqrt(H))
    x = torch.randn(B, T, I, generator=g, dtype=torch.float64)
    sd = {k: v.float() for k, v in rnn.state_dict().items()}
    w_ih = torch.cat([sd["weight_ih_l0"], sd["weight_ih_l0_reverse"]]).double()
    b = torch.cat([sd["bias_ih_l0"].double() + sd["bias_hh_l0"].double(),
                   sd["bias_ih_l0_reverse"].double() + sd["bias_hh_l0_reverse"].double()])
    gin = (x @ w_ih.T + b).float().to(DEV)  # the projection is srn_conv_gemm's job; fed exactly here
    w_t = lstm_w_hh_t(sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]).to(DEV)
    ld = 2 * H + 8
    out = torch.full((B, T, ld), float("nan"), device=DEV)
    ops.CallOp("srn_bilstm_recur", (gin, T * 8 * H, 8 * H, torch.tensor(lens, dtype=torch.int32, device=DEV), w_t,
                                    (out, 4), T * ld, ld, B, T, H))()
    torch.cuda.synchronize()
    o = out.cpu().double()
    for i, L in enumerate(lens):
        with torch.no_grad():
            ref = rnn(x[i:i + 1, :L].double())[0][0]
        got = o[i, :L, 4:4 + 2 * H]
        assert (got - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), (H, i)
        assert (o[i, L:, 4:4 + 2 * H] == 0).all()
    assert torch.isnan(o[..., :4]).all() and torch.isnan(o[..., 4 + 2 * H:]).all()  # nothing outside its columns


@pytest.mark.parametrize("dil", [1, 2])
def test_layer0_conv_against_conv2d(dil):
    g = torch.Generator().manual_seed(dil)
    B, T, Fq, C, ld = 2, 97, 39, 12, 40
    lens = [97, 60]
    x = torch.randn(B, T, ld, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g)
    bias = torch.randn(C, generator=g)
    out = torch.full((B, T, Fq + 2, C), float("nan"), device=DEV)
    ops.CallOp("srn_trans_conv0", (x.to(DEV), T * ld, ld, torch.tensor(lens, dtype=torch.int32, device=DEV),
                                   w.reshape(C, 9).to(DEV), bias.to(DEV), out, B, T, Fq, C, dil))()
    torch.cuda.synchronize()
    o = out.cpu().double()
    for i, L in enumerate(lens):
        xi = x[i, :L, :Fq].double()[None, None]
        ref = F.relu(F.conv2d(xi, w.double(), bias.double(), padding=(dil, 1), dilation=(dil, 1)))[0]  # (C, L, F)
        assert (o[i, :L, 1:Fq + 1].permute(2, 0, 1) - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
        assert (o[i, :, 0] == 0).all() and (o[i, :, Fq + 1] == 0).all() and (o[i, L:] == 0).all()


def test_top_db_clamp_is_per_item():
    """two items 40 dB apart: each is clamped at its OWN maximum - 80 dB; one batch-wide maximum (torchaudio on a
    (B, F, T) tensor) would floor the quiet item 40 dB higher and fail here"""
    g = torch.Generator().manual_seed(1)
    B, T, nb, n_mels = 2, 50, 65, 16
    lens = [50, 41]
    spec = torch.randn(B, T, 2 * nb, generator=g, dtype=torch.float64) * torch.logspace(0, -6, T, dtype=torch.float64)[:, None]
    spec[1] *= 0.01  # 40 dB quieter
    mel = torch.rand(nb, n_mels, generator=g, dtype=torch.float64)
    out = torch.full((B, T, n_mels), float("nan"), device=DEV)
    gmax = torch.zeros(B, dtype=torch.int32, device=DEV)
    ops.CallOp("srn_mel_db", (spec.float().to(DEV), 2 * nb, nb, mel.float().to(DEV),
                              torch.tensor(lens, dtype=torch.int32, device=DEV), gmax, out, n_mels, B, T, n_mels, 1e-10,
                              80.0))()
    torch.cuda.synchronize()
    o = out.cpu().double()
    sf = spec.float().double()
    dbs = [10 * torch.log10(torch.clamp((sf[i, :L, :nb] ** 2 + sf[i, :L, nb:] ** 2) @ mel.float().double(), min=1e-10))
           for i, L in enumerate(lens)]
    batch_max = max(d.max() for d in dbs)
    for i, L in enumerate(lens):
        ref = torch.max(dbs[i], dbs[i].max() - 80.0)
        assert (o[i, :L] - ref).abs().max().item() <= 1e-3, i
        assert (o[i, L:] == 0).all()
        wrong = torch.max(dbs[i], batch_max - 80.0)
        if i == 1:
            assert (wrong - ref).abs().max().item() > 10.0  # the test tells the two clamps apart
