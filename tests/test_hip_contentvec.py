"""ContentVec on the MI355X (serenade_amd/contentvec.py + contentvec.hip + SRN_POST_GELU): the reduced fixture and the
hubert-base geometry against transformers, exact ragged batching, graph replay, and unit checks of the new kernels."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from serenade_amd import _lib, ops
from serenade_amd.contentvec import ContentVec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gate(out, ref, what):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape, what
    m = np.abs(ref).max()
    err = np.abs(out - ref)
    mx, rms = err.max() / m, np.sqrt((err ** 2).mean()) / m
    assert mx <= 2e-5 and rms <= 2e-6, f"{what}: max {mx:.2e} rms {rms:.2e} of max|ref|"


def _seeded_state(cv, seed):
    """a HubertModel-shaped state dict from a seeded generator (no transformers needed): He-scaled convs, 0.02 linears
    (HubertPreTrainedModel._init_weights), perturbed norm affines"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in cv.state_shapes().items():
        r = torch.randn(shp, generator=g)
        if k.endswith("weight_g"):
            sd[k] = 1.0 + 0.1 * r
        elif k.endswith("weight_v") or (k.endswith("conv.weight")):
            sd[k] = r * math.sqrt(2.0 / (shp[1] * shp[2]))
        elif "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.2 * r
        elif k.endswith("bias"):
            sd[k] = 0.05 * r
        else:
            sd[k] = 0.02 * r
    return sd


@pytest.fixture(scope="module")
def small(golden):
    d = golden("contentvec_small")
    cfg = json.loads(str(d["config"]))
    cv = ContentVec(device=DEV, **cfg).load_state_dict({k[3:]: torch.from_numpy(v) for k, v in d.items()
                                                        if k.startswith("sd.")})
    return cv, d


def test_fixture_per_item(small):
    cv, d = small
    for i in range(2):
        out = cv(torch.from_numpy(d[f"wave{i}"]).to(DEV))
        torch.cuda.synchronize()
        _gate(out[0].cpu().numpy(), d[f"ref{i}"], f"item {i}")


def test_fixture_as_a_ragged_batch(small):
    cv, d = small
    n0, n1 = len(d["wave0"]), len(d["wave1"])
    x = torch.zeros(2, n1)
    x[0, :n0] = torch.from_numpy(d["wave0"])
    x[0, n0:] = 7.0  # padding never reaches a valid frame
    x[1] = torch.from_numpy(d["wave1"])
    out, T = cv(x.to(DEV), lengths=[n0, n1])
    torch.cuda.synchronize()
    for i in range(2):
        _gate(out[i, :T[i]].cpu().numpy(), d[f"ref{i}"], f"ragged item {i}")


@pytest.fixture(scope="module")
def base():
    cv = ContentVec(device=DEV)
    sd = _seeded_state(cv, 11)
    return cv.load_state_dict(sd), sd


def test_full_geometry_against_transformers_fp64(base):
    transformers = pytest.importorskip("transformers")
    cv, sd = base
    m = transformers.HubertModel(transformers.HubertConfig()).eval()
    m.feature_extractor.conv_layers[-1].conv.stride = (1,)
    pre = "encoder.pos_conv_embed.conv."
    sd_t = dict(sd)
    sd_t[pre + "parametrizations.weight.original0"] = sd_t.pop(pre + "weight_g")
    sd_t[pre + "parametrizations.weight.original1"] = sd_t.pop(pre + "weight_v")
    m.load_state_dict(sd_t, strict=False)
    m = m.double()
    g = torch.Generator().manual_seed(4)
    for n in (16000, 21937):
        x = 0.3 * torch.randn(n, generator=g)
        with torch.no_grad():
            ref = m(x.double().view(1, -1)).last_hidden_state[0].numpy()
        out = cv(x.to(DEV))
        torch.cuda.synchronize()
        _gate(out[0].cpu().numpy(), ref, f"hubert-base n={n}")


def test_exact_ragged_batch_equals_single_calls(base):
    """Split-K (on by default) reorders the sums of the small B = 1 grids, so it is off here: then the batch and the
    single calls run the same kernels and differ only where the padded length changes a reduction (the softmax rows
    of the shorter items); the longest item is bit for bit its own B = 1 call."""
    cv, _ = base
    lens = [16000, 37920, 48000]
    g = torch.Generator().manual_seed(9)
    x = 0.3 * torch.randn(3, 48000, generator=g)
    splitk = ops.SPLITK
    ops.SPLITK = False
    try:
        cv._plans.clear()
        out, T = cv(x.to(DEV), lengths=lens)
        ones = [cv(x[i, :n].to(DEV))[0] for i, n in enumerate(lens)]
    finally:
        ops.SPLITK = splitk
        cv._plans.clear()
    torch.cuda.synchronize()
    assert T == [cv.frames(n) for n in lens]
    for i, one in enumerate(ones):
        a, b = out[i, :T[i]].double(), one.double()
        assert (a - b).abs().max().item() <= 2e-6 * b.abs().max().item(), f"item {i}"
    assert torch.equal(out[2], ones[2])


def test_graph_replay_equals_eager(small):
    cv, d = small
    x = torch.from_numpy(d["wave1"]).to(DEV)
    eager = cv(x).clone()
    ops.set_graphs(True)
    try:
        cv._plans.clear()
        first = cv(x).clone()  # eager warm-up
        second = cv(x).clone()  # capture + replay
        third = cv(x).clone()  # replay
    finally:
        ops.set_graphs(False)
    torch.cuda.synchronize()
    assert torch.equal(first, eager) and torch.equal(second, eager) and torch.equal(third, eager)


# ------------------------------------------------------------------------------------------------ unit checks
def _route(op):
    out = (ctypes.c_int32 * 3)()
    assert _lib.lib().srn_conv_gemm_route(ctypes.byref(op.p), out) == 0
    return tuple(out)


@pytest.mark.parametrize("case", ["f32", "fast", "generic", "splitk", "halo", "strip"])
def test_post_gelu_on_every_family(case):
    g = torch.Generator().manual_seed(1)
    B, T, C, N, k = 2, 300, 64, 64, 3
    prec, route = _lib.PREC_FP32, _lib.ROUTE_AUTO
    want = {"f32": _lib.FAMILY_F32, "fast": _lib.FAMILY_FAST, "generic": _lib.FAMILY_GENERIC,
            "splitk": _lib.FAMILY_F32, "halo": _lib.FAMILY_HALO, "strip": _lib.FAMILY_STRIP}[case]
    if case == "fast":
        route = _lib.ROUTE_FAST_FP32
    elif case == "generic":
        route = _lib.ROUTE_GENERIC
    elif case == "splitk":
        B, T, C, N, k = 1, 40, 512, 64, 3
    elif case == "halo":
        prec, route, N, k = _lib.PREC_BF16X3, _lib.ROUTE_HALO, 128, 7
    elif case == "strip":
        prec, route = _lib.PREC_BF16X3, _lib.ROUTE_STRIP
    x = torch.randn(B, T, C, generator=g).to(DEV)
    wt = (torch.randn(N, C, k, generator=g) / math.sqrt(C * k)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    out = torch.zeros(B, T, N, device=DEV)
    op = ops.ConvOp(in0=x, w=ops.pack_conv_weight(wt), out=out, n_batch=B, T_in=T, T_out=T, C_in=C, N=N,
                    in0_bs=T * C, ld_in0=C, ldw=k * C, out_bs=T * N, ld_out=N, taps=ops.conv_taps(k), bias=bias,
                    post=_lib.POST_GELU, precision=prec, route=route)
    r = _route(op)
    assert r[0] == want, r
    if case == "splitk":
        assert r[2] > 1, r
    op()
    torch.cuda.synchronize()
    ref = F.gelu(F.conv1d(x.double().transpose(1, 2), wt.double(), bias.double(), padding=k // 2)).transpose(1, 2)
    tol = 2e-6 if prec == _lib.PREC_FP32 else 5e-4
    assert (out.double() - ref).abs().max().item() <= tol * ref.abs().max().item(), case


def test_conv0_and_channel_norm_on_valid_frames():
    g = torch.Generator().manual_seed(2)
    B, C, k, s = 2, 512, 10, 5
    ns = [8001, 5003]
    n = max(ns)
    wave = torch.randn(B, n, generator=g)
    T0 = (n - k) // s + 1
    lens = [(v - k) // s + 1 for v in ns]
    w = torch.randn(C, 1, k, generator=g) * 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    d = lambda t: t.to(DEV).contiguous()
    lib = _lib.lib()
    chunks = lib.srn_frame_stats_chunks(T0)
    out = torch.full((B, T0, C), float("nan"), device=DEV)
    parts = torch.zeros(B, chunks, C, 2, device=DEV, dtype=torch.float64)
    stats = torch.zeros(B, C, 2, device=DEV)
    y = torch.full((B, T0, C), float("nan"), device=DEV)
    dw, lens_d, dwave = d(w.reshape(C, k)), torch.tensor(lens, device=DEV, dtype=torch.int32), d(wave)
    ops.CallOp("srn_cvec_conv0", (dwave, n, n, lens_d, dw, out, parts, B, T0, C, k, s))()
    ops.CallOp("srn_channel_norm_gelu", (out, parts, chunks, lens_d, d(gamma), d(beta), stats, y, B, T0, C, 1e-5))()
    torch.cuda.synchronize()
    for b in range(B):
        c = F.conv1d(wave[b, :ns[b]].double().view(1, 1, -1), w.double(), stride=s)[0]  # (C, lens[b])
        assert c.shape[1] == lens[b]
        got = out[b, :lens[b]].double().cpu().t()
        assert (got - c).abs().max().item() <= 1e-6 * c.abs().max().item()
        assert (out[b, lens[b]:] == 0).all() and (y[b, lens[b]:] == 0).all()
        ref = F.gelu(F.group_norm(c.unsqueeze(0), C, gamma.double(), beta.double(), 1e-5))[0]
        gy = y[b, :lens[b]].double().cpu().t()
        assert (gy - ref).abs().max().item() <= 2e-5 * ref.abs().max().item(), b


@pytest.mark.parametrize("D,G,K", [(768, 16, 128), (128, 4, 16), (64, 4, 16)])
def test_posconv_against_grouped_conv1d(D, G, K):
    g = torch.Generator().manual_seed(3)
    B, T = 2, 203
    lens = [203, 150]
    x = torch.randn(B, T, D, generator=g)
    Cg = D // G
    w = torch.randn(D, Cg, K, generator=g) / math.sqrt(Cg * K)
    bias = 0.1 * torch.randn(D, generator=g)
    npad = 32 if Cg <= 32 else 64
    packed = torch.zeros(G, K, Cg, npad)
    packed[..., :Cg] = w.reshape(G, Cg, Cg, K).permute(0, 3, 2, 1)
    y = torch.full((B, T, D), float("nan"), device=DEV)
    ops.CallOp("srn_posconv_gelu_res", (x.to(DEV), torch.tensor(lens, device=DEV, dtype=torch.int32), packed.to(DEV),
                                        bias.to(DEV), y, B, T, D, G, K, K // 2))()
    torch.cuda.synchronize()
    for b in range(B):
        xv = x[b, :lens[b]].double().t().unsqueeze(0)  # rows past the length read as zero
        c = F.conv1d(xv, w.double(), bias.double(), padding=K // 2, groups=G)
        if K % 2 == 0:
            c = c[..., :-1]  # HubertSamePadLayer
        ref = x[b, :lens[b]].double() + F.gelu(c[0].t())
        got = y[b, :lens[b]].double().cpu()
        # one k-ordered fp32 fma chain over Cg * K (6144 at hubert-base) products: ~sqrt(K) 2^-24 per unit of the sum
        assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), b
    assert torch.isfinite(y).all()
