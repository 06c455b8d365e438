"""GPU parity tests (run with -m gpu on an MI355X): every HIP kernel family through the C ABI against
(a) the executable C-ABI spec / the CPU oracle on identical seeded inputs, (b) the reference's golden
vectors, and (c) size-independent properties at BASELINE.json's full sizes.

Tolerances: the path is fp32 end to end (exact-fp32 MFMA), so kernels are held to 2e-5 of the tensor's
max (summation-order noise); the end-to-end gates are the north-star ones: mel <= 1e-3 relative,
waveform <= 1e-4 absolute."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import serenade_oracle as O
from serenade_amd import _lib, models, ops, vocoder
from serenade_amd.utils.synth import SERENADE_PARAMS, fill_state_dict, synth_inputs
from tests import _emulator
from tests._weights import hifigan_weights, serenade_weights, sub
from tests.test_conv_route import library_forms

import serenade_amd

pytestmark = pytest.mark.gpu

MEL_RTOL = 1e-3
WAVE_ATOL = 1e-4


class _Tol:
    """kernel-level tolerance (fraction of the tensor's max) of the active contraction precision:
    exact-fp32 MFMA differs from the CPU only by summation order; split-bf16 carries ~2^-17 per product."""
    k = 2e-5
    model = 1e-4


KTOL = _Tol


@pytest.fixture(autouse=True, params=["fp32", "bf16x3", "bf16x6"])
def precision(request):
    serenade_amd.set_precision(request.param)
    # bf16x6 (exact three-way operand split, 6 MFMA per product) is held to the exact-fp32 tolerances
    _Tol.k = 1e-4 if request.param == "bf16x3" else 2e-5
    _Tol.model = MEL_RTOL if request.param == "bf16x3" else 1e-4
    yield request.param
    serenade_amd.set_precision("fp32")  # the package default


def T(a):
    return torch.from_numpy(np.asarray(a))


def nerr(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need an MI355X"
    _lib.lib()  # must load: the product has no fallback
    return torch.device("cuda:0")


class Mirror:
    """maps CPU tensors (and (tensor, offset) pairs) to device clones, preserving aliasing"""

    def __init__(self, dev):
        self.dev, self.map = dev, {}

    def __call__(self, x):
        if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], torch.Tensor):
            return (self(x[0]), x[1])
        if isinstance(x, torch.Tensor):
            if id(x) not in self.map:
                self.map[id(x)] = (x, x.to(self.dev).clone())
            return self.map[id(x)][1]
        return x

    def pairs(self):
        return list(self.map.values())


def run_conv_both(dev, kw, tol=None, tiles=(0,)):
    """run the kernel (for each tile id) and the spec on clones of the same inputs; compare every buffer"""
    base = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    tol = KTOL.k if tol is None else tol
    # two kernel families behind the one entry point: the specialised ones (conv_fast / halo / strip; auto) and the
    # generic conv_gemm kernel (ROUTE_GENERIC forces it)
    # (exact fp32 has two implementations of the specialised loop: conv_f32.hip, and conv_fast.hip's behind ROUTE_FAST_FP32)
    variants = ("auto", "generic", "fast_fp32")
    for tile, variant in [(t, u) for t in tiles for u in variants]:
        cpu = {}
        memo = {}

        def cl(v):
            if isinstance(v, torch.Tensor):
                if id(v) not in memo:
                    memo[id(v)] = v.clone()
                return memo[id(v)]
            if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], torch.Tensor):
                return (cl(v[0]), v[1])
            return v

        for k, v in kw.items():
            cpu[k] = cl(v)
        m = Mirror(dev)
        gpu = {k: m(v) for k, v in cpu.items()}
        gpu["tile"] = tile
        if variant == "generic":
            if gpu.get("route"):
                continue
            gpu["route"] = _lib.ROUTE_GENERIC
        if variant == "fast_fp32":
            if gpu.get("route") or serenade_amd.get_precision() != "fp32":
                continue
            gpu["route"] = _lib.ROUTE_FAST_FP32
        op = ops.ConvOp(**gpu)
        op()
        torch.cuda.synchronize()
        _emulator.emul_conv(cpu)
        for c, g in m.pairs():
            if c.is_floating_point():
                e = nerr(g, c)
                assert e < tol, f"tile {tile} {variant}: mismatch {e}"
    del base


def rnd(*s, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(s).astype(np.float32))


# 0 (the route's own choice) and every id up to the last one the library lists a form for -- 11: 64 x 64, loads two steps
# ahead; 7, 9: the single-LDS-stage forms (6, 8 have no form and run their twins 1, 2); 10: 32 x 64, step split over wave pairs
ALL_TILES = tuple(range(max(f.tile for f in library_forms()) + 1))


def test_library_exports_and_error_path(dev):
    lib = _lib.lib()
    assert lib.srn_abi_version() == 4
    rc = lib.srn_conv_gemm(None, None)
    assert rc != 0 and b"null" in lib.srn_last_error()


def test_linear_ragged(dev):
    M, K, N = 200, 96, 80
    kw = dict(in0=rnd(M, K, seed=1), w=rnd(N, K, seed=2), bias=rnd(N, seed=3), out=torch.zeros(M, N), n_batch=1,
              T_in=M, T_out=M, C_in=K, N=N, ld_in0=K, ldw=K, ld_out=N)
    run_conv_both(dev, kw, tiles=ALL_TILES)


def test_conv_k3_mask_and_gn_partials(dev):
    B, Tn, C, N = 2, 70, 64, 128
    x = rnd(B, Tn, C, seed=4)
    w = ops.pack_conv_weight(rnd(N, C, 3, seed=5))
    kw = dict(in0=x, w=w, bias=rnd(N, seed=6), out=torch.zeros(B, Tn, N), n_batch=B, T_in=Tn, T_out=Tn, C_in=C, N=N,
              in0_bs=Tn * C, ld_in0=C, ldw=3 * C, out_bs=Tn * N, ld_out=N, taps=ops.conv_taps(3),
              len_in=torch.tensor([70, 41], dtype=torch.int32), gn_partials=torch.zeros(B, 3, N // 32, 2))
    run_conv_both(dev, kw, tiles=ALL_TILES)
    # and directly against F.conv1d
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw.items()}
    ops.ConvOp(**g)()
    mask = (torch.arange(Tn)[None] < kw["len_in"][:, None]).float().unsqueeze(-1)
    ref = F.conv1d((x * mask).transpose(1, 2), rnd(N, C, 3, seed=5), kw["bias"], padding=1).transpose(1, 2)
    assert nerr(g["out"], ref) < KTOL.k


def test_conv_k7_reflect_leaky_and_dilated_k11(dev):
    B, Tn, C, N = 2, 45, 32, 64
    x = rnd(B, Tn, C, seed=7)
    w7 = rnd(N, C, 7, seed=8)
    kw = dict(in0=x, w=ops.pack_conv_weight(w7), bias=rnd(N, seed=9), out=torch.zeros(B, Tn, N), n_batch=B, T_in=Tn,
              T_out=Tn, C_in=C, N=N, in0_bs=Tn * C, ld_in0=C, ldw=7 * C, out_bs=Tn * N, ld_out=N,
              taps=ops.conv_taps(7), reflect=True, pro_act=_lib.ACT_LEAKY, pro_slope=0.2)
    run_conv_both(dev, kw, tiles=(0, 2, 4))
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw.items()}
    ops.ConvOp(**g)()
    ref = F.conv1d(F.pad(F.leaky_relu(x, 0.2).transpose(1, 2), (3, 3), mode="reflect"), w7, kw["bias"]).transpose(1, 2)
    assert nerr(g["out"], ref) < KTOL.k
    w11 = rnd(N, C, 11, seed=10)
    kw2 = dict(kw, w=ops.pack_conv_weight(w11), ldw=11 * C, taps=ops.conv_taps(11, 5), reflect=False,
               pro_slope=0.1, out=torch.zeros(B, Tn, N))
    run_conv_both(dev, kw2, tiles=(0, 5))
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw2.items()}
    ops.ConvOp(**g)()
    ref = F.conv1d(F.leaky_relu(x, 0.1).transpose(1, 2), w11, kw["bias"], dilation=5, padding=25).transpose(1, 2)
    assert nerr(g["out"], ref) < KTOL.k


def test_conv_stride2_and_concat(dev):
    B, Tn, C, N = 2, 67, 64, 64
    x, s = rnd(B, Tn, C, seed=11), rnd(B, Tn, 32, seed=12)
    To = (Tn + 1) // 2
    w = rnd(N, C, 3, seed=13)
    kw = dict(in0=x, w=ops.pack_conv_weight(w), bias=rnd(N, seed=14), out=torch.zeros(B, To, N), n_batch=B, T_in=Tn,
              T_out=To, C_in=C, N=N, in0_bs=Tn * C, ld_in0=C, ldw=3 * C, out_bs=To * N, ld_out=N,
              taps=ops.conv_taps(3), in_stride=2, len_in=torch.tensor([67, 30], dtype=torch.int32))
    run_conv_both(dev, kw, tiles=(0, 3, 4))
    wc = rnd(N, C + 32, 3, seed=15)
    kw2 = dict(in0=x, in1=s, C_in0=C, in1_bs=Tn * 32, ld_in1=32, w=ops.pack_conv_weight(wc), bias=None,
               out=torch.zeros(B, Tn, N), n_batch=B, T_in=Tn, T_out=Tn, C_in=C + 32, N=N, in0_bs=Tn * C, ld_in0=C,
               ldw=3 * (C + 32), out_bs=Tn * N, ld_out=N, taps=ops.conv_taps(3))
    run_conv_both(dev, kw2, tiles=(0, 1, 4))
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw2.items()}
    ops.ConvOp(**g)()
    ref = F.conv1d(torch.cat([x, s], -1).transpose(1, 2), wc, None, padding=1).transpose(1, 2)
    assert nerr(g["out"], ref) < KTOL.k


def test_geglu_epilogue(dev):
    M, K, inner = 150, 64, 128
    w, b = rnd(2 * inner, K, seed=16), rnd(2 * inner, seed=17)
    wp, bp = ops.pack_geglu(w, b)
    x = rnd(M, K, seed=18)
    kw = dict(in0=x, w=wp, bias=bp, out=torch.zeros(M, inner), n_batch=1, T_in=M, T_out=M, C_in=K, N=2 * inner,
              N_out=inner, ld_in0=K, ldw=K, ld_out=inner, geglu=True)
    run_conv_both(dev, kw, tiles=(0, 1, 2, 3))
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw.items()}
    ops.ConvOp(**g)()
    h, gate = (x @ w.t() + b).chunk(2, -1)
    assert nerr(g["out"], h * F.gelu(gate)) < KTOL.k


def test_residual_modes_inplace(dev):
    B, Tn, C, N = 2, 40, 32, 32
    x = rnd(B, Tn, C, seed=19)
    w = ops.pack_conv_weight(rnd(N, C, 3, seed=20))
    acc = rnd(B, Tn, N, seed=21)
    r = rnd(B, Tn, N, seed=22)
    common = dict(in0=x, w=w, bias=rnd(N, seed=23), n_batch=B, T_in=Tn, T_out=Tn, C_in=C, N=N, in0_bs=Tn * C,
                  ld_in0=C, ldw=3 * C, out_bs=Tn * N, ld_out=N, taps=ops.conv_taps(3))
    # out = (conv + r + acc) / 3 written in place over acc (HiFi-GAN stage mean)
    run_conv_both(dev, dict(common, out=acc, res=r, res_mode=_lib.RES_ADD, res_bs=Tn * N, ld_res=N, res2=acc,
                            res2_bs=Tn * N, ld_res2=N, post=_lib.POST_DIV, post_div=3.0), tiles=(0, 5))
    # Euler: h0[:, :, :N] += dt * (conv * mask) in place with a wider row stride
    h0 = rnd(B, Tn, 48, seed=24)
    run_conv_both(dev, dict(common, out=h0, out_bs=Tn * 48, ld_out=48, res=h0, res_mode=_lib.RES_AXPY, beta=0.1,
                            res_bs=Tn * 48, ld_res=48, len_out=torch.tensor([40, 17], dtype=torch.int32)),
                  tiles=(0, 4, 5))
    # tanh output: weights scaled so that the pre-activations are O(1) (error is judged on the tanh output)
    run_conv_both(dev, dict(common, w=w * 0.1, out=torch.zeros(B, Tn, N), post=_lib.POST_TANH), tiles=(0,))


def test_attention_batched_gemms(dev):
    B, H, L, d = 2, 2, 70, 64
    inner = H * d
    qkv = rnd(B, L, 3 * inner, seed=25)
    Lp = 72
    S = torch.zeros(B * H, L, Lp)
    kw = dict(in0=qkv, w=(qkv, inner), out=S, n_batch=B, n_head=H, T_in=L, T_out=L, C_in=d, N=L,
              in0_bs=L * 3 * inner, in0_hs=d, ld_in0=3 * inner, w_bs=L * 3 * inner, w_hs=d, ldw=3 * inner,
              out_bs=H * L * Lp, out_hs=L * Lp, ld_out=Lp, alpha=0.125)
    run_conv_both(dev, kw, tiles=(0, 1, 4))
    P = torch.softmax(rnd(B * H, L, Lp, seed=26), -1)
    P[:, :, L:] = 0
    O_ = torch.zeros(B, L, inner)
    kw2 = dict(in0=P, w=(qkv, 2 * inner), out=O_, n_batch=B, n_head=H, T_in=L, T_out=L, C_in=Lp, C_w=L, N=d,
               in0_bs=H * L * Lp, in0_hs=L * Lp, ld_in0=Lp, w_bs=L * 3 * inner, w_hs=d, ldw=3 * inner, w_nmajor=True,
               out_bs=L * inner, out_hs=d, ld_out=inner)
    run_conv_both(dev, kw2, tiles=(0, 1, 3, 4))
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw2.items()}
    ops.ConvOp(**g)()
    v = qkv[:, :, 2 * inner:].view(B, L, H, d).permute(0, 2, 1, 3)
    ref = (P[:, :, :L].view(B, H, L, L) @ v).permute(0, 2, 1, 3).reshape(B, L, inner)
    assert nerr(g["out"], ref) < KTOL.k


@pytest.mark.parametrize("stride,k", [(2, 4), (8, 16), (5, 10), (3, 6)])
def test_conv_transpose_phases(dev, stride, k):
    B, Tn, Ci, Co = 2, 19, 64, 32
    x = rnd(B, Tn, Ci, seed=27)
    w = rnd(Ci, Co, k, seed=28)
    bias = rnd(Co, seed=29)
    pad, opad = (1, 0) if (stride, k) == (2, 4) else (stride // 2 + stride % 2, stride % 2)
    ref = F.conv_transpose1d(F.leaky_relu(x, 0.1).transpose(1, 2), w, bias, stride=stride, padding=pad,
                             output_padding=opad).transpose(1, 2)
    To = ref.shape[1]
    out = torch.zeros(B, To, Co, device=dev)
    xd, bd = x.to(dev), bias.to(dev)
    for r, (taps, wp) in enumerate(ops.convtranspose_phases(w, stride, pad)):
        rows = (To - r + stride - 1) // stride
        ops.ConvOp(in0=xd, w=wp.to(dev), bias=bd, out=out, n_batch=B, T_in=Tn, T_out=rows, C_in=Ci, N=Co,
                   in0_bs=Tn * Ci, ld_in0=Ci, ldw=wp.shape[1], out_bs=To * Co, ld_out=Co, taps=taps,
                   pro_act=_lib.ACT_LEAKY, pro_slope=0.1, out_t_stride=stride, out_t_off=r)()
    assert nerr(out, ref) < KTOL.k


def test_prologue_silu_mish(dev):
    M, K, N = 10, 128, 96
    for act in (_lib.ACT_SILU, _lib.ACT_MISH):
        kw = dict(in0=rnd(M, K, seed=30) * 3, w=rnd(N, K, seed=31), bias=rnd(N, seed=32), out=torch.zeros(M, N),
                  n_batch=1, T_in=M, T_out=M, C_in=K, N=N, ld_in0=K, ldw=K, ld_out=N, pro_act=act)
        run_conv_both(dev, kw, tiles=(0, 4))


def _run_call(dev, name, args):
    cpu = [a.clone() if isinstance(a, torch.Tensor) else a for a in args]
    m = Mirror(dev)
    gpu = [m(a) for a in cpu]
    ops.CallOp(name, gpu)()
    torch.cuda.synchronize()
    _emulator.emul_call(name, cpu)
    worst = 0.0
    for c, g in m.pairs():
        if c.is_floating_point():
            worst = max(worst, nerr(g, c))
    return worst


def _partials(x):
    B, Tn, C = x.shape
    mt, nt = (Tn + 31) // 32, C // 32
    pad = torch.zeros(B, mt * 32, C)
    pad[:, :Tn] = x
    t = pad.reshape(B, mt, 32, nt, 32)
    return torch.stack([t.sum(dim=(2, 4)), (t ** 2).sum(dim=(2, 4))], dim=-1).contiguous()


def _fused_tail_equals_tail_then_layernorm(dev, x, lens, gam, bet, res, ss, g2, b2, groups):
    """srn_resblock_tail_ln against srn_resblock_tail + srn_layernorm, bit for bit (both run row_common.h's LayerNorm)"""
    B, Tn, C = x.shape
    d = lambda t: t.to(dev)
    args = (d(x), d(_partials(x)), d(gam), d(bet), d(lens), d(res), (d(ss), C), (d(ss), 2 * C), 4 * C)
    y_a, y_b, n_a, n_b = (torch.zeros(B, Tn, C, device=dev) for _ in range(4))
    ops.resblock_tail_op(*args, y_a, B, Tn, C, groups=groups)()
    ops.layernorm_op(y_a, d(g2), d(b2), n_a, B * Tn, C)()
    ops.resblock_tail_ln_op(*args, y_b, d(g2), d(b2), n_b, B, Tn, C, groups=groups)()
    torch.cuda.synchronize()
    assert y_a.abs().sum() > 0 and n_a.abs().sum() > 0
    assert torch.equal(y_a, y_b) and torch.equal(n_a, n_b)


@pytest.mark.parametrize("C,groups", [(128, 4), (320, 2), (1024, 8)])
def test_fused_tail_is_bit_identical_to_tail_then_layernorm(dev, C, groups):
    """half a wave; a partly filled second float4 slot; every slot full.  B = 2, T = 5: the last rows' waves idle"""
    B, Tn = 2, 5
    x = rnd(B, Tn, C, seed=33) * 2 + 0.3
    lens = torch.tensor([5, 3], dtype=torch.int32)
    _fused_tail_equals_tail_then_layernorm(dev, x, lens, 1 + 0.1 * rnd(C, seed=34), 0.1 * rnd(C, seed=35),
                                           rnd(B, Tn, C, seed=38), rnd(B, 4 * C, seed=37), 1 + 0.1 * rnd(C, seed=45),
                                           0.1 * rnd(C, seed=46), groups)


@pytest.mark.parametrize("C", [4, 260, 1024])
def test_rowln_fwd_with_a_shared_affine_is_bit_identical_to_layernorm(dev, C):
    """one lane; lane 0 alone in the second float4 slot; every slot full.  10 rows: the last workgroup is partly empty"""
    B, Tn = 2, 5
    x = (rnd(B, Tn, C, seed=50) * 2 + 0.3).to(dev)
    m, a = (1 + 0.1 * rnd(C, seed=51)).to(dev), (0.1 * rnd(C, seed=52)).to(dev)
    y_a, y_b = torch.zeros(B, Tn, C, device=dev), torch.zeros(B, Tn, C, device=dev)
    ops.CallOp("srn_rowln_fwd", (x, m, 0, a, 0, y_a, B, Tn, C, 1e-5))()
    ops.layernorm_op(x, m, a, y_b, B * Tn, C)()
    torch.cuda.synchronize()
    assert y_a.abs().sum() > 0 and torch.equal(y_a, y_b)


@pytest.mark.parametrize("H", [4, 128, 1024 // 3])  # both launchers require 3 H <= 1024
def test_gru_recur_last_is_the_last_state_of_gru_train_fwd(dev, H):
    B, Tn = 3, 5
    gi, w, bh = rnd(B, Tn, 3 * H, seed=70).to(dev), (rnd(H, 3 * H, seed=71) / 11).to(dev), (0.1 * rnd(3 * H, seed=72)).to(dev)
    h = torch.zeros(B, H, device=dev)
    hs, gates = torch.zeros(B, Tn + 1, H, device=dev), torch.zeros(B, Tn, 4 * H, device=dev)
    ops.gru_recur_last_op(gi, w, bh, h, B, Tn, H)()
    ops.CallOp("srn_gru_train_fwd", (gi, w, bh, hs, gates, B, Tn, H))()
    torch.cuda.synchronize()
    assert h.abs().sum() > 0 and torch.equal(h, hs[:, Tn])


def test_norm_and_elementwise_kernels(dev):
    B, Tn, C = 2, 75, 512
    x = rnd(B, Tn, C, seed=33) * 2 + 0.3
    lens = torch.tensor([75, 44], dtype=torch.int32)
    gam, bet, tb = 1 + 0.1 * rnd(C, seed=34), 0.1 * rnd(C, seed=35), rnd(4 * C, seed=36)
    e = _run_call(dev, "srn_gn_mish_apply", [x, _partials(x), gam, bet, (tb, C), 0, lens, torch.zeros(B, Tn, C), B,
                                             Tn, C, 8, 1e-5, 0])
    assert e < KTOL.k
    # valid_stats: statistics over each item's own rows (its padded rows zeroed by the producing conv) == the
    # GroupNorm of the unpadded item
    xz = x * (torch.arange(Tn)[None] < lens[:, None]).float().unsqueeze(-1)
    yv = torch.zeros(B, Tn, C, device=dev)
    ops.gn_mish_apply_op(xz.to(dev), _partials(xz).to(dev), gam.to(dev), bet.to(dev), None, lens.to(dev), yv, B, Tn, C,
                         valid_stats=True)()
    for b in range(B):
        n = int(lens[b])
        one = F.mish(F.group_norm(x[b:b + 1, :n].transpose(1, 2), 8, gam, bet, 1e-5)).transpose(1, 2)
        assert nerr(yv[b:b + 1, :n], one) < KTOL.k and not yv[b, n:].any()
    e = _run_call(dev, "srn_gn_mish_apply", [xz, _partials(xz), gam, bet, None, 0, lens, torch.zeros(B, Tn, C), B, Tn,
                                             C, 8, 1e-5, 1])
    assert e < KTOL.k
    # against torch's GroupNorm directly (statistics over the padded length)
    y = torch.zeros(B, Tn, C, device=dev)
    ops.gn_mish_apply_op(x.to(dev), _partials(x).to(dev), gam.to(dev), bet.to(dev), None, lens.to(dev), y, B, Tn, C)()
    mask = (torch.arange(Tn)[None] < lens[:, None]).float().unsqueeze(-1)
    ref = F.mish(F.group_norm(x.transpose(1, 2), 8, gam, bet, 1e-5)).transpose(1, 2) * mask
    assert nerr(y, ref) < KTOL.k
    ss = rnd(B, 4 * C, seed=37)
    e = _run_call(dev, "srn_resblock_tail", [x, _partials(x), gam, bet, lens, rnd(B, Tn, C, seed=38), (ss, C),
                                             (ss, 2 * C), 4 * C, torch.zeros(B, Tn, C), B, Tn, C, 8, 1e-5, 1e-5, 0])
    assert e < KTOL.k
    e = _run_call(dev, "srn_resblock_tail", [xz, _partials(xz), gam, bet, lens, rnd(B, Tn, C, seed=38), (ss, C),
                                             (ss, 2 * C), 4 * C, torch.zeros(B, Tn, C), B, Tn, C, 8, 1e-5, 1e-5, 1])
    assert e < KTOL.k
    # the fused form (tail + the transformer block's norm1 in one launch) against the spec, and bit for bit against the
    # two separate launches
    g2, b2 = 1 + 0.1 * rnd(C, seed=45), 0.1 * rnd(C, seed=46)
    e = _run_call(dev, "srn_resblock_tail_ln", [x, _partials(x), gam, bet, lens, rnd(B, Tn, C, seed=38), (ss, C),
                                                (ss, 2 * C), 4 * C, torch.zeros(B, Tn, C), B, Tn, C, 8, 1e-5, 1e-5, 0,
                                                g2, b2, torch.zeros(B, Tn, C), 1e-5])
    assert e < KTOL.k
    _fused_tail_equals_tail_then_layernorm(dev, x, lens, gam, bet, rnd(B, Tn, C, seed=38), ss, g2, b2, 8)
    src = rnd(2, 9, 5, seed=44)
    e = _run_call(dev, "srn_scatter_rows", [src, 45, 5, torch.zeros(2, 16, 8), 128, 8, 2,
                                            torch.tensor([3, 7], dtype=torch.int32),
                                            torch.tensor([9, 4], dtype=torch.int32), 2, 9, 5])
    assert e == 0
    e = _run_call(dev, "srn_layernorm", [x.reshape(-1, C), gam, bet, torch.zeros(B * Tn, C), B * Tn, C, 1e-5])
    assert e < KTOL.k
    for L, ld in ((70, 72), (300, 300), (1280, 1280), (2176, 2176)):
        s = rnd(4, L, ld, seed=39) * 3
        e = _run_call(dev, "srn_softmax_rows", [s, torch.tensor([L, max(1, L - 9)], dtype=torch.int32), 4, 2, L, ld])
        assert e < KTOL.k
    t = torch.tensor([0.0, 0.1, 0.3, 0.9], dtype=torch.float32)
    e = _run_call(dev, "srn_sinusoidal_emb", [t, torch.zeros(4, 256), 4, 242, 256, 1000.0])
    assert e < 2e-4  # sin/cos of arguments up to 1e3: 1 ulp of the argument is ~6e-5
    src = rnd(2, 9, 5, seed=40)
    e = _run_call(dev, "srn_copy_channels", [src, 45, 5, 1, torch.zeros(2, 9, 16), 144, 16, 3, 2, 9, 3])
    assert e == 0.0
    e = _run_call(dev, "srn_transpose_ct", [rnd(2, 80, 37, seed=41), (torch.zeros(2, 37, 96), 8), 2, 80, 37, 80 * 37,
                                            37, 37 * 96, 96])
    assert e == 0.0
    one = torch.ones(80)
    e = _run_call(dev, "srn_renorm", [rnd(50, 80, seed=42), one * 0.9, 0.1 * rnd(80, seed=43), 0.1 * rnd(80, seed=44),
                                      one * 1.1, torch.zeros(50, 80), 50, 80])
    assert e < 1e-6
    for C2, k in ((32, 7), (16, 5)):
        e = _run_call(dev, "srn_out_conv_tanh", [rnd(2, 300, C2, seed=45), rnd(k, C2, seed=46) * 0.2, rnd(1, seed=47),
                                                 torch.zeros(2, 300), 2, 300, C2, k, 0.01])
        assert e < KTOL.k


def test_gst_kernels(dev):
    # recurrence on a precomputed input projection, attention on precomputed K / V
    e = _run_call(dev, "srn_gru_recur_last", [rnd(3, 5, 384, seed=70), rnd(128, 384, seed=71) / 11,
                                              0.1 * rnd(384, seed=72), torch.zeros(3, 128), 3, 5, 128])
    assert e < KTOL.k
    a = [rnd(2, 128, seed=73), rnd(128, 256, seed=74) / 11, 0.1 * rnd(256, seed=75), rnd(50, 256, seed=76),
         rnd(50, 256, seed=77), rnd(256, 256, seed=78) / 16, 0.1 * rnd(256, seed=79), torch.zeros(2, 256), 2, 128, 50,
         256, 4]
    assert _run_call(dev, "srn_style_token_attention_kv", a) < KTOL.k


# ------------------------------------------------------------------------------------------------
#  model-level parity against the reference's golden vectors and the oracle
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    m = models.Serenade(**SERENADE_PARAMS)
    m.load_state_dict(serenade_weights())
    return m.eval().to(dev)


@pytest.fixture(scope="module")
def voc(dev):
    w, params = hifigan_weights()
    g = vocoder.HiFiGANGenerator(**params)
    from serenade_amd import _shapes
    g.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**params, weight_norm=True)), seed=0))
    one = np.ones(80, dtype=np.float32)
    return vocoder.Vocoder.from_generator(g, {"sampling_rate": 24000}, {"mean": 0 * one, "scale": one}, dev,
                                          trg_stats={"mean": 0 * one, "scale": one}), w, params


@pytest.mark.parametrize("tag", ["L48", "L65"])
def test_decoder_forward_golden(dev, model, golden, tag):
    g = golden("decoder_" + tag)
    mask = O.make_non_pad_mask(g["lens"].tolist()).unsqueeze(1).to(dev)
    out = model.cfm_decoder.estimator(T(g["x"]).to(dev), mask, T(g["mu"]).to(dev), T(g["t"]).to(dev),
                                      T(g["spk"]).to(dev))
    assert nerr(out, g["out"]) < KTOL.model


def test_euler_golden(dev, model, golden):
    g = golden("euler_L48")
    mask = O.make_non_pad_mask(g["lens"].tolist()).unsqueeze(1).to(dev)
    out = model.cfm_decoder.solve_euler(T(g["z"]).to(dev), torch.linspace(0, 1, 11), T(g["mu"]).to(dev), mask,
                                        T(g["spk"]).to(dev))
    assert nerr(out, g["out"]) < MEL_RTOL


def test_encoder_gst_golden(dev, model, golden):
    g = golden("encoder")
    assert nerr(model.encoder(T(g["x"]).to(dev)), g["y"]) < 5 * KTOL.k
    g = golden("gst")
    assert nerr(model.gst(T(g["speech"]).to(dev)), g["style"]) < 5e-5


def _infer(model, d, dev, **kw):
    g = lambda k: d[k].to(dev)
    return model.inference(g("x"), d["lengths"], g("midi"), g("lft"), g("ref_x"), d["ref_lengths"], g("ref_logmel"),
                           g("ref_midi"), g("ref_lft"), **kw)


def test_inference_and_vocoder_golden(dev, model, voc, golden):
    g, gh = golden("inference"), golden("hifigan")
    d = synth_inputs(1, 64, T_ref=16, seed=4321)
    mel = _infer(model, d, dev, noise=(d["z"] / 0.667) * 0.667)
    assert mel.shape == (64, 80) and nerr(mel, g["mel_b1"]) < MEL_RTOL
    wave, sr = voc[0].decode(mel)
    assert sr == 24000 and wave.shape == (64 * 240,)
    assert (wave.cpu() - T(gh["wave_b1"])).abs().max().item() < WAVE_ATOL
    d = synth_inputs(2, 40, T_ref=16, seed=4322, lengths=[40, 29])
    mel2 = _infer(model, d, dev, noise=(d["z"] / 0.667) * 0.667)
    assert nerr(mel2, g["mel_b2"]) < MEL_RTOL
    y = voc[0].model(T(gh["c"]).to(dev))
    assert nerr(y, gh["y"]) < KTOL.model


def test_hifigan_small_variant_golden(dev, golden):
    g = golden("hifigan_small")
    w, params = hifigan_weights(seed=1, small=True)
    gen = vocoder.HiFiGANGenerator(**dict(params, use_weight_norm=False))
    gen.load_state_dict(w)
    y = gen.to(dev)(T(g["c"]).to(dev))
    assert nerr(y, g["y"]) < KTOL.model


def test_cpu_generator_noise_matches_reference_semantics(dev, model):
    d = synth_inputs(1, 24, T_ref=16, seed=7)
    torch.manual_seed(11)
    a = _infer(model, d, dev)
    torch.manual_seed(11)
    z = torch.randn((1, 80, 40)) * 0.667
    b = _infer(model, d, dev, noise=z)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
#  BASELINE.json sizes: oracle on one utterance + size-independent properties
# ------------------------------------------------------------------------------------------------
def test_full_size_batch_parity_and_properties(dev, model, voc):
    """C2/C3 shape (B=8, T=1024, T_ref=256, 10 Euler steps + HiFi-GAN).
    (1) utterance 3 of the batch equals the CPU oracle on that utterance alone (mel 1e-3 rel, wave 1e-4 abs);
    (2) per-utterance independence: the batched result equals a B=1 run of the same utterance;
    (3) determinism: two runs are bit-identical."""
    B, Tn, Tr = 8, 1024, 256
    d = synth_inputs(B, Tn, T_ref=Tr, seed=1235)
    mel = _infer(model, d, dev, noise=d["z"])
    assert mel.shape == (B, Tn, 80) and torch.isfinite(mel).all()
    mel_again = _infer(model, d, dev, noise=d["z"])
    assert torch.equal(mel, mel_again)
    wave = voc[0].decode_batch(mel)
    assert wave.shape == (B, Tn * 240) and torch.isfinite(wave).all()
    i = 3
    one = {k: v[i:i + 1] for k, v in d.items()}
    mel1 = _infer(model, one, dev, noise=one["z"])
    assert nerr(mel1, mel[i]) < 1e-5
    w = serenade_weights()
    ref = O.serenade_inference(w, one["x"], one["lengths"], one["midi"], one["lft"], one["ref_x"], one["ref_lengths"],
                               one["ref_logmel"], one["ref_midi"], one["ref_lft"], one["z"])
    assert nerr(mel[i], ref) < MEL_RTOL
    id80 = {"mean": torch.zeros(80), "scale": torch.ones(80)}
    wref = O.vocoder_decode(voc[1], ref, voc[2], id80, id80)
    assert (wave[i].cpu() - wref).abs().max().item() < WAVE_ATOL


def test_ragged_batch_padding_invariance(dev, model):
    """An utterance's converted frames must not depend on the padding it is batched with
    (every per-frame op is masked; GroupNorm statistics include padded frames *of its own row only*)."""
    d = synth_inputs(2, 96, T_ref=32, seed=99, lengths=[96, 61])
    mel = _infer(model, d, dev, noise=d["z"])
    w = serenade_weights()
    ref = O.serenade_inference(w, d["x"], d["lengths"], d["midi"], d["lft"], d["ref_x"], d["ref_lengths"],
                               d["ref_logmel"], d["ref_midi"], d["ref_lft"], d["z"])
    assert nerr(mel, ref) < MEL_RTOL


def test_long_form_T4096_runs_and_matches_oracle_prefix(dev, model):
    """C5 shape per GPU (T=4096, L=4352): finite output; cheap oracle check on the estimator alone."""
    B, L = 1, 4352
    rng = np.random.default_rng(5)
    x = T(rng.standard_normal((B, 80, L)).astype(np.float32))
    mu = T(rng.standard_normal((B, 162, L)).astype(np.float32))
    spk = T(rng.standard_normal((B, 256)).astype(np.float32))
    mask = torch.ones(B, 1, L, dtype=torch.bool)
    out = model.cfm_decoder.estimator(x.to(dev), mask.to(dev), mu.to(dev), torch.tensor(0.5), spk.to(dev))
    ref = O.decoder_forward(sub(serenade_weights(), "cfm_decoder.estimator."), x, mask, mu, torch.tensor(0.5), spk)
    assert nerr(out, ref) < KTOL.model


def test_training_forward_values_golden(dev, model, golden):
    """a1' Serenade.forward (loss values; per-sample time embedding) on the reference's own random draws."""
    g = golden("forward")
    draws = {"uniform": float(g["uniform"]), "seg_start": int(g["seg_start"]), "t": T(g["t"]).to(dev),
             "z": T(g["z"]).to(dev)}
    ret = model(T(g["x"]).to(dev), T(g["lens"]), T(g["logmel"]).to(dev), T(g["midi"]).to(dev), T(g["lft"]).to(dev),
                draws=draws)
    assert nerr(ret["gauss_mel"], g["gauss_mel"]) < 5 * KTOL.k
    assert abs(ret["prior_loss"].item() / float(g["prior_loss"]) - 1) < 1e-4
    assert abs(ret["cfm_loss"].item() / float(g["cfm_loss"]) - 1) < 1e-3


def test_transposed_tail_epilogue(dev):
    """QKV projection: columns >= out_tr_col0 land in out_tr[b][c - col0][t] (V^T), the rest row-major in out"""
    B, Tn, K, N, c0 = 2, 203, 64, 192, 128
    Tp = 224
    kw = dict(in0=rnd(B, Tn, K, seed=41), w=rnd(N, K, seed=42), bias=rnd(N, seed=43), out=torch.zeros(B, Tn, N),
              n_batch=B, T_in=Tn, T_out=Tn, C_in=K, N=N, in0_bs=Tn * K, ld_in0=K, ldw=K, out_bs=Tn * N, ld_out=N,
              out_tr=torch.zeros(B, N - c0, Tp), out_tr_col0=c0, out_tr_bs=(N - c0) * Tp, ld_out_tr=Tp,
              len_out=torch.tensor([203, 90], dtype=torch.int32))
    run_conv_both(dev, kw, tiles=(0, 1, 3, 4))
    m = Mirror(dev)
    g = {k: m(v) for k, v in kw.items()}
    ops.ConvOp(**g)()
    ref = kw["in0"] @ kw["w"].t() + kw["bias"]
    ref[1, 90:] = 0
    assert nerr(g["out"][:, :, :c0], ref[:, :, :c0]) < KTOL.k and g["out"][:, :, c0:].abs().max().item() == 0
    assert nerr(g["out_tr"][:, :, :Tn], ref[:, :, c0:].transpose(1, 2)) < KTOL.k
    assert g["out_tr"][:, :, Tn:].abs().max().item() == 0  # pad columns are never written


def test_hipgraph_replay_is_bitwise_the_eager_run(dev, model, voc):
    """ops.set_graphs(True): the plans (Euler loop, HiFi-GAN) replay as captured hipGraphs -- same launches, same bits"""
    d = synth_inputs(2, 72, T_ref=24, seed=77, lengths=[72, 50])
    outs = []
    try:
        for graphs in (False, True):
            ops.set_graphs(graphs)
            for m in model.modules():  # fresh plans, so the graph arm captures its own
                if hasattr(m, "_plans"):
                    m._plans = {}
            for _ in range(3):  # eager warm-up call, capturing call, replay
                mel = _infer(model, d, dev, noise=d["z"])
                wave = voc[0].decode_batch(mel)
            outs.append((mel.cpu(), wave.cpu()))
    finally:
        ops.set_graphs(False)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_bf16x6_is_as_accurate_as_the_fp32_mfma(dev, precision):
    """the claim behind the `fp32_emulated_bf16x6_mode` bench line: against an fp64 reference a K = 2048 contraction in
    bf16x6 (exact hi + mid + lo split, 6 bf16 MFMAs per product, fp32 accumulate) is no less accurate than the exact-fp32
    MFMA chain (both are limited by their fp32 accumulation order), and ~10x more accurate than bf16x3"""
    if precision != "fp32":
        pytest.skip("one arm: the test sets the modes itself")
    M, N, K = 512, 512, 2048
    x, w = rnd(1, M, K, seed=11), rnd(N, K, seed=12)
    ref = (x[0].double() @ w.double().t())
    errs = {}
    for mode in ("fp32", "bf16x6", "bf16x3"):
        serenade_amd.set_precision(mode)
        out = torch.zeros(1, M, N, device=dev)
        ops.ConvOp(in0=x.to(dev), w=w.to(dev), out=out, n_batch=1, T_in=M, T_out=M, C_in=K, N=N, in0_bs=M * K, ld_in0=K,
                   ldw=K, out_bs=M * N, ld_out=N)()
        d = (out[0].cpu().double() - ref).abs()
        errs[mode] = (d.max().item() / ref.abs().max().item(), d.pow(2).mean().sqrt().item() / ref.pow(2).mean().sqrt().item())
    serenade_amd.set_precision("fp32")
    assert errs["bf16x6"][0] <= 1.5 * errs["fp32"][0] and errs["bf16x6"][1] <= 1.5 * errs["fp32"][1], errs
    assert errs["bf16x6"][1] < 1e-6 and errs["bf16x3"][1] > 3 * errs["bf16x6"][1], errs
