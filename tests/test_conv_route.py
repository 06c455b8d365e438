"""CPU checks of srn_conv_gemm's kernel choice (conv_gemm.hip's conv_route, exported as srn_conv_gemm_route): which
kernel family, tile id and K-slice count every contraction of the inference plans and of the training step's forward
gets, against the committed table tests/conv_routes.json; invariants of the route over a sweep of shapes; and the
kernel forms the library lists (srn_conv_gemm_forms: what its launch and its route read) against the committed snapshot
tests/conv_forms.json.

The plans are built under the kernel emulator (tests/_emulator.py); the route is asked for each ConvOp's params as the
GPU build would fill them: weight planes attached in the split-bf16 modes and the split-K workspace attached where the
library asks for one (ops.ConvOp._build).

    python -m tests.test_conv_route         # prints the table for tests/conv_routes.json
    python -m tests.test_conv_route forms   # prints the snapshot for tests/conv_forms.json
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import serenade_amd
from serenade_amd import _lib, _shapes, models, ops, training, vocoder
from serenade_amd.utils.synth import HIFIGAN_PARAMS, SERENADE_PARAMS, fill_state_dict
from tests import _emulator
from tests._weights import serenade_weights, sub

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_routes.json")
FORMS_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_forms.json")
FAMILY = {_lib.FAMILY_GENERIC: "generic", _lib.FAMILY_F32: "f32", _lib.FAMILY_FAST: "fast", _lib.FAMILY_HALO: "halo",
          _lib.FAMILY_STRIP: "strip"}
# (plan, precision): inference plans of bench.py's headline (B = 8 x T = 1024, 256 prompt frames) and its B = 1 x T = 256
# line; the training step's forward at B = 2 x L = 256
CONFIGS = [(plan, prec) for plan in ("B8xT1024", "B1xT256") for prec in ("fp32", "bf16x3", "bf16x6")] + [("train", "fp32")]


@pytest.fixture(scope="module")
def lib():
    from serenade_amd import build
    build.build(verbose=False)  # no-op when up to date; hipcc cross-compiles without a GPU
    return _lib.lib()


def route(p):
    """(family name, tile, K slices) of one params struct; raises on a validation error"""
    out = (ctypes.c_int32 * 3)()
    _lib.check(_lib.lib().srn_conv_gemm_route(ctypes.byref(p), out), "srn_conv_gemm_route")
    return FAMILY[out[0]], out[1], out[2]


def device_params(op):
    """op.p as ops.ConvOp._build fills it on a GPU: weight planes of static k-major weights in the split-bf16 modes,
    then the split-K workspace wherever the library asks for one"""
    p = _lib.SrnConvParams.from_buffer_copy(op.p)
    if (p.precision in (_lib.PREC_BF16X3, _lib.PREC_BF16X6) and isinstance(op.kw["w"], torch.Tensor) and p.w_bs == 0
            and p.w_hs == 0 and not p.w_nmajor):
        p.w_hi = p.w  # any 16-byte aligned address: the route only asks whether there is one
        if p.precision == _lib.PREC_BF16X6:
            p.w_lo = p.w
    if ops.SPLITK and _lib.lib().srn_conv_gemm_workspace_bytes(ctypes.byref(p)) > 0:
        p.ws, p.ws_bytes = p.out, ops.SPLITK_WS_BYTES
    return p


def key(p):
    """the fields of a contraction the route may look at, as one short string"""
    span = max(p.tap_off[:p.n_taps]) - min(p.tap_off[:p.n_taps])
    k = f"{p.n_batch}x{p.n_head} T{p.T_out} N{p.N} C{p.C_in}"
    k += f"/{p.C_in0}" if 0 < p.C_in0 < p.C_in else ""
    k += f" k{p.n_taps}" + (f"s{span}" if p.n_taps > 1 else "") + (f" st{p.in_stride}" if p.in_stride > 1 else "")
    for flag, name in ((p.geglu, "geglu"), (p.w_nmajor, "nmaj"), (p.pad_reflect, "refl"), (p.gn_partials, "gn"),
                       (p.out_tr, "tr"), (p.res_mode, "res"), (p.w_bs or p.w_hs, "wz"), (p.C_w and p.C_w != p.C_in, "cw"),
                       (p.pro_act, f"act{p.pro_act}"), (p.ldw != p.n_taps * p.C_in, "ldw")):
        if flag:
            k += " " + name
    return k


class _Collect:
    """records every ConvOp built inside the block"""

    def __enter__(self):
        self.ops, self._init = [], ops.ConvOp.__init__
        init = self._init

        def rec(op, **kw):
            init(op, **kw)
            self.ops.append(op)
        ops.ConvOp.__init__ = rec
        return self

    def __exit__(self, *exc):
        ops.ConvOp.__init__ = self._init


def plan_ops(plan, prec):
    serenade_amd.set_precision(prec)
    try:
        with _emulator.installed(), _Collect() as c:
            if plan == "train":
                g = torch.Generator().manual_seed(0)
                B, L = 2, 256
                est = training.Estimator(sub(serenade_weights(), "cfm_decoder.estimator."), torch.device("cpu"))
                mask = torch.ones(B, 1, L)
                training.cfm_loss(est, torch.randn(B, 80, L, generator=g), mask, torch.randn(B, 162, L, generator=g),
                                  torch.randn(B, 256, generator=g), mask,
                                  draws={"t": torch.rand(B, 1, 1, generator=g), "z": torch.randn(B, 80, L, generator=g)})
            else:
                B, T = {"B8xT1024": (8, 1024), "B1xT256": (1, 256)}[plan]
                model = models.Serenade(**SERENADE_PARAMS)
                model.load_state_dict(serenade_weights())
                ip = model.eval()._inference_plan(B, T, 256, 10)
                ip.pl.set_schedule(*ip._sched)  # the Euler steps' op lists are built with the schedule
                gen = vocoder.HiFiGANGenerator(**HIFIGAN_PARAMS)
                gen.load_state_dict(fill_state_dict(_shapes.as_meta(_shapes.hifigan_shapes(**HIFIGAN_PARAMS, weight_norm=True))))
                gen.plan(B, T)
        return c.ops
    finally:
        serenade_amd.set_precision("fp32")


def routes(plan, prec):
    """{key: "family tile ksplit"} over the ConvOps of one configuration"""
    out = {}
    for op in plan_ops(plan, prec):
        p = device_params(op)
        fam, tile, ks = route(p)
        r = f"{fam} {tile} {ks}"
        k = key(p)
        assert out.setdefault(k, r) == r, f"{plan} {prec}: {k} gets {out[k]} and {r}"
    return dict(sorted(out.items()))


@pytest.mark.parametrize("plan,prec", CONFIGS)
def test_plan_routes_match_the_table(lib, plan, prec):
    want = json.load(open(TABLE))[f"{plan} {prec}"]
    got = routes(plan, prec)
    diff = {k: (want.get(k), got.get(k)) for k in set(want) | set(got) if want.get(k) != got.get(k)}
    assert not diff, diff


def test_route_validates_like_the_launch(lib):
    out = (ctypes.c_int32 * 3)()
    p = _lib.SrnConvParams()
    assert lib.srn_conv_gemm_route(ctypes.byref(p), out) == -1
    assert b"null in0" in lib.srn_last_error()
    assert lib.srn_conv_gemm_route(None, out) == -1
    assert b"null params" in lib.srn_last_error()


@functools.lru_cache(maxsize=None)
def library_forms():
    """the rows of srn_conv_gemm_forms: every kernel form the launchers' lists hold, in the library's order"""
    from serenade_amd import build
    build.build(verbose=False)  # no-op when up to date
    return _lib.conv_forms()


def form_rows(fam, p):
    """the library's rows a launch of family `fam` is looked up in for p's arithmetic and B layout (the generic
    family's fp32 rows run bf16x6 too)"""
    prec = _lib.PREC_FP32 if fam == "generic" and p.precision == _lib.PREC_BF16X6 else p.precision
    return [f for f in library_forms() if FAMILY[f.family] == fam and f.precision == prec and f.nmajor == p.w_nmajor]


def forms_snapshot():
    """what tests/conv_forms.json holds: the library's rows, and the names of the forms the sweep makes of them"""
    from tests import _conv_cases
    return {"fields": list(_lib.ConvForm._fields), "rows": [[FAMILY[f.family], *f[1:]] for f in library_forms()],
            "sweep": list(_conv_cases.forms())}


def test_library_forms_match_the_snapshot(lib):
    """a row lost or added by accident changes the cases and the expectation of the sweep alike: the snapshot does not
    move with it"""
    want = json.load(open(FORMS_TABLE))
    got = forms_snapshot()
    assert got["fields"] == want["fields"]
    assert got["rows"] == want["rows"], [r for r in got["rows"] + want["rows"] if (r in got["rows"]) != (r in want["rows"])]


def sweep(n, seed=0):
    """random contractions of the path's kinds: taps / dilation, stride 2, concat input, GEGLU, n-major B, thin
    channels, small grids, heads, weight planes, residuals, GroupNorm partials; those the validation refuses are
    left out"""
    rng = np.random.default_rng(seed)
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    buf = torch.zeros(64)
    a = buf.data_ptr()
    for _ in range(n):
        p = _lib.SrnConvParams()
        p.n_batch, p.n_head = pick([1, 1, 2, 4, 8, 16]), pick([1, 1, 1, 4])
        p.in_stride = pick([1, 1, 1, 2])
        p.T_out = pick([1, 7, 32, 64, 100, 256, 333, 640, 1024, 1280, 4096, 40000])
        p.T_in = p.T_out * p.in_stride
        p.C_in = pick([4, 20, 32, 64, 80, 96, 128, 256, 512, 1024, 1536])
        p.N = pick([4, 8, 32, 48, 64, 80, 128, 160, 256, 512, 1024, 2048, 3072])
        k, d = pick([1, 1, 2, 3, 3, 5, 7, 11]), pick([1, 1, 2, 3, 5])
        p.w_nmajor = int(rng.integers(6) == 0)
        p.n_taps = 1 if p.w_nmajor else k
        for i in range(p.n_taps):
            p.tap_off[i] = (i - (p.n_taps - 1) // 2) * d
        p.pad_reflect = int(rng.integers(8) == 0)
        p.geglu = int(rng.integers(5) == 0 and p.N % 64 == 0)
        p.pro_act, p.pro_slope = pick([0, 0, 1, 1, 2, 3]), pick([0.0, 0.1, 0.2, 1.5])
        p.precision = pick([_lib.PREC_FP32, _lib.PREC_BF16X3, _lib.PREC_BF16X6])
        p.in0 = p.w = p.out = a
        p.ld_in0 = p.C_in
        if p.C_in % 32 == 0 and p.C_in >= 64 and rng.integers(5) == 0:
            p.C_in0 = 32 * int(rng.integers(1, p.C_in // 32))
            p.in1, p.ld_in0, p.ld_in1 = a, p.C_in0, p.C_in - p.C_in0
        p.ldw = p.N if p.w_nmajor else p.n_taps * p.C_in
        if rng.integers(8) == 0:
            p.w_bs = p.ldw * p.N
        p.ld_out = p.N
        if not p.geglu and rng.integers(4) == 0:
            p.res_mode, p.res, p.ld_res = _lib.RES_ADD, a, p.N
        if not p.geglu and p.N % 32 == 0 and rng.integers(5) == 0:
            p.gn_partials = a
        if p.precision != _lib.PREC_FP32 and rng.integers(3):
            p.w_hi = a
            p.w_lo = a if rng.integers(2) else None
        if rng.integers(2):
            p.ws, p.ws_bytes = a, pick([1000, ops.SPLITK_WS_BYTES])
        if _lib.lib().srn_conv_gemm_route(ctypes.byref(p), (ctypes.c_int32 * 3)()) == 0:
            yield p


def test_route_invariants_over_a_sweep(lib):
    seen = set()
    for p in sweep(4000):
        fam, tile, ks = route(p)
        seen.add((fam, tile, ks > 1))
        rows = form_rows(fam, p)
        assert tile in {f.tile for f in rows}, (key(p), p.precision, fam, tile)
        assert ks == 1 or (fam in ("f32", "fast") and p.ws and p.ws_bytes >= ks * p.n_batch * p.n_head * p.T_out * p.N * 4)
        assert fam not in ("halo", "strip") or p.precision == _lib.PREC_BF16X3
        assert fam != "f32" or p.precision == _lib.PREC_FP32
        if ks > 1:
            assert [tile] == [f.tile for f in rows if f.kslices] and 2 <= ks <= 8
        if ks > 1:  # the workspace query asks the same route
            assert lib.srn_conv_gemm_workspace_bytes(ctypes.byref(p)) == ks * p.n_batch * p.n_head * p.T_out * p.N * 4
    # the sweep reaches every family, the split-K slices of both and the single-stage / split-step tiles
    for want in [("generic", 4, False), ("halo", 1, False), ("strip", 0, False), ("f32", 7, False), ("f32", 9, False),
                 ("f32", 10, False), ("f32", 11, True), ("fast", 4, True), ("fast", 7, False)]:
        assert want in seen, want


def test_forced_routes_and_tiles(lib):
    """the test / A-B routes keep their meaning; a forced tile a family lacks runs its twin from the tile table"""
    for p in sweep(2000, seed=1):
        p.route = _lib.ROUTE_GENERIC
        assert route(p)[0] == "generic"
        p.route = _lib.ROUTE_FAST_FP32
        assert route(p)[0] != "f32"
        p.route = _lib.ROUTE_TILED
        assert route(p)[0] not in ("halo", "strip")
        p.route = _lib.ROUTE_AUTO
        p.ws = None
        if p.w_nmajor or p.pro_act > 1 or p.geglu:
            continue
        for tile, twin in ((7, 4), (9, 3), (10, 4), (11, 4)):
            p.tile = tile
            fam, got, _ = route(p)
            if fam == "fast" and p.precision == _lib.PREC_BF16X3:
                assert got == twin
            if fam == "generic":
                assert got == twin
        for tile, twin in ((6, 1), (8, 2)):  # ids without a kernel of their own
            p.tile = tile
            fam, got, _ = route(p)
            if fam in ("fast", "generic"):
                assert got == twin
        p.tile = 12  # an id the table does not know: refused, unless the strip kernel (no tile ids) takes the shape
        rc = lib.srn_conv_gemm_route(ctypes.byref(p), (ctypes.c_int32 * 3)())
        assert rc == -1 or route(p)[0] == "strip"


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["forms"]:
        snap = forms_snapshot()
        lines = ",\n  ".join(json.dumps(r) for r in snap["rows"])
        print('{\n "fields": %s,\n "rows": [\n  %s\n ],\n "sweep": %s\n}'
              % (json.dumps(snap["fields"]), lines, json.dumps(snap["sweep"], indent=1).replace("\n", "\n ")))
    else:
        print(json.dumps({f"{plan} {prec}": routes(plan, prec) for plan, prec in CONFIGS}, indent=1))
