"""Every answer of srn_conv_gemm's kernel choice, from two builds of the library side by side:

    python tools/routediff.py OLD.so NEW.so [N]

srn_conv_gemm_route (return code, error text, family / tile / K slices) and srn_conv_gemm_workspace_bytes on
tests.test_conv_route.sweep(N = 100000), each shape under route 0 .. 5 and tile 0 .. 12; on the params of every case of
the kernel-form sweep (tests/_conv_cases.py) as a GPU build fills them; and on its rejects.  Prints the counts and exits
with 1 on any difference.  Host only: no device is touched.  Run it before and after a change to conv_route.
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from serenade_amd import _lib, ops  # noqa: E402
from tests import _conv_cases as C  # noqa: E402
from tests.test_conv_route import device_params, sweep  # noqa: E402


def load(path):
    h = ctypes.CDLL(os.path.abspath(path))
    for name in ("srn_conv_gemm_route", "srn_conv_gemm_workspace_bytes", "srn_last_error"):
        getattr(h, name).restype, getattr(h, name).argtypes = _lib._SIGS[name]
    return h


def answer(h, p):
    out = (ctypes.c_int32 * 3)()
    rc = h.srn_conv_gemm_route(ctypes.byref(p), out)
    return rc, (tuple(out) if rc == 0 else h.srn_last_error()), h.srn_conv_gemm_workspace_bytes(ctypes.byref(p))


def main(old, new, n=100000):
    old, new = load(old), load(new)
    asked = differ = 0

    def ask(p, what):
        nonlocal asked, differ
        a, b = answer(old, p), answer(new, p)
        asked += 1
        if a != b:
            differ += 1
            if differ <= 20:
                print("DIFFERS", what, a, b)

    for i, p in enumerate(sweep(n)):
        for route in range(6):
            for tile in range(13):
                p.route, p.tile = route, tile
                ask(p, f"sweep {i} route {route} tile {tile}")
    print(f"sweep: {asked} params asked, {differ} differ", flush=True)
    for form, vid in C.all_ids():
        args, _ = C.materialize(C.make(form, vid))
        ask(device_params(ops.ConvOp(**C.kwargs(args))), f"case {form} {vid}")
    for rid, *_ in C.rejects():
        case, edit = C.reject_case(rid)
        op = ops.ConvOp(**C.kwargs(C.materialize(case)[0]))
        if edit is not None:
            edit(op.p)
        ask(op.p, f"reject {rid}")
    print(f"with {len(C.all_ids())} sweep cases and {len(C.rejects())} rejects: {asked} params asked, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], *map(int, sys.argv[3:4])))
