"""The magic-number division of csrc/fastdiv.h (make_fdiv: n / d == (n * mul) >> shift for 0 <= n < 2^26,
mul = ceil(2^k / d), k = 26 + ceil(log2 d)), as conv_f32.hip and resunit_f32.hip use it, checked exhaustively near every
boundary: the kernels derive tile coordinates from it on the scalar unit, so a wrong quotient would silently mis-place a
tile.  The (mul, shift) pairs come from the header itself, compiled into a host probe with the system compiler."""
import os
import random
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "serenade_amd", "csrc")

PROBE = """#include <stdio.h>
#include "fastdiv.h"
int main() {
  unsigned d;
  while (scanf("%u", &d) == 1) {
    const FDiv f = make_fdiv(d);
    printf("%u %u\\n", f.mul, f.shift);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler for the fastdiv.h probe"
    tmp = tmp_path_factory.mktemp("fastdiv")
    (tmp / "probe.cpp").write_text(PROBE)
    exe = tmp / "probe"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(tmp / "probe.cpp")])

    def make_fdivs(ds):
        out = subprocess.check_output([str(exe)], input=" ".join(str(d) for d in ds).encode()).split()
        assert len(out) == 2 * len(ds)
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(len(ds))]

    return make_fdivs


def closed_form(d):
    lg = 0
    while (1 << lg) < d:
        lg += 1
    k = 26 + lg
    return ((1 << k) + d - 1) // d, k


def test_fastdiv_is_exact_below_2_pow_26(probe):
    rng = random.Random(7)
    ds = list(range(1, 300)) + [2 ** i + j for i in range(2, 26) for j in (-1, 0, 1)] + [rng.randrange(1, 1 << 26) for _ in range(300)]
    for d, (mul, k) in zip(ds, probe(ds)):
        assert (mul, k) == closed_form(d), d
        assert mul < (1 << 32) and k < 64
        ns = {0, 1, d - 1, d, d + 1, (1 << 26) - 1}
        ns |= {q * d + r for q in (1, 2, 3, 1000, ((1 << 26) - 1) // d) for r in (-1, 0, 1)}
        ns |= {rng.randrange(0, 1 << 26) for _ in range(50)}
        for n in ns:
            if 0 <= n < (1 << 26):
                assert (n * mul) >> k == n // d, (n, d)
