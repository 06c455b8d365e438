// fastdiv.h -- the magic-number division that places every tile of conv_f32.hip and resunit_f32.hip.  Includes only
// <stdint.h> and hides the device qualifiers from a plain host compiler, so tests/test_fastdiv.py compiles this very
// file into its probe.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SRN_FDIV_DEVICE __device__ __forceinline__
#else
#define SRN_FDIV_DEVICE inline
#endif

// n / d == (n * mul) >> shift for 0 <= n < 2^26 (host: make_fdiv); scalar operands stay on the scalar ALU
struct FDiv {
  uint32_t mul, shift;
};
SRN_FDIV_DEVICE int fdiv(const int n, const FDiv d) {
  return (int)(((uint64_t)(uint32_t)n * d.mul) >> d.shift);
}

// mul = ceil(2^k / d), k = 26 + ceil(log2 d); 1 <= d < 2^26
inline FDiv make_fdiv(const uint32_t d) {
  int lg = 0;
  while ((1u << lg) < d) ++lg;
  const int k = 26 + lg;
  return FDiv{(uint32_t)(((1ull << k) + d - 1) / d), (uint32_t)k};
}
