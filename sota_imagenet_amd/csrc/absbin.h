// absbin.h — the bins of the |x| histogram behind callbacks.GradDistributionTB (optim_hist.hip), stated once for the kernels; ops.py states the
// same three numbers for the host (ABSBIN_BINS, ABSBIN_SHIFT, ABSBIN_K0) and tests/test_grad_dist_host.py holds the two together.
//   key(x) = the 32 bits of the float with the sign bit cleared: ordered like |x|, NaN above every number
//   bin(x) = clamp((key >> 20) - K0, 0, 511): the 8 exponent bits and the top 3 mantissa bits, i.e. eight bins per octave, linear in the mantissa
// The lower edge of bin b >= 1 is the float with bits (K0 + b) << 20.  K0 = (77 << 3) + 2: the float with bits K0 << 20 is 2^-50 * 1.25 = 1.1102e-15,
// the smallest edge of this grid above the 1e-15 the reference clamps its log10 at, and bin 0 is everything whose key >> 20 is at most K0, i.e.
// everything below bin 1's edge 2^-50 * 1.375 = 1.2212e-15: zeros, -0.0, denormals, whatever the reference shows as -15 and the sliver up to
// 1.2212e-15 that this grid does not tell apart from it.  Bin 511 starts at 2^14 * 1.125 and also takes infinities and NaN.
#pragma once
#include <cstdint>

namespace mi355 {

constexpr int kAbsBinBins = 512;
constexpr int kAbsBinShift = 20;
constexpr int kAbsBinK0 = (77 << 3) + 2;

#if defined(__HIPCC__)
__host__ __device__
#endif
inline int absbin_of_bits(uint32_t bits) {
  const int b = (int)((bits & 0x7fffffffu) >> kAbsBinShift) - kAbsBinK0;
  return b < 0 ? 0 : (b > kAbsBinBins - 1 ? kAbsBinBins - 1 : b);
}

}  // namespace mi355
