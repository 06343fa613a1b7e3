// The host solve of the exposure fit (include/dvo_amd.h, "Exposure compensation", rules 7 and 8): from the six exact integer sums
// of a pass to gain, bias, r2 and the degenerate code.  Plain C++ with no HIP in it, so that a stand-alone program can include it
// and run it under a sanitizer (tests/test_exposure.py builds one); dvo_exposure.cpp is its only user in the library.
//
// The three determinants are exact in 128 bits: with at most 2^22 pairs and |X|, |Y| <= 2^20,
//     n <= 2^22, |sx|, |sy| <= 2^42, sxx, syy, |sxy| <= 2^62
//     |n * sxx|, |sx * sx| <= 2^84,  |sy * sxx|, |sx * sxy| <= 2^104: every product and difference below stays inside 2^105.
#pragma once

#include <cmath>
#include <cstdint>

namespace dvo_amd {
namespace exposure {

typedef __int128 wide;

struct Sums {
  long long n, sx, sy, sxx, sxy, syy;
};

struct Fit {
  double gain, bias, r2;
  int degenerate;  // 0, or the code of rule 8
};

// (double) v, correctly rounded (round to nearest, ties to even) whatever the compiler's runtime does with a 128-bit integer: a
// magnitude of more than 64 bits is cut to its top 64 with the bits cut off ORed into the lowest one kept -- 64 > 53 + 2, so the
// hardware's conversion of that word rounds as it would have rounded the whole -- and scaled back by an exact power of two.
inline double to_double(wide v) {
  const bool neg = v < 0;
  const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  const std::uint64_t hi = (std::uint64_t)(m >> 64), lo = (std::uint64_t)m;
  double d;
  if (hi == 0) {
    d = (double)lo;
  } else {
    const int s = 64 - __builtin_clzll(hi);  // 1..64: the bits above the low word
    std::uint64_t top = (std::uint64_t)(m >> s);
    const unsigned __int128 cut = m & (((unsigned __int128)1 << s) - 1);
    if (cut != 0) top |= 1u;
    d = std::ldexp((double)top, s);
  }
  return neg ? -d : d;
}

// rule 7 and rule 8 of one pass; `scale` is the quantisation as a double
inline Fit solve(const Sums &S, long long min_pairs, double min_gain, double max_gain, double scale) {
  Fit f{1.0, 0.0, 0.0, 0};
  if (S.n < min_pairs) {
    f.degenerate = 1;
    return f;
  }
  const wide n = S.n, sx = S.sx, sy = S.sy, sxx = S.sxx, sxy = S.sxy, syy = S.syy;
  const wide det = n * sxx - sx * sx;
  if (det <= 0) {
    f.degenerate = 2;
    return f;
  }
  const wide ng = n * sxy - sx * sy;
  const wide nb = sy * sxx - sx * sxy;
  const wide dety = n * syy - sy * sy;
  const double ddet = to_double(det);
  const double gain = to_double(ng) / ddet;
  if (!std::isfinite(gain) || !(gain >= min_gain && gain <= max_gain)) {
    f.degenerate = 3;
    return f;
  }
  f.gain = gain;
  f.bias = (to_double(nb) / ddet) / scale;
  f.r2 = dety <= 0 ? 0.0 : (to_double(ng) / ddet) * (to_double(ng) / to_double(dety));
  return f;
}

}  // namespace exposure
}  // namespace dvo_amd
