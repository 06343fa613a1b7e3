// The host solve of the exposure fit (dvo_slam_amd/csrc/dvo_exposure_solve.h) as a stand-alone program, so that it can run under a
// sanitizer without anything being loaded into Python: tests/test_exposure.py compiles it with -fsanitize=undefined and feeds it
// sums at the 2^62 bound, where an overflow of the 128-bit products would hide.  One request per line of standard input:
//     s n sx sy sxx sxy syy min_pairs min_gain max_gain scale   ->   gain bias r2 (as %a) and the degenerate code
//     d <a decimal integer of up to 128 bits>                   ->   its conversion to double (as %a)
#include <cstdio>
#include <cstring>

#include "dvo_exposure_solve.h"

using namespace dvo_amd::exposure;

static wide parse_wide(const char *s) {
  const bool neg = *s == '-';
  if (neg) ++s;
  unsigned __int128 m = 0;
  for (; *s >= '0' && *s <= '9'; ++s) m = m * 10u + (unsigned)(*s - '0');
  return neg ? (wide)((unsigned __int128)0 - m) : (wide)m;
}

int main() {
  char line[512], digits[128];
  while (std::fgets(line, sizeof line, stdin)) {
    Sums S;
    long long min_pairs;
    double min_gain, max_gain, scale;
    if (line[0] == 's' && std::sscanf(line + 1, "%lld %lld %lld %lld %lld %lld %lld %lf %lf %lf", &S.n, &S.sx, &S.sy, &S.sxx, &S.sxy, &S.syy,
                                      &min_pairs, &min_gain, &max_gain, &scale) == 10) {
      const Fit f = solve(S, min_pairs, min_gain, max_gain, scale);
      std::printf("%a %a %a %d\n", f.gain, f.bias, f.r2, f.degenerate);
    } else if (line[0] == 'd' && std::sscanf(line + 1, "%127s", digits) == 1) {
      std::printf("%a\n", to_double(parse_wide(digits)));
    } else {
      std::fprintf(stderr, "bad request: %s", line);
      return 2;
    }
  }
  return 0;
}
