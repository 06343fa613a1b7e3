// The host-only launch rules (dvo_slam_amd/csrc/dvo_launch_rules.h) as a stand-alone program: no HIP, built by
// tests/test_launch_rules.py with -fsanitize=address,undefined -fno-sanitize-recover=all.  Every line of standard input is one of
//   grid n gx block           -> gy
//   rows T[0..15] | rows null -> the 12 floats of rows_from_column_major as hexadecimal bit patterns
//   inverse T[0..15] | inverse null -> ... of inverse_rows
//   relative A[0..15] B[0..15]      -> ... of relative_rows
// (doubles as strtod reads them: hex floats).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dvo_launch_rules.h"

namespace {

// up to `want` doubles from `at`; the number read
int doubles(const char *at, double *v, int want) {
  int got = 0;
  for (; got < want; ++got) {
    char *end = nullptr;
    v[got] = std::strtod(at, &end);
    if (end == at) break;
    at = end;
  }
  return got;
}

void print_rows(const float M[12]) {
  for (int i = 0; i < 12; ++i) {
    unsigned bits;
    std::memcpy(&bits, &M[i], sizeof bits);
    std::printf("%08x%c", bits, i == 11 ? '\n' : ' ');
  }
}

}  // namespace

int main() {
  using namespace dvo_amd::host;
  char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    char word[16] = "";
    int used = 0;
    if (std::sscanf(line, "%15s%n", word, &used) != 1) continue;
    const char *rest = line + used;
    double v[32];
    float M[12];
    if (!std::strcmp(word, "grid")) {
      long long n = 0;
      unsigned gx = 0;
      int block = 0;
      if (std::sscanf(rest, "%lld %u %d", &n, &gx, &block) != 3) return 2;
      std::printf("%u\n", grid_rows(n, gx, block));
      continue;
    }
    const bool null = std::strstr(rest, "null") != nullptr;
    const int want = !std::strcmp(word, "relative") ? 32 : 16;
    if (!null && doubles(rest, v, want) != want) {
      std::fprintf(stderr, "a `%s` line without its %d values\n", word, want);
      return 2;
    }
    if (!std::strcmp(word, "rows"))
      rows_from_column_major(null ? nullptr : v, M);
    else if (!std::strcmp(word, "inverse"))
      inverse_rows(null ? nullptr : v, M);
    else if (!std::strcmp(word, "relative") && !null)
      relative_rows(v, v + 16, M);
    else
      return 2;
    print_rows(M);
  }
  return 0;
}
