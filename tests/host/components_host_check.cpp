// Host check of dvo_slam_amd/csrc/dvo_components_core.h: the find, the lock-free union, the 16-bit minimum, the depth edge rule and
// the ranking key that the component kernels run on the device, run here on the host first -- a union that does not end would hang
// a GPU.  A stand-alone program (tests/test_mask_components.py builds it with -fsanitize=address,undefined and runs it):
//   - the unions of a plane applied in many shuffled orders and orientations, sequentially: every order must give the canonical
//     labels (a component's root is its smallest pixel index, found by a flood fill here) and no union may retry;
//   - the same unions dealt to several threads that apply them at once through __atomic builtins, on 32-bit parents and on 16-bit
//     parents packed two to a word (the device's LDS form): the canonical labels again, and every union's retries within the bound
//     the termination argument gives, a + b;
//   - the edge rule is symmetric and the ranking key orders by (area descending, root ascending).
// Prints one line and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "dvo_components_core.h"

using namespace dvo_amd::components;

namespace {

struct Parents32 {
  int *p;
  int load(int i) const { return __atomic_load_n(p + i, __ATOMIC_RELAXED); }
  int fetch_min(int i, int v) {
    int cur = __atomic_load_n(p + i, __ATOMIC_RELAXED);
    while (cur > v && !__atomic_compare_exchange_n(p + i, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
    return cur;
  }
};

struct Parents16 {
  unsigned *words;
  int load(int i) const { return (int)((__atomic_load_n(words + (i >> 1), __ATOMIC_RELAXED) >> ((i & 1) * 16)) & 0xffffu); }
  unsigned load_word(int k) const { return __atomic_load_n(words + k, __ATOMIC_RELAXED); }
  unsigned cas_word(int k, unsigned expected, unsigned desired) {
    __atomic_compare_exchange_n(words + k, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected;  // (what the word held: `expected` itself when the exchange took place)
  }
  int fetch_min(int i, int v) { return cc_fetch_min_u16(*this, i, v); }
};

struct Plane {
  int w, h;
  std::vector<unsigned char> fg;
  std::vector<float> z;  // empty: no depth
  const char *name;
};

int g_failures = 0;
void fail(const char *what, const Plane &P, int detail) {
  std::fprintf(stderr, "components_host_check: %s (plane %s %dx%d, %d)\n", what, P.name, P.w, P.h, detail);
  ++g_failures;
}

Plane random_plane(int w, int h, double density, unsigned seed, const char *name) {
  Plane P{w, h, std::vector<unsigned char>((size_t)w * h), {}, name};
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (auto &b : P.fg) b = u(rng) < density;
  return P;
}

// a one-pixel-wide path that runs along every other row and joins them alternately at the right and the left end
Plane serpentine(int w, int h) {
  Plane P{w, h, std::vector<unsigned char>((size_t)w * h, 0), {}, "serpentine"};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      if (y % 2 == 0) P.fg[(size_t)y * w + x] = 1;
      else P.fg[(size_t)y * w + x] = (x == ((y / 2) % 2 == 0 ? w - 1 : 0));
  return P;
}

// teeth that join only in the last row: the smallest index of the component is far from where its parts meet
Plane comb(int w, int h) {
  Plane P{w, h, std::vector<unsigned char>((size_t)w * h, 0), {}, "comb"};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) P.fg[(size_t)y * w + x] = (x % 2 == 0) || y == h - 1;
  return P;
}

Plane checkerboard(int w, int h) {
  Plane P{w, h, std::vector<unsigned char>((size_t)w * h, 0), {}, "checkerboard"};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) P.fg[(size_t)y * w + x] = (x + y) % 2 == 0;
  return P;
}

// a depth staircase over a full plane: steps of every size around the tolerance
Plane staircase(int w, int h, unsigned seed) {
  Plane P = random_plane(w, h, 0.9, seed, "staircase");
  P.z.resize((size_t)w * h);
  std::mt19937 rng(seed + 1);
  std::uniform_real_distribution<float> u(0.0f, 0.04f);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) P.z[(size_t)y * w + x] = 1.0f + 0.01f * (float)(x / 3) + u(rng);
  return P;
}

std::vector<std::pair<int, int>> edges_of(const Plane &P, int connectivity) {
  static const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, 0, -1, 1};
  std::vector<std::pair<int, int>> e;
  for (int y = 0; y < P.h; ++y)
    for (int x = 0; x < P.w; ++x) {
      const int i = y * P.w + x;
      if (!P.fg[i]) continue;
      for (int k = 0; k < (connectivity == 8 ? 4 : 2); ++k) {
        const int yy = y + dy[k], xx = x + dx[k];
        if (yy < 0 || xx < 0 || xx >= P.w) continue;
        const int j = yy * P.w + xx;
        if (!P.fg[j]) continue;
        if (!P.z.empty() && !cc_depth_edge(P.z[i], P.z[j], 0.0f, 10.0f)) continue;
        e.emplace_back(i, j);
      }
    }
  return e;
}

// the canonical roots by a flood fill in index order: the first pixel that reaches a component is its smallest index
std::vector<int> flood(const Plane &P, const std::vector<std::pair<int, int>> &e) {
  const int n = P.w * P.h;
  std::vector<std::vector<int>> adj(n);
  for (auto &p : e) adj[p.first].push_back(p.second), adj[p.second].push_back(p.first);
  std::vector<int> root(n, -1), stack;
  for (int i = 0; i < n; ++i) {
    if (!P.fg[i] || root[i] >= 0) continue;
    root[i] = i, stack.push_back(i);
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      for (int u : adj[v])
        if (root[u] < 0) root[u] = i, stack.push_back(u);
    }
  }
  return root;
}

template <class P>
bool labels_are(const P &parents, const Plane &pl, const std::vector<int> &want) {
  for (int i = 0; i < pl.w * pl.h; ++i)
    if (pl.fg[i] && cc_find(parents, i) != want[i]) return false;
  return true;
}

template <class P>
void run_threads(P parents, const std::vector<std::pair<int, int>> &order, int n_threads, long long *max_retries, bool *bound_held) {
  std::vector<std::thread> pool;
  std::vector<long long> worst(n_threads, 0);
  std::vector<char> ok(n_threads, 1);
  for (int t = 0; t < n_threads; ++t)
    pool.emplace_back([&, t]() {
      P mine = parents;
      for (size_t k = t; k < order.size(); k += n_threads) {
        const int a = order[k].first, b = order[k].second;
        const int retries = cc_union(mine, a, b);
        if (retries > worst[t]) worst[t] = retries;
        if (retries > a + b) ok[t] = 0;
      }
    });
  for (auto &th : pool) th.join();
  for (int t = 0; t < n_threads; ++t) {
    *max_retries = std::max(*max_retries, worst[t]);
    if (!ok[t]) *bound_held = false;
  }
}

void check_plane(const Plane &P, int connectivity, int orders, std::mt19937 &rng, long long *unions, long long *max_retries) {
  const int n = P.w * P.h;
  const auto e = edges_of(P, connectivity);
  const auto want = flood(P, e);
  auto order = e;
  std::vector<int> p32(n);
  std::vector<unsigned> p16((n + 1) / 2);
  for (int round = 0; round < orders; ++round) {
    std::shuffle(order.begin(), order.end(), rng);
    for (auto &pr : order)
      if (rng() & 1u) std::swap(pr.first, pr.second);
    // sequentially: no retry at all, and the canonical labels
    for (int i = 0; i < n; ++i) p32[i] = i;
    Parents32 seq{p32.data()};
    int retried = 0;
    for (auto &pr : order) retried += cc_union(seq, pr.first, pr.second);
    *unions += (long long)order.size();
    if (retried) fail("a sequential union retried", P, retried);
    if (!labels_are(seq, P, want)) fail("a sequential order gave other labels", P, round);
    for (int i = 0; i < n; ++i)
      if (p32[i] > i) fail("a parent exceeds its index", P, i);
    // from four threads at once, 32-bit parents
    if (round % 4 == 0) {
      bool held = true;
      for (int i = 0; i < n; ++i) p32[i] = i;
      run_threads(Parents32{p32.data()}, order, 4, max_retries, &held);
      *unions += (long long)order.size();
      if (!held) fail("a concurrent union retried more than a + b times", P, round);
      if (!labels_are(Parents32{p32.data()}, P, want)) fail("a concurrent order gave other labels", P, round);
    }
    // ... and 16-bit parents packed two to a word, where the plane fits a tile
    if (round % 4 == 1 && n <= 65536) {
      bool held = true;
      for (int i = 0; i < n; ++i) {
        unsigned &wd = p16[i >> 1];
        wd = (i & 1) ? ((wd & 0xffffu) | ((unsigned)i << 16)) : (unsigned)i;
      }
      run_threads(Parents16{p16.data()}, order, 4, max_retries, &held);
      *unions += (long long)order.size();
      if (!held) fail("a concurrent 16-bit union retried more than a + b times", P, round);
      if (!labels_are(Parents16{p16.data()}, P, want)) fail("a concurrent 16-bit order gave other labels", P, round);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(20240521u);
  long long unions = 0, max_retries = 0;
  std::vector<Plane> planes;
  planes.push_back(random_plane(23, 17, 0.3, 1, "random 0.3"));
  planes.push_back(random_plane(23, 17, 0.6, 2, "random 0.6"));
  planes.push_back(random_plane(64, 64, 0.6, 3, "random tile"));
  planes.push_back(random_plane(40, 9, 0.9, 4, "random 0.9"));
  planes.push_back(serpentine(31, 21));
  planes.push_back(serpentine(64, 64));
  planes.push_back(comb(33, 12));
  planes.push_back(checkerboard(20, 15));
  planes.push_back(staircase(37, 11, 5));
  for (const Plane &P : planes)
    for (int connectivity : {4, 8}) check_plane(P, connectivity, P.w * P.h > 2000 ? 8 : 40, rng, &unions, &max_retries);

  // the edge rule is symmetric, and true for equal depths
  std::uniform_real_distribution<float> z(0.3f, 8.0f), step(-0.2f, 0.2f), s(0.0f, 20.0f);
  for (int k = 0; k < 200000; ++k) {
    const float a = z(rng), b = a + step(rng), ms = k % 3 ? 0.0f : 0.01f, sg = s(rng);
    if (cc_depth_edge(a, b, ms, sg) != cc_depth_edge(b, a, ms, sg) || !cc_depth_edge(a, a, ms, sg)) {
      std::fprintf(stderr, "components_host_check: the edge rule is not symmetric at %a %a\n", a, b);
      ++g_failures;
      break;
    }
  }
  // the ranking key: larger key = larger area, then smaller root; the root comes back out of the key
  std::uniform_int_distribution<int> area(1, 1 << 30), root(0, (1 << 30) - 1);
  for (int k = 0; k < 200000; ++k) {
    const int a0 = k % 5 ? area(rng) : 7, a1 = k % 7 ? area(rng) : 7, r0 = root(rng), r1 = root(rng);
    if (r0 == r1) continue;
    const bool first = a0 != a1 ? a0 > a1 : r0 < r1;
    const unsigned long long k0 = cc_rank_key(a0, r0), k1 = cc_rank_key(a1, r1);
    if ((k0 > k1) != first || k0 == 0 || cc_rank_key_root(k0) != r0 || cc_rank_key_root(k1) != r1) {
      std::fprintf(stderr, "components_host_check: the ranking key misorders (%d, %d) and (%d, %d)\n", a0, r0, a1, r1);
      ++g_failures;
      break;
    }
  }
  if (g_failures) return 1;
  std::printf("components_host_check: ok, %lld unions over %zu planes, at most %lld retries in one union\n", unions, planes.size(),
              max_retries);
  return 0;
}
