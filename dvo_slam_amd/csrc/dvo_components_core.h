// The pieces of the connected-component kernels (dvo_components.cpp) that decide whether a labelling is right and whether it ends:
// find, the lock-free union, the 16-bit minimum inside a 32-bit word that a tile's LDS parents need, the depth edge rule and the
// ranking key of keep_largest.  Plain C++ behind one macro, so that tests/host/components_host_check.cpp runs exactly these functions
// on the host -- sequentially and from several threads, in many orders -- before any of it runs on a device.
//
// A parent array p over indices 0 .. n-1 is seen through an accessor P:
//     int  P::load(int i) const           the parent of i (an atomic or volatile read: other workers may be writing)
//     int  P::fetch_min(int i, int v)     p[i] = min(p[i], v) atomically, returns what p[i] held before
// INVARIANT: p[i] <= i at all times, and p[i] == i makes i a root.  Every write lowers an entry (fetch_min), so the entries never
// rise.  A chain i -> p[i] -> p[p[i]] ... therefore falls strictly until it meets a root, and the root of a set is its smallest
// index: the canonical name the rules in include/dvo_amd.h ask for, whatever order the unions were applied in.
#pragma once

#if defined(__HIPCC__)
#define DVO_CC_HD __host__ __device__ __forceinline__
#else
#define DVO_CC_HD inline
#endif

namespace dvo_amd {
namespace components {

// The root of i.  Ends: every step goes to a strictly smaller index (the invariant), and indices are >= 0.  Writes nothing.
template <class P>
DVO_CC_HD int cc_find(const P &p, int i) {
  for (;;) {
    const int q = p.load(i);
    if (q == i) return i;
    i = q;
  }
}

// Unites the sets of a and b, any number of workers at once.  Returns the number of retries.
//
// Each round finds the two roots, orders them a > b and lowers p[a] to b with one fetch_min.  If that found p[a] == a, a was still
// a root and now hangs under the smaller root b: done.  Otherwise another worker was faster and p[a] held some old < a: the entry
// is now min(old, b), which may have cut the link a -> old, so the round goes on uniting (old, b) -- that restores whatever the
// minimum replaced and is what the caller asked for as well, a and old being in one set.
// WHY IT ENDS: a retry replaces a by old, and old < a strictly; b is only ever replaced by its root, which is <= b.  So a + b
// falls by at least one per retry and is >= 0: at most a + b retries on any input and under any interleaving, and none at all when
// nobody else writes (then the roots found are still roots when fetch_min lands).
template <class P>
DVO_CC_HD int cc_union(P &p, int a, int b) {
  int retries = 0;
  for (;;) {
    a = cc_find(p, a);
    b = cc_find(p, b);
    if (a == b) return retries;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = p.fetch_min(a, b);
    if (old == a) return retries;
    a = old;
    ++retries;
  }
}

// p[i] = min(p[i], v) for 16-bit entries packed two to a 32-bit word (entry i: bits 16 (i & 1) .. of word i >> 1), on top of a
// word accessor W:  unsigned W::load_word(int k) const;  unsigned W::cas_word(int k, unsigned expected, unsigned desired) (returns
// what the word held).  Returns the entry's old value.  Ends: the compare-and-swap fails only when the word changed, a word
// changes only by one of its two entries falling, and an entry falls at most 65535 times.
template <class W>
DVO_CC_HD int cc_fetch_min_u16(W &w, int i, int v) {
  const int k = i >> 1, shift = (i & 1) * 16;
  unsigned seen = w.load_word(k);
  for (;;) {
    const int cur = (int)((seen >> shift) & 0xffffu);
    if (cur <= v) return cur;
    const unsigned want = (seen & ~(0xffffu << shift)) | ((unsigned)v << shift);
    const unsigned got = w.cas_word(k, seen, want);
    if (got == seen) return cur;
    seen = got;
  }
}

// the depth edge rule of "Mask components": fp32, every operation rounded on its own (the translation units that include this are
// built with -ffp-contract=off)
DVO_CC_HD bool cc_depth_edge(float za, float zb, float max_step, float depth_sigmas) {
  const float zn = za < zb ? za : zb;  // fminf of two finite numbers
  const float t = zn - 0.4f;
  const float tt = t * t;
  const float s = 0.0019f * tt;  // (the sensor sigma step by step, not rules::depth_sigma: this header is compiled for the host alone too)
  const float m = 0.0012f + s;
  const float tol = max_step + depth_sigmas * m;
  const float d = za - zb;
  return (d < 0.0f ? -d : d) <= tol;
}

// keep_largest ranks by (area descending, root ascending): the larger key wins.  Never 0 for a component (area >= 1).
DVO_CC_HD unsigned long long cc_rank_key(int area, int root) {
  return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(~(unsigned)root);
}
DVO_CC_HD int cc_rank_key_root(unsigned long long key) { return (int)~(unsigned)(key & 0xffffffffull); }

}  // namespace components
}  // namespace dvo_amd
