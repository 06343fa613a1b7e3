// Connected components of masks and of depth, on the device: dvo_amd_mask_filter_components / _many keep the components of a
// foreground that pass an area band, touch a seed mask or are among the k largest; dvo_amd_mask_components hands out one level's
// label plane and per-component records.  The fourth producer of masks from masks next to dvo_mask_ops.cpp: every result is an
// ordinary dvo_amd_mask (mask_alloc / mask_finish), the inputs are only read.  The rules are pinned in include/dvo_amd.h ("Mask
// components"); tests/mask_components_ref.py restates them with numpy and scipy.sparse.csgraph.
//
// A call of any number of items and levels is FIVE launches, each over all (item, level) planes at once, and one synchronisation:
//   k_cc_local    a block owns a 64 x 64 tile of a plane.  Per pixel: foreground, and which of its four BACKWARD neighbours (W, N,
//                 NW, NE) it has an edge to under the connectivity and the depth rule -- five bits in a byte plane that the later
//                 passes read instead of the inputs; the refused pairs are counted here (every pair has one backward end).  Then a
//                 union-find over the tile in LDS, 16-bit tile indices packed two to a word: the row edges, a flatten, the edges
//                 to the row above, and every pixel's tile root goes out as a GLOBAL pixel index into the int32 parent plane.
//   k_cc_border   the edges that cross a tile seam, united on the global parent plane with atomicMin (cc_union).
//   k_cc_flatten  every pixel to its root.  A wave peels off its lanes root by root, reduces their count, box and seed bit with
//                 cross-lane moves and sends one set of integer atomics per (wave, root) to the root's record; roots append
//                 themselves to the plane's work list.
//   k_cc_select   one block per plane walks the work list: the area band and the seed test, the largest area, and for keep_largest
//                 up to 8 rounds of a 64-bit atomicMax over (area << 32) | ~root, each round below the previous winner.
//   k_cc_write    the byte planes and kept[l].
// The parent arrays obey dvo_components_core.h's invariant (an entry never exceeds its index, entries only fall), so the root of a
// component is its smallest pixel index whatever order the unions landed in; all atomics are integer: every output is a function
// of the inputs alone and two runs are bit-identical.  Nothing here waits for another thread: the only loops that depend on other
// threads' writes are cc_union's retry and the 16-bit compare-and-swap, and both are bounded (see the core header).
#include "dvo_internal.h"
#include "dvo_device_rules.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <string>

#include "dvo_components_core.h"

namespace dvo_amd {
namespace components {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 64;                       // a tile is kTile x kTile pixels: 4096 indices, 8 KB of 16-bit parents
constexpr int kTileRows = kTile / kWaves;       // consecutive rows of a tile column that one thread owns
constexpr int kLanePixels = 4;                  // border, write: pixels per lane
constexpr int kChunk = kBlock * kLanePixels;
constexpr int kSelectBlock = 1024;
constexpr int kRecInts = 8;                     // area, x0, y0, x1, y1, seeded, kept, passed
constexpr int kPlaneCounts = 8;                 // foreground, components, kept_components, kept_pixels, largest_area, edges_cut, work list
static_assert(kTile * kTile <= 65536, "a tile index fits 16 bits");
static_assert(DVO_AMD_COMPONENTS_COUNTS <= kPlaneCounts - 1, "a plane's counts and its work-list cursor");

enum { kFg = 1, kW = 2, kN = 4, kNW = 8, kNE = 16 };

// one (item, level) as the kernels read it
struct Plane {
  const unsigned char *mask;   // null: every pixel counts
  const float *z;              // null: no depth
  const unsigned char *seeds;  // null: no seeds
  unsigned char *out;          // the result's plane (null: dvo_amd_mask_components)
  int *kept;                   // the result's counter of the level
  int *parent;                 // [n] -1 = background, else a pixel of the same component with a smaller or equal index
  int *rec;                    // [n][kRecInts], valid at tile roots (initialised by k_cc_local), meaningful at roots
  int *roots;                  // [n] the work list of k_cc_select: the roots, in whatever order they arrived
  unsigned char *ebits;        // [n] kFg | kW | kN | kNW | kNE
  unsigned long long *counts;  // [kPlaneCounts]
  int w, h, tiles_x, tiles;
  int min_area, max_area;
};

struct LdsParents {
  unsigned *words;
  __device__ int load(int i) const { return (int)((const volatile unsigned short *)words)[i]; }
  __device__ unsigned load_word(int k) const { return ((const volatile unsigned *)words)[k]; }
  __device__ unsigned cas_word(int k, unsigned expected, unsigned desired) { return atomicCAS(words + k, expected, desired); }
  __device__ int fetch_min(int i, int v) { return cc_fetch_min_u16(*this, i, v); }
};

struct GlobalParents {
  int *p;
  __device__ int load(int i) const { return __atomic_load_n(p + i, __ATOMIC_RELAXED); }
  __device__ int fetch_min(int i, int v) { return atomicMin(p + i, v); }
};

// a pixel as the edge rule sees it: NaN for background and for anything outside the plane, else its depth (0 without a depth plane:
// cc_depth_edge(0, 0) holds for every max_step >= 0 and depth_sigmas >= 0)
__device__ __forceinline__ float cc_pixel(const Plane &R, int x, int y) {
  if (x < 0 || y < 0 || x >= R.w || y >= R.h) return __builtin_nanf("");
  const size_t at = (size_t)y * (size_t)R.w + (size_t)x;
  if (R.mask && R.mask[at] == 0) return __builtin_nanf("");
  if (!R.z) return 0.0f;
  const float z = R.z[at];
  return rules::finite_f(z) ? z : __builtin_nanf("");
}

__global__ void __launch_bounds__(kBlock) k_cc_local(const Plane *__restrict__ planes, int n_planes, int connectivity, float max_step,
                                                     float depth_sigmas) {
  __shared__ unsigned s_words[kTile * kTile / 2];
  LdsParents lds = {s_words};
  unsigned short *lab = (unsigned short *)s_words;
  const int col = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * kTileRows;
  for (int rec = blockIdx.y; rec < n_planes; rec += gridDim.y) {
    const Plane R = planes[rec];                 // uniform over the block
    if ((int)blockIdx.x >= R.tiles) continue;    // (block-uniform: no barrier is skipped by part of a block)
    const int tx0 = ((int)blockIdx.x % R.tiles_x) * kTile, ty0 = ((int)blockIdx.x / R.tiles_x) * kTile;
    const int x = tx0 + col;
    unsigned char e[kTileRows];
    int n_fg = 0, n_cut = 0;
    // the row above the thread's first: its W, own and E pixels (NaN outside the plane)
    float pw = cc_pixel(R, x - 1, ty0 + r0 - 1), pc = cc_pixel(R, x, ty0 + r0 - 1), pe = cc_pixel(R, x + 1, ty0 + r0 - 1);
#pragma unroll
    for (int k = 0; k < kTileRows; ++k) {
      const int y = ty0 + r0 + k;
      const float zw = cc_pixel(R, x - 1, y), zc = cc_pixel(R, x, y), ze = cc_pixel(R, x + 1, y);
      unsigned bits = 0u;
      if (zc == zc) {
        bits = kFg, ++n_fg;
        if (zw == zw) {
          if (cc_depth_edge(zc, zw, max_step, depth_sigmas)) bits |= kW;
          else ++n_cut;
        }
        if (pc == pc) {
          if (cc_depth_edge(zc, pc, max_step, depth_sigmas)) bits |= kN;
          else ++n_cut;
        }
        if (connectivity == 8) {
          if (pw == pw) {
            if (cc_depth_edge(zc, pw, max_step, depth_sigmas)) bits |= kNW;
            else ++n_cut;
          }
          if (pe == pe) {
            if (cc_depth_edge(zc, pe, max_step, depth_sigmas)) bits |= kNE;
            else ++n_cut;
          }
        }
      }
      e[k] = (unsigned char)bits;
      lab[(r0 + k) * kTile + col] = (unsigned short)((r0 + k) * kTile + col);
      pw = zw, pc = zc, pe = ze;
    }
    n_fg = rules::wave_sum(n_fg), n_cut = rules::wave_sum(n_cut);
    if ((threadIdx.x & 63) == 0) {
      if (n_fg) atomicAdd(R.counts + 0, (unsigned long long)n_fg);
      if (n_cut) atomicAdd(R.counts + 5, (unsigned long long)n_cut);
    }
    __syncthreads();
    // the row edges inside the tile ...
#pragma unroll
    for (int k = 0; k < kTileRows; ++k)
      if ((e[k] & kW) && col > 0) cc_union(lds, (r0 + k) * kTile + col, (r0 + k) * kTile + col - 1);
    __syncthreads();
    // ... flattened, so that the unions across rows start from runs, not from chains (a 16-bit store next to 16-bit loads of the
    // same entries: whichever a reader sees is an ancestor)
#pragma unroll
    for (int k = 0; k < kTileRows; ++k) {
      const int i = (r0 + k) * kTile + col;
      if (e[k] & kFg) lab[i] = (unsigned short)cc_find(lds, i);
    }
    __syncthreads();
    // ... the edges to the row above inside the tile
#pragma unroll
    for (int k = 0; k < kTileRows; ++k) {
      const int row = r0 + k, i = row * kTile + col;
      if (row == 0) continue;
      if (e[k] & kN) cc_union(lds, i, i - kTile);
      if ((e[k] & kNW) && col > 0) cc_union(lds, i, i - kTile - 1);
      if ((e[k] & kNE) && col < kTile - 1) cc_union(lds, i, i - kTile + 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTileRows; ++k) {
      const int row = r0 + k, i = row * kTile + col, y = ty0 + row;
      if (x >= R.w || y >= R.h) continue;
      const size_t g = (size_t)y * (size_t)R.w + (size_t)x;
      R.ebits[g] = e[k];
      if (!(e[k] & kFg)) {
        R.parent[g] = -1;
        continue;
      }
      const int t = cc_find(lds, i);
      R.parent[g] = (ty0 + (t >> 6)) * R.w + tx0 + (t & 63);  // (the tile root lies in the plane: it is a foreground pixel)
      if (t == i) {  // only a tile root can be a root of the plane: the records of the others are never touched
        int4 *r = (int4 *)(R.rec + g * kRecInts);
        r[0] = make_int4(0, INT_MAX, INT_MAX, -1), r[1] = make_int4(-1, 0, 0, 0);
      }
    }
    __syncthreads();  // the labels are written again for the block's next plane
  }
}

__global__ void __launch_bounds__(kBlock) k_cc_border(const Plane *__restrict__ planes, int n_planes) {
  for (int rec = blockIdx.y; rec < n_planes; rec += gridDim.y) {
    const Plane R = planes[rec];
    const int n = R.w * R.h;
    const int g0 = (blockIdx.x * kBlock + threadIdx.x) * kLanePixels;
    if (g0 >= n) continue;  // (n is a multiple of 4: four pixels of one row, or none)
    const unsigned word = *(const unsigned *)(R.ebits + g0);
    if (!(word & 0x1e1e1e1eu)) continue;
    GlobalParents P = {R.parent};
    const int y = g0 / R.w, x0 = g0 - y * R.w;
    const bool top = (y & (kTile - 1)) == 0;
#pragma unroll
    for (int k = 0; k < kLanePixels; ++k) {
      const unsigned bits = (word >> (8 * k)) & 0xffu;
      const int x = x0 + k, g = g0 + k;
      const bool left = (x & (kTile - 1)) == 0, right = (x & (kTile - 1)) == kTile - 1;
      // (a set bit says the neighbour is a foreground pixel of the plane: the indices below are inside it)
      if ((bits & kW) && left) cc_union(P, g, g - 1);
      if ((bits & kN) && top) cc_union(P, g, g - R.w);
      if ((bits & kNW) && (top || left)) cc_union(P, g, g - R.w - 1);
      if ((bits & kNE) && (top || right)) cc_union(P, g, g - R.w + 1);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_cc_flatten(const Plane *__restrict__ planes, int n_planes) {
  const int lane = threadIdx.x & 63;
  for (int rec = blockIdx.y; rec < n_planes; rec += gridDim.y) {
    const Plane R = planes[rec];
    const int n = R.w * R.h;
    if ((int)(blockIdx.x * kBlock) >= n) continue;  // (block-uniform; within a block every lane of a wave reaches the ballots)
    const int g = blockIdx.x * kBlock + threadIdx.x;
    GlobalParents P = {R.parent};
    int root = -1;
    if (g < n && P.load(g) >= 0) {
      root = cc_find(P, g);
      R.parent[g] = root;  // (no union runs in this launch: a reader sees the old ancestor or the root)
    }
    const bool fg = root >= 0;
    const int y = fg ? g / R.w : 0, x = fg ? g - y * R.w : 0;
    const int seeded = fg && R.seeds && R.seeds[g] != 0 ? 1 : 0;
    // roots join the work list: one cursor step per wave
    const unsigned long long is_root = __ballot(fg && root == g);
    if (is_root) {
      int base = 0;  // (a plane has at most 2^30 pixels: the cursor fits)
      if (lane == 0) base = (int)atomicAdd(R.counts + 6, (unsigned long long)__popcll(is_root));
      base = __shfl(base, 0);
      if (fg && root == g) R.roots[base + __popcll(is_root & ((1ull << lane) - 1ull))] = g;
    }
    // the wave's pixels root by root
    unsigned long long todo = __ballot(fg);
    while (todo) {  // (wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const int lr = __shfl(root, leader);
      const bool mine = fg && root == lr;
      const unsigned long long m = __ballot(mine);
      int vx0 = mine ? x : INT_MAX, vy0 = mine ? y : INT_MAX, vx1 = mine ? x : -1, vy1 = mine ? y : -1, vs = mine ? seeded : 0;
      if (__popcll(m) > 1) {
#pragma unroll
        for (int off = 32; off; off >>= 1) {
          vx0 = min(vx0, __shfl_xor(vx0, off)), vy0 = min(vy0, __shfl_xor(vy0, off));
          vx1 = max(vx1, __shfl_xor(vx1, off)), vy1 = max(vy1, __shfl_xor(vy1, off));
          vs |= __shfl_xor(vs, off);
        }
      }
      if (lane == leader) {
        int *r = R.rec + (size_t)lr * kRecInts;
        atomicAdd(r + 0, __popcll(m));
        atomicMin(r + 1, vx0), atomicMin(r + 2, vy0), atomicMax(r + 3, vx1), atomicMax(r + 4, vy1);
        if (vs) atomicOr(r + 5, 1);
      }
      todo &= ~m;
    }
  }
}

__global__ void __launch_bounds__(kSelectBlock) k_cc_select(const Plane *__restrict__ planes, int keep_largest) {
  __shared__ int s_largest, s_kept;
  __shared__ unsigned long long s_best;
  const Plane R = planes[blockIdx.x];
  const int n_roots = (int)R.counts[6];
  if (threadIdx.x == 0) s_largest = 0, s_kept = 0;
  __syncthreads();
  int largest = 0, kept = 0;
  for (int i = threadIdx.x; i < n_roots; i += kSelectBlock) {
    int *r = R.rec + (size_t)R.roots[i] * kRecInts;
    const int area = r[0];
    const bool pass = R.min_area <= area && (R.max_area < 0 || area <= R.max_area) && (!R.seeds || r[5] != 0);
    largest = max(largest, area);
    if (keep_largest == 0) {
      if (pass) r[6] = 1, ++kept;
    } else {
      r[7] = pass ? 1 : 0;
    }
  }
  if (largest) atomicMax(&s_largest, largest);
  if (kept) atomicAdd(&s_kept, kept);
  __syncthreads();
  unsigned long long below = ~0ull;
  for (int round = 0; round < keep_largest; ++round) {  // (block-uniform: keep_largest <= 8)
    if (threadIdx.x == 0) s_best = 0ull;
    __syncthreads();
    unsigned long long best = 0ull;
    for (int i = threadIdx.x; i < n_roots; i += kSelectBlock) {
      const int root = R.roots[i];
      const int *r = R.rec + (size_t)root * kRecInts;
      if (!r[7]) continue;
      const unsigned long long key = cc_rank_key(r[0], root);
      if (key < below && key > best) best = key;
    }
    if (best) atomicMax(&s_best, best);
    __syncthreads();
    const unsigned long long winner = s_best;
    __syncthreads();  // (everyone has read the winner before thread 0 clears it for the next round)
    if (winner == 0ull) break;  // (block-uniform) fewer components passed than keep_largest
    if (threadIdx.x == 0) R.rec[(size_t)cc_rank_key_root(winner) * kRecInts + 6] = 1, ++s_kept;
    below = winner;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    R.counts[1] = (unsigned long long)n_roots;
    R.counts[2] = (unsigned long long)s_kept;
    R.counts[4] = (unsigned long long)s_largest;
  }
}

__global__ void __launch_bounds__(kBlock) k_cc_write(const Plane *__restrict__ planes, int n_planes) {
  for (int rec = blockIdx.y; rec < n_planes; rec += gridDim.y) {
    const Plane R = planes[rec];
    const int n = R.w * R.h;
    if ((int)(blockIdx.x * kChunk) >= n) continue;  // (block-uniform)
    const int g0 = (blockIdx.x * kBlock + threadIdx.x) * kLanePixels;
    unsigned word = 0u;
    if (g0 < n) {
      const int4 p = *(const int4 *)(R.parent + g0);
      const int roots[kLanePixels] = {p.x, p.y, p.z, p.w};
#pragma unroll
      for (int k = 0; k < kLanePixels; ++k)
        if (roots[k] >= 0 && R.rec[(size_t)roots[k] * kRecInts + 6] != 0) word |= 1u << (8 * k);
      *(unsigned *)(R.out + g0) = word;
    }
    int c = 0;
#pragma unroll
    for (int k = 0; k < kLanePixels; ++k) c += __popcll(__ballot((word >> (8 * k)) & 1u));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(R.kept, c);
  }
}

}  // namespace components
}  // namespace dvo_amd

using namespace dvo_amd;
using namespace dvo_amd::host;
using namespace dvo_amd::components;

namespace {

// dvo_amd_debug_components_timing: two events around the launches of a call on the prep stream (off unless asked for).  One pair
// of events per device, recorded without the device's mutex: a diagnostic for one thread at a time.  Two threads that call on one
// device with timing on may interleave their records, and last_ms then spans parts of both calls.
DeviceTiming g_timing[kMaxDevices];

// the plane table, the counts and the working planes of the call in flight: grown to the largest call and kept, used with the
// device's mutex held from the table's upload to the last thing enqueued that touches it (as dvo_mask_ops.cpp's warp area)
DeviceBuf g_area[kMaxDevices];

void drop(dvo_amd_mask *m) {
  (void)hipFree(m->mem);
  delete m;
}

// one item of a call: what it is labelled from and the geometry that follows
struct Item {
  const dvo_amd_mask *mask;
  const dvo_amd_pyramid *depth;
  const dvo_amd_mask *seeds;
  int w, h, levels, device;
};

int check_options(const char *entry, const dvo_amd_component_options *opt) {
  if (!opt) return invalid(entry, "the options are NULL");
  if (opt->connectivity != 4 && opt->connectivity != 8) return invalid(entry, "connectivity must be 4 or 8");
  if (!std::isfinite(opt->max_step) || opt->max_step < 0.0f) return invalid(entry, "max_step must be finite and >= 0");
  if (!std::isfinite(opt->depth_sigmas) || opt->depth_sigmas < 0.0f) return invalid(entry, "depth_sigmas must be finite and >= 0");
  if (opt->keep_largest < 0 || opt->keep_largest > DVO_AMD_COMPONENTS_MAX_LARGEST)
    return invalid(entry, "keep_largest is outside 0.." + std::to_string(DVO_AMD_COMPONENTS_MAX_LARGEST));
  return DVO_AMD_OK;
}

// the argument checks of one item (no device needed); `who` prefixes the reason ("item 3: ")
int check_item(const char *entry, const std::string &who, const dvo_amd_mask *mask, const dvo_amd_pyramid *depth, const dvo_amd_mask *seeds,
               Item *it) {
  if (!mask && !depth) return invalid(entry, who + "mask and depth are both NULL");
  it->mask = mask, it->depth = depth, it->seeds = seeds;
  if (mask) {
    it->w = mask->w, it->h = mask->h, it->levels = mask->levels, it->device = mask->device;
    if (depth) {
      if (depth->lv[0].w != it->w || depth->lv[0].h != it->h)
        return invalid(entry, who + "the mask is " + std::to_string(it->w) + "x" + std::to_string(it->h) + " but depth is " +
                                  std::to_string(depth->lv[0].w) + "x" + std::to_string(depth->lv[0].h));
      if (depth->n_levels < it->levels)
        return invalid(entry, who + "the mask has " + std::to_string(it->levels) + " levels but depth has " + std::to_string(depth->n_levels));
    }
  } else {
    it->w = depth->lv[0].w, it->h = depth->lv[0].h, it->levels = depth->n_levels, it->device = depth->device;
    const int rc = check_mask_size(entry, it->w, it->h, it->levels);
    if (rc) return rc;
  }
  if (seeds) {
    if (seeds->w != it->w || seeds->h != it->h)
      return invalid(entry, who + "the foreground is " + std::to_string(it->w) + "x" + std::to_string(it->h) + " but seeds is " +
                                std::to_string(seeds->w) + "x" + std::to_string(seeds->h));
    if (seeds->levels < it->levels)
      return invalid(entry, who + "the foreground has " + std::to_string(it->levels) + " levels but seeds has " + std::to_string(seeds->levels));
  }
  return DVO_AMD_OK;
}

bool one_device(const Item &it, int device) {
  return (!it.mask || it.mask->device == device) && (!it.depth || it.depth->device == device) && (!it.seeds || it.seeds->device == device);
}

// where the working planes of `n_planes` planes lie in the area; `pixels` is the sum of the planes' pixel counts, each rounded up
// to 256, so that every plane of every kind starts 256-byte aligned when the planes are laid out back to back
struct Layout {
  size_t table, counts, parent, rec, roots, ebits, total;
};
Layout layout(size_t n_planes, size_t pixels) {
  Layout L;
  L.table = 0;
  L.counts = align_up(sizeof(Plane) * n_planes, 256);
  L.parent = L.counts + align_up(sizeof(unsigned long long) * kPlaneCounts * n_planes, 256);
  L.rec = L.parent + sizeof(int) * pixels;
  L.roots = L.rec + sizeof(int) * kRecInts * pixels;
  L.ebits = L.roots + sizeof(int) * pixels;
  L.total = L.ebits + pixels;
  return L;
}

int grow_area(DeviceBuf &area, size_t bytes) { return grow(area, bytes, 1 << 20, "components area"); }

// the table of a call's planes in the area at `base`; out[k] may be null (dvo_amd_mask_components)
void fill_table(std::vector<Plane> &table, const std::vector<Item> &items, const std::vector<int> &first_level, const std::vector<int> &n_levels,
                const std::vector<dvo_amd_mask *> &made, const dvo_amd_component_options *opt, char *base, const Layout &L, int *max_n,
                int *max_tiles) {
  size_t r = 0, px = 0;  // px: pixels of the planes before, each count rounded up to 256 (layout)
  *max_n = 1, *max_tiles = 1;
  for (size_t k = 0; k < items.size(); ++k) {
    const Item &it = items[k];
    for (int l = first_level[k]; l < first_level[k] + n_levels[k]; ++l, ++r) {
      Plane &R = table[r];
      R.w = it.w >> l, R.h = it.h >> l;
      const size_t n = (size_t)R.w * (size_t)R.h;
      R.mask = it.mask ? it.mask->plane[l] : nullptr;
      R.z = it.depth ? it.depth->lv[l].z_plane : nullptr;
      R.seeds = it.seeds ? it.seeds->plane[l] : nullptr;
      R.out = made[k] ? made[k]->plane[l] : nullptr;
      R.kept = made[k] ? made[k]->counters + l : nullptr;
      R.parent = (int *)(base + L.parent) + px;
      R.rec = (int *)(base + L.rec) + px * kRecInts;
      R.roots = (int *)(base + L.roots) + px;
      R.ebits = (unsigned char *)(base + L.ebits) + px;
      R.counts = (unsigned long long *)(base + L.counts) + kPlaneCounts * r;
      R.tiles_x = (R.w + kTile - 1) / kTile;
      R.tiles = R.tiles_x * ((R.h + kTile - 1) / kTile);
      R.min_area = opt->min_area[l], R.max_area = opt->max_area[l];
      *max_n = std::max(*max_n, (int)n), *max_tiles = std::max(*max_tiles, R.tiles);
      px += align_up(n, 256);
    }
  }
}

// k_cc_local, k_cc_border, k_cc_flatten: the labelling, shared by the filter and the inspection entry
hipError_t launch_labelling(const Plane *d_table, size_t n_planes, int max_n, int max_tiles, const dvo_amd_component_options *opt,
                            hipStream_t st) {
  const unsigned gt = (unsigned)max_tiles, g4 = (unsigned)((max_n + kChunk - 1) / kChunk), g1 = (unsigned)((max_n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_cc_local, dim3(gt, grid_rows((long long)n_planes, gt, kBlock)), dim3(kBlock), 0, st, d_table, (int)n_planes,
                     opt->connectivity, opt->max_step, opt->depth_sigmas);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cc_border, dim3(g4, grid_rows((long long)n_planes, g4, kBlock)), dim3(kBlock), 0, st, d_table, (int)n_planes);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cc_flatten, dim3(g1, grid_rows((long long)n_planes, g1, kBlock)), dim3(kBlock), 0, st, d_table, (int)n_planes);
  return hipGetLastError();
}

int filter_many(const char *entry, bool single, int n, const dvo_amd_mask *const *masks, const dvo_amd_pyramid *const *depths,
                const dvo_amd_mask *const *seeds, const dvo_amd_component_options *opt, dvo_amd_mask **out, long long *counts) {
  if (out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative count");
  if (!out) return invalid(entry, "out is NULL");
  if (!masks && !depths) return invalid(entry, "masks and depths are both NULL");
  int rc = check_options(entry, opt);
  if (rc) return rc;
  std::vector<Item> items((size_t)std::max(n, 0));
  size_t n_planes = 0, pixels = 0;
  for (int k = 0; k < n; ++k) {
    const std::string who = single ? std::string() : "item " + std::to_string(k) + ": ";
    Item &it = items[(size_t)k];
    rc = check_item(entry, who, masks ? masks[k] : nullptr, depths ? depths[k] : nullptr, seeds ? seeds[k] : nullptr, &it);
    if (rc) return rc;
    for (int l = 0; l < it.levels; ++l) {
      if (opt->min_area[l] < 0) return invalid(entry, who + "min_area[" + std::to_string(l) + "] is negative");
      pixels += align_up((size_t)(it.w >> l) * (size_t)(it.h >> l), 256);
    }
    n_planes += (size_t)it.levels;
  }
  for (int k = 0; k < n; ++k)
    if (!one_device(items[(size_t)k], items[0].device)) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;
  if (n_planes > (size_t)(1 << 24)) return invalid(entry, "more than 2^24 (item, level) planes");
  if (pixels > (size_t)1 << 34) return invalid(entry, "more than 2^34 pixels in one call");

  const int device = items[0].device;
  std::vector<dvo_amd_mask *> made((size_t)n, nullptr);
  hipStream_t st = nullptr;
  auto unwind = [&](int status) {
    if (st) (void)hipStreamSynchronize(st);
    for (dvo_amd_mask *m : made)
      if (m) drop(m);
    return status;
  };
  Bracket bracket(g_timing[device]);
  for (int k = 0; k < n; ++k) {
    rc = mask_alloc(entry, device, items[(size_t)k].w, items[(size_t)k].h, items[(size_t)k].levels, &made[(size_t)k], &st);
    if (rc) return unwind(rc);
  }
  const Layout L = layout(n_planes, pixels);
  std::unique_lock<std::mutex> area_lock(device_mutex(device));
  DeviceBuf &area = g_area[device];
  rc = grow_area(area, L.total);
  if (rc) {
    area_lock.unlock();
    return unwind(rc);
  }
  char *base = (char *)area.p;
  std::vector<Plane> table(n_planes);
  std::vector<int> first((size_t)n, 0), levels((size_t)n);
  for (int k = 0; k < n; ++k) levels[(size_t)k] = items[(size_t)k].levels;
  int max_n = 1, max_tiles = 1;
  fill_table(table, items, first, levels, made, opt, base, L, &max_n, &max_tiles);
  const Plane *d_table = (const Plane *)(base + L.table);
  const size_t count_bytes = sizeof(unsigned long long) * kPlaneCounts * n_planes;
  std::vector<unsigned long long> h_counts(counts ? kPlaneCounts * n_planes : 0);
  std::vector<int> h_kept((size_t)n * DVO_AMD_MAX_LEVELS, 0);
  hipError_t e = bracket.begin(st);
  if (e == hipSuccess) e = hipMemcpyAsync(base + L.table, table.data(), sizeof(Plane) * n_planes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(base + L.counts, 0, count_bytes, st);
  if (e == hipSuccess) e = launch_labelling(d_table, n_planes, max_n, max_tiles, opt, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_cc_select, dim3((unsigned)n_planes), dim3(kSelectBlock), 0, st, d_table, opt->keep_largest);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    const unsigned g4 = (unsigned)((max_n + kChunk - 1) / kChunk);
    hipLaunchKernelGGL(k_cc_write, dim3(g4, grid_rows((long long)n_planes, g4, kBlock)), dim3(kBlock), 0, st, d_table, (int)n_planes);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts.data(), base + L.counts, count_bytes, hipMemcpyDeviceToHost, st);
  // every mask but the last hands its counters over here; the last goes through mask_finish, which drains the stream for all
  for (int k = 0; k + 1 < n && e == hipSuccess; ++k)
    e = hipMemcpyAsync(h_kept.data() + (size_t)k * DVO_AMD_MAX_LEVELS, made[(size_t)k]->counters, sizeof(int) * made[(size_t)k]->levels,
                       hipMemcpyDeviceToHost, st);
  area_lock.unlock();
  dvo_amd_mask *last = made[(size_t)n - 1];
  made[(size_t)n - 1] = nullptr;  // (mask_finish owns it from here: on failure it is gone)
  dvo_amd_mask *finished = nullptr;
  rc = mask_finish(last, e, st, &finished);
  if (rc) return unwind(rc);
  made[(size_t)n - 1] = finished;
  bracket.read();
  for (int k = 0; k + 1 < n; ++k)
    for (int l = 0; l < made[(size_t)k]->levels; ++l) made[(size_t)k]->kept[l] = h_kept[(size_t)k * DVO_AMD_MAX_LEVELS + l];
  if (counts) {
    size_t r = 0;
    for (int k = 0; k < n; ++k)
      for (int l = 0; l < made[(size_t)k]->levels; ++l, ++r) {
        const unsigned long long *c = h_counts.data() + kPlaneCounts * r;
        long long *o = counts + DVO_AMD_COMPONENTS_COUNTS * r;
        o[0] = (long long)c[0], o[1] = (long long)c[1], o[2] = (long long)c[2], o[3] = made[(size_t)k]->kept[l], o[4] = (long long)c[4],
        o[5] = (long long)c[5];
      }
  }
  for (int k = 0; k < n; ++k) out[k] = made[(size_t)k];
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_component_options(dvo_amd_component_options *opt) {
  if (!opt) return;
  opt->connectivity = 8, opt->max_step = 0.0f, opt->depth_sigmas = 10.0f, opt->keep_largest = 0;
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) opt->min_area[l] = 0, opt->max_area[l] = -1;
}

int dvo_amd_mask_filter_components_many(int n, const dvo_amd_mask *const *masks, const dvo_amd_pyramid *const *depths,
                                        const dvo_amd_mask *const *seeds, const dvo_amd_component_options *opt, dvo_amd_mask **out,
                                        long long *counts) {
  return filter_many("dvo_amd_mask_filter_components_many", false, n, masks, depths, seeds, opt, out, counts);
}

int dvo_amd_mask_filter_components(const dvo_amd_mask *mask, const dvo_amd_pyramid *depth, const dvo_amd_mask *seeds,
                                   const dvo_amd_component_options *opt, dvo_amd_mask **out, long long *counts) {
  static const char *entry = "dvo_amd_mask_filter_components";
  if (out) *out = nullptr;
  if (!out) return invalid(entry, "out is NULL");
  if (!mask && !depth) return invalid(entry, "mask and depth are both NULL");
  return filter_many(entry, true, 1, &mask, &depth, &seeds, opt, out, counts);
}

int dvo_amd_mask_components(const dvo_amd_mask *mask, const dvo_amd_pyramid *depth, const dvo_amd_mask *seeds,
                            const dvo_amd_component_options *opt, int level, int *labels, dvo_amd_component *components, int capacity,
                            int *n_components) {
  static const char *entry = "dvo_amd_mask_components";
  if (n_components) *n_components = 0;
  if (!n_components) return invalid(entry, "n_components is NULL");
  int rc = check_options(entry, opt);
  if (rc) return rc;
  if (capacity < 0) return invalid(entry, "a negative capacity");
  if (capacity > 0 && !components) return invalid(entry, "components is NULL but capacity is not 0");
  std::vector<Item> items(1);
  rc = check_item(entry, "", mask, depth, seeds, &items[0]);
  if (rc) return rc;
  const Item &it = items[0];
  if (level < 0 || level >= it.levels) return invalid(entry, "level " + std::to_string(level) + " is outside the item's " + std::to_string(it.levels) + " levels");
  for (int l = 0; l < it.levels; ++l)  // (not read here, but validated as the filter validates it)
    if (opt->min_area[l] < 0) return invalid(entry, "min_area[" + std::to_string(l) + "] is negative");
  if (!one_device(it, it.device)) return DVO_AMD_ERR_DEVICE_MISMATCH;
  int ndev = 0;
  rc = have_device(&ndev);
  if (rc) return rc;
  const int device = it.device;
  if (device < 0 || device >= ndev || device >= kMaxDevices) return invalid(entry, "no such device");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;
  const size_t n = (size_t)(it.w >> level) * (size_t)(it.h >> level);
  const Layout L = layout(1, align_up(n, 256));
  Bracket bracket(g_timing[device]);
  std::vector<int> h_parent(n), h_roots, h_rec;
  unsigned long long h_counts[kPlaneCounts] = {};
  size_t n_written = 0;
  {
    std::unique_lock<std::mutex> area_lock(device_mutex(device));
    DeviceBuf &area = g_area[device];
    rc = grow_area(area, L.total);
    if (rc) return rc;
    char *base = (char *)area.p;
    std::vector<Plane> table(1);
    int max_n = 1, max_tiles = 1;
    fill_table(table, items, std::vector<int>(1, level), std::vector<int>(1, 1), std::vector<dvo_amd_mask *>(1, nullptr), opt, base, L, &max_n,
               &max_tiles);
    hipError_t e = bracket.begin(st);
    if (e == hipSuccess) e = hipMemcpyAsync(base + L.table, table.data(), sizeof(Plane), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(base + L.counts, 0, sizeof(h_counts), st);
    if (e == hipSuccess) e = launch_labelling((const Plane *)(base + L.table), 1, max_n, max_tiles, opt, st);
    if (e == hipSuccess) e = bracket.end(st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_parent.data(), table[0].parent, sizeof(int) * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_counts, base + L.counts, sizeof(h_counts), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // the roots are the pixels that are their own parent, in ascending order as the rules want them (the device's work list holds
    // them in arrival order); their records lie at their pixel index: one copy up to the last record asked for.  The area stays
    // this call's until the lock goes
    if (e == hipSuccess) {
      for (size_t i = 0; i < n; ++i)
        if (h_parent[i] == (int)i) h_roots.push_back((int)i);
      if (h_roots.size() != (size_t)h_counts[6]) e = hipErrorUnknown;  // (the work list and the label plane disagree: never)
    }
    const size_t want = std::min(h_roots.size(), (size_t)capacity);
    if (e == hipSuccess && want) {
      h_rec.resize(((size_t)h_roots[want - 1] + 1) * kRecInts);
      e = hipMemcpyAsync(h_rec.data(), table[0].rec, sizeof(int) * h_rec.size(), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    n_written = want;
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(st);
      return fail_hip("component labelling", e);
    }
  }
  bracket.read();
  *n_components = (int)h_counts[6];
  if (labels)
    for (size_t i = 0; i < n; ++i) labels[i] = h_parent[i] + 1;  // background is -1 on the device
  for (size_t i = 0; i < n_written; ++i) {
    const int *r = h_rec.data() + (size_t)h_roots[i] * kRecInts;
    dvo_amd_component &c = components[i];
    c.root = h_roots[i], c.area = r[0], c.x0 = r[1], c.y0 = r[2], c.x1 = r[3], c.y1 = r[4], c.seeded = r[5];
  }
  return DVO_AMD_OK;
}

/* instrumentation: with enable != 0 every later dvo_amd_mask_filter_components / _many and dvo_amd_mask_components on `device` is
 * bracketed by two events on the prep stream; *last_ms (may be NULL) receives the device time of the most recent bracketed call */
int dvo_amd_debug_components_timing(int device, int enable, double *last_ms) {
  return timing_entry(g_timing, device, enable, nullptr, nullptr, last_ms);
}

}  // extern "C"
