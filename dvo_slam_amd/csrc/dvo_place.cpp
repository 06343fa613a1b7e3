// The place index: loop-closure candidates by appearance.  dvo_amd_find_constraint_candidates trusts the estimated poses; after a
// long loop, or when tracking is lost, they are exactly what cannot be trusted.  A dvo_amd_place_index keeps one int8 descriptor per
// keyframe on the device -- a coarse level's intensity plane, local mean removed, quantised -- and answers "which keyframes look
// like this one / like this frame": the k keys of highest cosine.  The rule is pinned in include/dvo_amd.h ("Place index");
// tests/place_ref.py restates it in numpy.  The kernels live in dvo_kernels.hip:
//   k_place_describe   ONE launch for all pyramids of a call: a block per pyramid writes the row, its zero padding and its norm
//   k_place_dots       Q . X^T on the int8 matrix instruction (v_mfma_i32_16x16x64_i8), exact int32
//   k_place_topk       a block per query: eligibility, the score, k rounds of arg-max
// This file is the host side: the index object, the argument checks, growth, panels, the copies.  The entries take no context: they
// run on the device's prep stream under the index's own mutex.  1 / sqrt(norm) is formed HERE, in double on the host, so that it is
// correctly rounded and restatable; the device only multiplies.
#include "dvo_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

namespace {

typedef DeviceBuf Buf;  // device memory grown to the largest call (in 64 KiB steps) and kept

}  // namespace

struct dvo_amd_place_index {
  int device = 0;
  int level = 0;
  float gain = 1.0f;
  int w = 0, h = 0, dim = 0;  // fixed by the first add
  int size = 0, capacity = 0;
  signed char *rows = nullptr;  // device, [capacity][dim]
  int *nn = nullptr;            // device, [capacity]
  double *r = nullptr;          // device, [capacity]: the first r_uploaded entries are there (the rest goes up with the next query)
  int r_uploaded = 0;
  std::vector<int> h_nn;        // [size]
  std::vector<double> h_r;      // [size]: 1 / sqrt(nn), 0 where nn == 0
  std::mutex mu;                // one call at a time works on an index: the buffers below are the call's
  Buf ptrs, qrows, dots, io;
};

using namespace dvo_amd;
using namespace dvo_amd::host;

namespace {

constexpr int kInitialCapacity = DVO_AMD_PLACE_INITIAL_CAPACITY;
constexpr size_t kDotsCapBytes = (size_t)DVO_AMD_PLACE_DOTS_CAP_MB << 20;  // the dots of a query call in device scratch: above it, row panels
constexpr int kMaxPanelRows = 1 << 16;

// dvo_amd_debug_place_timing: two events around the launches of the most recent scores / query call (off unless asked for)
DeviceTiming g_timing[kMaxDevices];

int dots_tile() {  // DVO_AMD_PLACE_TILE=1|2|4: the workgroup tile of k_place_dots (tuning; 0 = chosen by the number of queries)
  static const int t = [] {
    const char *e = getenv("DVO_AMD_PLACE_TILE");
    return e ? atoi(e) : 0;
  }();
  return t;
}

int grow(Buf &b, size_t bytes, const char *what) { return grow(b, bytes, 1 << 16, what); }

void release(Buf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr, b.bytes = 0;
}

inline double inv_norm(int nn) { return nn > 0 ? 1.0 / std::sqrt((double)nn) : 0.0; }

int check_query_options(const char *entry, const dvo_amd_place_query_options *opt) {
  if (opt->k < 1 || opt->k > DVO_AMD_PLACE_MAX_K) return invalid(entry, "k is outside 1.." + std::to_string(DVO_AMD_PLACE_MAX_K));
  if (std::isnan(opt->min_score)) return invalid(entry, "min_score is NaN");
  if (opt->exclude_recent < 0) return invalid(entry, "exclude_recent is negative");
  return DVO_AMD_OK;
}

// may these pyramids be described for `ix`: NULL entries, the level, the size (the index's, or the call's first pyramid's)
int check_pyramids(const char *entry, const dvo_amd_place_index *ix, int n, const dvo_amd_pyramid *const *p, const char *what, int *w_out,
                   int *h_out) {
  int w = ix->w, h = ix->h;
  for (int i = 0; i < n; ++i) {
    if (!p[i]) return invalid(entry, std::string(what) + " " + std::to_string(i) + " is NULL");
    if (p[i]->n_levels < ix->level + 1)
      return invalid(entry, std::string(what) + " " + std::to_string(i) + " has fewer than " + std::to_string(ix->level + 1) + " levels");
    const LevelData &L = p[i]->lv[ix->level];
    if (w == 0 && h == 0) w = L.w, h = L.h;
    if (L.w != w || L.h != h)
      return invalid(entry, std::string(what) + " " + std::to_string(i) + ": level " + std::to_string(ix->level) + " is " + std::to_string(L.w) + "x" +
                                std::to_string(L.h) + ", the index holds " + std::to_string(w) + "x" + std::to_string(h));
  }
  if ((long long)w * (long long)h > DVO_AMD_PLACE_MAX_DIM)
    return invalid(entry, "a descriptor of more than " + std::to_string(DVO_AMD_PLACE_MAX_DIM) + " values: use a coarser level");
  *w_out = w, *h_out = h;
  return DVO_AMD_OK;
}

// the descriptors of n pyramids into rows[0..n) and nn[0..n), enqueued on st (the pointer table lives in ix.ptrs)
hipError_t describe(dvo_amd_place_index &ix, int n, const dvo_amd_pyramid *const *p, int w, int h, int dim, signed char *rows, int *nn,
                    std::vector<const float *> &table, hipStream_t st) {
  table.resize((size_t)n);
  for (int i = 0; i < n; ++i) table[(size_t)i] = p[i]->lv[ix.level].r_i;  // the level's intensity plane, row-major w x h
  hipError_t e = hipMemcpyAsync(ix.ptrs.p, table.data(), sizeof(const float *) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_place_describe((const float *const *)ix.ptrs.p, n, w, h, dim, ix.gain, rows, nn, st);
  return e;
}

int panel_rows(int n_queries, int n) {
  const long long fit = (long long)(kDotsCapBytes / (sizeof(int) * (size_t)std::max(n, 1)));
  return (int)std::max<long long>(1, std::min<long long>(std::min<long long>(n_queries, kMaxPanelRows), std::max<long long>(fit / 64 * 64, 64)));
}

// the common end of the two query entries.  Query i is row h_qid[i] of the index (h_qid[i] >= 0) or row i of `frame_rows`; h_rq[i]
// is its 1 / sqrt(norm).  Called with the index's mutex held and the device set; everything is enqueued on st and drained here.
int run_query(dvo_amd_place_index &ix, const char *what, int nq, const std::vector<int> &h_qid, const std::vector<double> &h_rq,
              const signed char *frame_rows, const dvo_amd_place_query_options *opt, int *candidates, double *scores, int *counts,
              hipStream_t st) {
  const int n = ix.size, k = opt->k;
  const size_t nk = (size_t)nq * (size_t)k;
  // io: [r_query nq][scores nq k] doubles, then [query ids nq][candidates nq k][counts nq] ints
  const size_t io_bytes = sizeof(double) * ((size_t)nq + nk) + sizeof(int) * (2 * (size_t)nq + nk);
  int rc = grow(ix.io, io_bytes, "place query");
  if (rc) return rc;
  const int panel = panel_rows(nq, n);
  rc = grow(ix.dots, sizeof(int) * (size_t)panel * (size_t)n, "place dots");
  if (rc) return rc;
  double *d_rq = (double *)ix.io.p, *d_scores = d_rq + nq;
  int *d_qid = (int *)(d_scores + nk), *d_cand = d_qid + nq, *d_counts = d_cand + nk;
  Bracket bracket(g_timing[ix.device]);
  hipError_t e = hipSuccess;
  if (ix.r_uploaded < n) {
    e = hipMemcpyAsync(ix.r + ix.r_uploaded, ix.h_r.data() + ix.r_uploaded, sizeof(double) * (size_t)(n - ix.r_uploaded), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) ix.r_uploaded = n;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(d_rq, h_rq.data(), sizeof(double) * (size_t)nq, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_qid, h_qid.data(), sizeof(int) * (size_t)nq, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = bracket.begin(st);
  for (int q0 = 0; q0 < nq && e == hipSuccess; q0 += panel) {
    const int cnt = std::min(panel, nq - q0);
    e = launch_place_dots(ix.rows, frame_rows ? nullptr : d_qid + q0, frame_rows ? frame_rows + (size_t)q0 * (size_t)ix.dim : nullptr, cnt, ix.rows, n,
                          ix.dim, (int *)ix.dots.p, dots_tile(), st);
    if (e == hipSuccess)
      e = launch_place_topk((const int *)ix.dots.p, cnt, n, d_qid + q0, d_rq + q0, ix.r, k, opt->min_score, opt->exclude_recent,
                            d_cand + (size_t)q0 * k, d_scores + (size_t)q0 * k, d_counts + q0, st);
  }
  if (e == hipSuccess) e = bracket.end(st);
  if (e == hipSuccess) e = hipMemcpyAsync(candidates, d_cand, sizeof(int) * nk, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(scores, d_scores, sizeof(double) * nk, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip(what, e);
  bracket.read();
  return DVO_AMD_OK;
}

void nothing_found(int nq, int k, int *candidates, double *scores, int *counts) {
  for (size_t i = 0; i < (size_t)nq * (size_t)k; ++i) candidates[i] = -1, scores[i] = std::nan("");
  for (int i = 0; i < nq; ++i) counts[i] = 0;
}

}  // namespace

extern "C" {

void dvo_amd_default_place_options(dvo_amd_place_options *opt) {
  if (!opt) return;
  opt->level = 3, opt->gain = 1.0f;
}

void dvo_amd_default_place_query_options(dvo_amd_place_query_options *opt) {
  if (!opt) return;
  opt->k = 5, opt->min_score = 0.0, opt->exclude_recent = 0;
}

int dvo_amd_place_index_create(int device, const dvo_amd_place_options *opt, dvo_amd_place_index **out) {
  static const char *entry = "dvo_amd_place_index_create";
  if (out) *out = nullptr;
  if (!opt || !out) return invalid(entry, "a NULL pointer");
  if (opt->level < 0 || opt->level >= DVO_AMD_MAX_LEVELS) return invalid(entry, "level is outside 0.." + std::to_string(DVO_AMD_MAX_LEVELS - 1));
  if (!std::isfinite(opt->gain) || !(opt->gain > 0.0f)) return invalid(entry, "gain must be finite and positive");
  int ndev = 0;
  const int rc = have_device(&ndev);
  if (rc) return rc;
  if (device < 0 || device >= ndev || device >= kMaxDevices) return invalid(entry, "no such device");
  dvo_amd_place_index *ix = new dvo_amd_place_index();  // (nothing is allocated on the device before the first add)
  ix->device = device, ix->level = opt->level, ix->gain = opt->gain;
  *out = ix;
  return DVO_AMD_OK;
}

void dvo_amd_place_index_destroy(dvo_amd_place_index *ix) {
  if (!ix) return;
  if (hipSetDevice(ix->device) == hipSuccess) {
    if (ix->rows) (void)hipFree(ix->rows);  // (hipFree waits for whatever still uses the memory)
    if (ix->nn) (void)hipFree(ix->nn);
    if (ix->r) (void)hipFree(ix->r);
    release(ix->ptrs), release(ix->qrows), release(ix->dots), release(ix->io);
  }
  delete ix;
}

int dvo_amd_place_index_add(dvo_amd_place_index *ix, int n, const dvo_amd_pyramid *const *pyramids, int *first_id) {
  static const char *entry = "dvo_amd_place_index_add";
  if (first_id) *first_id = -1;
  if (!ix) return invalid(entry, "a NULL pointer");
  if (n < 0) return invalid(entry, "a negative pyramid count");
  if (n > 0 && !pyramids) return invalid(entry, "a NULL pointer");
  std::lock_guard<std::mutex> lk(ix->mu);
  int w = 0, h = 0;
  int rc = check_pyramids(entry, ix, n, pyramids, "pyramid", &w, &h);
  if (rc) return rc;
  if ((long long)ix->size + n > INT_MAX) return invalid(entry, "more than 2^31 - 1 rows");
  for (int i = 0; i < n; ++i)
    if (pyramids[i]->device != ix->device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n == 0) {
    if (first_id) *first_id = ix->size;
    return DVO_AMD_OK;
  }
  const int dim = (w * h + 63) / 64 * 64;
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(ix->device, &st);
  if (rc) return rc;
  rc = grow(ix->ptrs, sizeof(const float *) * (size_t)n, "place table");
  if (rc) return rc;

  // growth: a new allocation of twice the rows (at least DVO_AMD_PLACE_INITIAL_CAPACITY, at least what the call needs), the old rows copied
  signed char *old_rows = nullptr;
  int *old_nn = nullptr;
  double *old_r = nullptr;
  hipError_t e = hipSuccess;
  if (ix->size + n > ix->capacity) {
    long long cap = std::max(ix->capacity, kInitialCapacity);
    while (cap < (long long)ix->size + n) cap *= 2;
    cap = std::min<long long>(cap, INT_MAX);
    signed char *rows = nullptr;
    int *nn = nullptr;
    double *r = nullptr;
    e = hipMalloc((void **)&rows, (size_t)cap * (size_t)dim);
    if (e == hipSuccess) e = hipMalloc((void **)&nn, sizeof(int) * (size_t)cap);
    if (e == hipSuccess) e = hipMalloc((void **)&r, sizeof(double) * (size_t)cap);
    if (e == hipSuccess && ix->size > 0) e = hipMemcpyAsync(rows, ix->rows, (size_t)ix->size * (size_t)dim, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && ix->size > 0) e = hipMemcpyAsync(nn, ix->nn, sizeof(int) * (size_t)ix->size, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(st);
      if (rows) (void)hipFree(rows);
      if (nn) (void)hipFree(nn);
      if (r) (void)hipFree(r);
      return e == hipErrorOutOfMemory ? (int)DVO_AMD_ERR_OUT_OF_MEMORY : fail_hip("place index growth", e);
    }
    old_rows = ix->rows, old_nn = ix->nn, old_r = ix->r;
    ix->rows = rows, ix->nn = nn, ix->r = r, ix->capacity = (int)cap;
    ix->r_uploaded = 0;  // (the host keeps every r: the next query uploads them)
  }
  std::vector<const float *> table;
  std::vector<int> norms((size_t)n);
  e = describe(*ix, n, pyramids, w, h, dim, ix->rows + (size_t)ix->size * (size_t)dim, ix->nn + ix->size, table, st);
  if (e == hipSuccess) e = hipMemcpyAsync(norms.data(), ix->nn + ix->size, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // the call's one synchronisation
  if (e == hipSuccess) e = es;
  if (old_rows) (void)hipFree(old_rows);
  if (old_nn) (void)hipFree(old_nn);
  if (old_r) (void)hipFree(old_r);
  if (e != hipSuccess) return fail_hip("place index add", e);  // (the rows behind `size` are scratch: the index is as it was)
  for (int i = 0; i < n; ++i) ix->h_nn.push_back(norms[(size_t)i]), ix->h_r.push_back(inv_norm(norms[(size_t)i]));
  if (first_id) *first_id = ix->size;
  ix->w = w, ix->h = h, ix->dim = dim, ix->size += n;
  return DVO_AMD_OK;
}

int dvo_amd_place_index_info(const dvo_amd_place_index *index, int *size, int *width, int *height, int *dim) {
  if (!index) return invalid("dvo_amd_place_index_info", "a NULL pointer");
  dvo_amd_place_index &ix = *const_cast<dvo_amd_place_index *>(index);
  std::lock_guard<std::mutex> lk(ix.mu);
  if (size) *size = ix.size;
  if (width) *width = ix.w;
  if (height) *height = ix.h;
  if (dim) *dim = ix.dim;
  return DVO_AMD_OK;
}

int dvo_amd_place_index_download(const dvo_amd_place_index *index, int first, int n, signed char *descriptors, int *norms) {
  static const char *entry = "dvo_amd_place_index_download";
  if (!index) return invalid(entry, "a NULL pointer");
  if (n < 0) return invalid(entry, "a negative row count");
  dvo_amd_place_index &ix = *const_cast<dvo_amd_place_index *>(index);
  std::lock_guard<std::mutex> lk(ix.mu);
  if (first < 0 || (long long)first + n > ix.size) return invalid(entry, "rows outside the index");
  const int rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;
  if (norms) std::copy(ix.h_nn.begin() + first, ix.h_nn.begin() + first + n, norms);
  if (descriptors) {
    HIP_TRY(hipSetDevice(ix.device));
    HIP_TRY(hipMemcpy(descriptors, ix.rows + (size_t)first * (size_t)ix.dim, (size_t)n * (size_t)ix.dim, hipMemcpyDeviceToHost));
  }
  return DVO_AMD_OK;
}

int dvo_amd_place_scores(const dvo_amd_place_index *index, int n_queries, const int *query_ids, int first, int n, int *dots) {
  static const char *entry = "dvo_amd_place_scores";
  if (!index) return invalid(entry, "a NULL pointer");
  if (n_queries < 0) return invalid(entry, "a negative query count");
  if (n < 0) return invalid(entry, "a negative key count");
  if (n_queries > 0 && !query_ids) return invalid(entry, "a NULL pointer");
  if (n_queries > 0 && n > 0 && !dots) return invalid(entry, "a NULL pointer");
  dvo_amd_place_index &ix = *const_cast<dvo_amd_place_index *>(index);
  std::lock_guard<std::mutex> lk(ix.mu);
  for (int i = 0; i < n_queries; ++i)
    if (query_ids[i] < 0 || query_ids[i] >= ix.size) return invalid(entry, "query " + std::to_string(i) + ": id " + std::to_string(query_ids[i]) + " is outside the index");
  if (first < 0 || (long long)first + n > ix.size) return invalid(entry, "keys outside the index");
  int rc = have_device();
  if (rc) return rc;
  if (n_queries == 0 || n == 0) return DVO_AMD_OK;
  HIP_TRY(hipSetDevice(ix.device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(ix.device, &st);
  if (rc) return rc;
  rc = grow(ix.io, sizeof(int) * (size_t)n_queries, "place scores");
  if (rc) return rc;
  const int panel = panel_rows(n_queries, n);
  rc = grow(ix.dots, sizeof(int) * (size_t)panel * (size_t)n, "place dots");
  if (rc) return rc;
  int *d_qid = (int *)ix.io.p;
  Bracket bracket(g_timing[ix.device]);
  hipError_t e = hipMemcpyAsync(d_qid, query_ids, sizeof(int) * (size_t)n_queries, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = bracket.begin(st);
  for (int q0 = 0; q0 < n_queries && e == hipSuccess; q0 += panel) {
    const int cnt = std::min(panel, n_queries - q0);
    e = launch_place_dots(ix.rows, d_qid + q0, nullptr, cnt, ix.rows + (size_t)first * (size_t)ix.dim, n, ix.dim, (int *)ix.dots.p, dots_tile(), st);
    if (e == hipSuccess && q0 + cnt == n_queries) e = bracket.end(st);
    if (e == hipSuccess) e = hipMemcpyAsync(dots + (size_t)q0 * (size_t)n, ix.dots.p, sizeof(int) * (size_t)cnt * (size_t)n, hipMemcpyDeviceToHost, st);
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("place scores", e);
  bracket.read();
  return DVO_AMD_OK;
}

int dvo_amd_place_query(const dvo_amd_place_index *index, int n_queries, const int *query_ids, const dvo_amd_place_query_options *opt,
                        int *candidates, double *scores, int *counts) {
  static const char *entry = "dvo_amd_place_query";
  if (!index || !opt) return invalid(entry, "a NULL pointer");
  if (n_queries < 0) return invalid(entry, "a negative query count");
  if (n_queries > 0 && (!query_ids || !candidates || !scores || !counts)) return invalid(entry, "a NULL pointer");
  int rc = check_query_options(entry, opt);
  if (rc) return rc;
  dvo_amd_place_index &ix = *const_cast<dvo_amd_place_index *>(index);
  std::lock_guard<std::mutex> lk(ix.mu);
  for (int i = 0; i < n_queries; ++i)
    if (query_ids[i] < 0 || query_ids[i] >= ix.size) return invalid(entry, "query " + std::to_string(i) + ": id " + std::to_string(query_ids[i]) + " is outside the index");
  rc = have_device();
  if (rc) return rc;
  if (n_queries == 0) return DVO_AMD_OK;
  HIP_TRY(hipSetDevice(ix.device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(ix.device, &st);
  if (rc) return rc;
  std::vector<int> qid(query_ids, query_ids + n_queries);
  std::vector<double> rq((size_t)n_queries);
  for (int i = 0; i < n_queries; ++i) rq[(size_t)i] = ix.h_r[(size_t)query_ids[i]];
  return run_query(ix, "place query", n_queries, qid, rq, nullptr, opt, candidates, scores, counts, st);
}

int dvo_amd_place_query_frames(const dvo_amd_place_index *index, int n_queries, const dvo_amd_pyramid *const *frames,
                               const dvo_amd_place_query_options *opt, int *candidates, double *scores, int *counts) {
  static const char *entry = "dvo_amd_place_query_frames";
  if (!index || !opt) return invalid(entry, "a NULL pointer");
  if (n_queries < 0) return invalid(entry, "a negative query count");
  if (n_queries > 0 && (!frames || !candidates || !scores || !counts)) return invalid(entry, "a NULL pointer");
  int rc = check_query_options(entry, opt);
  if (rc) return rc;
  dvo_amd_place_index &ix = *const_cast<dvo_amd_place_index *>(index);
  std::lock_guard<std::mutex> lk(ix.mu);
  int w = 0, h = 0;
  rc = check_pyramids(entry, &ix, n_queries, frames, "frame", &w, &h);
  if (rc) return rc;
  for (int i = 0; i < n_queries; ++i)
    if (frames[i]->device != ix.device) return DVO_AMD_ERR_DEVICE_MISMATCH;
  rc = have_device();
  if (rc) return rc;
  if (n_queries == 0) return DVO_AMD_OK;
  if (ix.size == 0) {  // an empty index: nothing to compare with, nothing to launch
    nothing_found(n_queries, opt->k, candidates, scores, counts);
    return DVO_AMD_OK;
  }
  HIP_TRY(hipSetDevice(ix.device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(ix.device, &st);
  if (rc) return rc;
  rc = grow(ix.ptrs, sizeof(const float *) * (size_t)n_queries, "place table");
  if (rc) return rc;
  const size_t row_bytes = align_up((size_t)n_queries * (size_t)ix.dim, 256);
  rc = grow(ix.qrows, row_bytes + sizeof(int) * (size_t)n_queries, "place frames");
  if (rc) return rc;
  signed char *d_rows = (signed char *)ix.qrows.p;
  int *d_nn = (int *)((char *)ix.qrows.p + row_bytes);
  std::vector<const float *> table;
  std::vector<int> norms((size_t)n_queries);
  hipError_t e = describe(ix, n_queries, frames, ix.w, ix.h, ix.dim, d_rows, d_nn, table, st);
  if (e == hipSuccess) e = hipMemcpyAsync(norms.data(), d_nn, sizeof(int) * (size_t)n_queries, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // the norms are needed on the host: r_query is formed there
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail_hip("place query (frames)", e);
  std::vector<int> qid((size_t)n_queries, -1);
  std::vector<double> rq((size_t)n_queries);
  for (int i = 0; i < n_queries; ++i) rq[(size_t)i] = inv_norm(norms[(size_t)i]);
  return run_query(ix, "place query (frames)", n_queries, qid, rq, d_rows, opt, candidates, scores, counts, st);
}

/* instrumentation: with enable != 0 the kernel launches of every later dvo_amd_place_scores / _query / _query_frames on `device` are
 * bracketed by two events on the prep stream; *last_ms (may be NULL) receives the device time of the most recent bracketed call */
int dvo_amd_debug_place_timing(int device, int enable, double *last_ms) {
  return timing_entry(g_timing, device, enable, nullptr, nullptr, last_ms);
}

}  // extern "C"
