// Masks from what the tracker itself knows: dvo_amd_mask_from_residuals / _many keep the pixels of a reference pyramid whose
// residuals at a transformation are inliers of the t-distribution -- Mahalanobis distance under a precision at most a threshold --
// and drop what the weights would down-weight: moving objects, specular surfaces, depth ghosts.  The fourth producer of masks next
// to dvo_mask.cpp, dvo_budget.cpp and dvo_mask_ops.cpp: every result is an ordinary dvo_amd_mask (mask_alloc / mask_finish), the
// pyramids are only read.  The rule is pinned in include/dvo_amd.h under "Residual masks"; tests/residual_mask_ref.py restates it.
//
// The kernel, k_residual_mask, lives in dvo_kernels.hip next to the residual stage it calls.  This file is the host side: the
// argument checks, the per-(pair, level) record table in a kept per-device area, ONE launch for all pairs and levels of a call on
// the device's prep stream and ONE synchronisation (mask_finish's).  A context gives its device and its reciprocal mode; no
// tracker slot is used, no selection is built or looked up, and the context's queue may be busy.
#include "dvo_internal.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>

using namespace dvo_amd;
using namespace dvo_amd::host;

static_assert(DVO_AMD_RESIDUAL_MASK_COUNTS == 5, "evaluated, invalid, inlier, outlier, kept");

namespace {

// the record table and the counter blocks of the call in flight (grown to the largest call and kept; used with the device's mutex
// held from the table's upload to the last thing enqueued that touches it, as dvo_amd_mask_warp_many's area)
DeviceBuf g_area[kMaxDevices];

void drop(dvo_amd_mask *m) {
  (void)hipFree(m->mem);
  delete m;
}

int from_residuals_many(const char *entry, dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                        const dvo_amd_pyramid *const *currents, const double *T, const dvo_amd_residual_mask_options *opts,
                        dvo_amd_mask **out, long long *counts, float *const *distance) {
  if (out && n > 0)
    for (int k = 0; k < n; ++k) out[k] = nullptr;
  if (n < 0) return invalid(entry, "a negative count");
  if (!ctx || !references || !currents || !T || !opts || !out) return invalid(entry, "a NULL pointer");
  size_t n_records = 0;
  bool mismatch = false;
  for (int k = 0; k < n; ++k) {
    const std::string pair = "pair " + std::to_string(k);
    const dvo_amd_pyramid *ref = references[k], *cur = currents[k];
    if (!ref || !cur) return invalid(entry, pair + ": a NULL pyramid");
    if (!finite_all(T + 16 * (size_t)k, 16)) return invalid(entry, pair + ": the transformation has a non-finite entry");
    const dvo_amd_residual_mask_options &o = opts[k];
    for (int l = 0; l < ref->n_levels && l < DVO_AMD_MAX_LEVELS; ++l) {
      const float *P = o.precision[l];
      if (!finite_all(P, 4)) return invalid(entry, pair + ": precision[" + std::to_string(l) + "] has a non-finite entry");
      if (P[0] == 0.0f && P[1] == 0.0f && P[2] == 0.0f && P[3] == 0.0f)
        return invalid(entry, pair + ": precision not set for level " + std::to_string(l) + " (all zero)");
    }
    for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l)
      if (!(o.max_distance[l] >= 0.0f))  // (false for NaN; +inf passes)
        return invalid(entry, pair + ": max_distance[" + std::to_string(l) + "] is NaN or negative");
    for (int l = 0; l < ref->n_levels; ++l) {  // what dvo_amd_residuals asks of a level pair
      const int rc = check_level_pair(ctx, ref, cur, l);
      if (rc == DVO_AMD_ERR_TOO_FEW_LEVELS)
        return invalid(entry, pair + ": the reference has " + std::to_string(ref->n_levels) + " levels but the current has " +
                                  std::to_string(cur->n_levels));
      if (rc == DVO_AMD_ERR_DEVICE_MISMATCH) mismatch = true;  // (reported behind every argument error; the sizes are still looked at)
      if (rc == DVO_AMD_ERR_INVALID_ARGUMENT || ref->lv[l].w != cur->lv[l].w || ref->lv[l].h != cur->lv[l].h)
        return invalid(entry, pair + ": level " + std::to_string(l) + " is " + std::to_string(ref->lv[l].w) + "x" +
                                  std::to_string(ref->lv[l].h) + " in the reference but " + std::to_string(cur->lv[l].w) + "x" +
                                  std::to_string(cur->lv[l].h) + " in the current");
    }
    n_records += (size_t)ref->n_levels;
  }
  if (ctx->rcp.table)
    return invalid(entry, "the context is in the host-rcpps reciprocal mode, which this entry does not cover (dvo_amd_set_reciprocal_mode)");
  if (mismatch) return DVO_AMD_ERR_DEVICE_MISMATCH;
  int rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;
  for (int k = 0; k < n; ++k) {
    rc = check_mask_size(entry, references[k]->lv[0].w, references[k]->lv[0].h, references[k]->n_levels);
    if (rc) return rc;
  }
  if (n_records > (size_t)(1 << 24)) return invalid(entry, "more than 2^24 (pair, level) records");

  const int device = ctx->device;
  std::vector<dvo_amd_mask *> made((size_t)n, nullptr);
  float *d_distance = nullptr;  // (single call with distance planes: one allocation for all levels, freed before the return)
  hipStream_t st = nullptr;
  auto unwind = [&](int status) {
    if (st) (void)hipStreamSynchronize(st);
    for (dvo_amd_mask *m : made)
      if (m) drop(m);
    if (d_distance) (void)hipFree(d_distance);
    return status;
  };
  for (int k = 0; k < n; ++k) {
    const dvo_amd_pyramid *r = references[k];
    rc = mask_alloc(entry, device, r->lv[0].w, r->lv[0].h, r->n_levels, &made[(size_t)k], &st);
    if (rc) return unwind(rc);
  }
  size_t distance_at[DVO_AMD_MAX_LEVELS] = {};
  if (distance) {  // (n == 1)
    size_t floats = 0;
    for (int l = 0; l < references[0]->n_levels; ++l) distance_at[l] = floats, floats += align_up((size_t)references[0]->lv[l].n, 64);
    const hipError_t ed = hipMalloc((void **)&d_distance, sizeof(float) * floats);
    if (ed != hipSuccess) {
      d_distance = nullptr;
      return unwind(ed == hipErrorOutOfMemory ? (int)DVO_AMD_ERR_OUT_OF_MEMORY : fail_hip("hipMalloc (distance planes)", ed));
    }
  }
  // the counter blocks lead the area (zeroed as one block that starts at the allocation's start), the table follows
  const size_t count_bytes = align_up(sizeof(unsigned) * kRmWords * n_records, 256), table_bytes = sizeof(ResidualMaskRecord) * n_records;
  std::unique_lock<std::mutex> area_lock(device_mutex(device));
  DeviceBuf &area = g_area[device];
  rc = grow(area, count_bytes + table_bytes, 1 << 16, "residual mask table");
  if (rc) {
    area_lock.unlock();
    return unwind(rc);
  }
  unsigned *d_counts = (unsigned *)area.p;
  ResidualMaskRecord *d_table = (ResidualMaskRecord *)((char *)area.p + count_bytes);
  std::vector<ResidualMaskRecord> table(n_records);
  int max_n = 1;
  size_t r = 0;
  for (int k = 0; k < n; ++k) {
    float Tf[16];
    for (int i = 0; i < 16; ++i) Tf[i] = (float)T[16 * (size_t)k + i];  // transformation.cast<float>(), as dvo_amd_error_image
    const dvo_amd_residual_mask_options &o = opts[k];
    for (int l = 0; l < references[k]->n_levels; ++l, ++r) {
      const LevelData &A = references[k]->lv[l], &C = currents[k]->lv[l];
      ResidualMaskRecord &R = table[r];
      R.z = A.z_plane, R.zd = A.c_b, R.ri = A.r_i, R.tx = A.tx, R.ty = A.ty;
      R.cur = currents[k]->cur_desc + l;
      R.out = made[(size_t)k]->plane[l], R.kept = made[(size_t)k]->counters + l;
      R.distance = d_distance ? d_distance + distance_at[l] : nullptr;
      R.counts = d_counts + kRmWords * r;
      R.w = A.w, R.n = A.n;
      kt_from_float_transform(C, Tf, R.kt);
      for (int i = 0; i < 4; ++i) R.P[i] = o.precision[l][i];
      R.max_distance = o.max_distance[l];
      R.invalid_keep = o.invalid_keep, R.unevaluated_keep = o.unevaluated_keep;
      max_n = std::max(max_n, R.n);
    }
  }
  std::vector<unsigned> h_counts(kRmWords * n_records);
  std::vector<int> h_kept((size_t)n * DVO_AMD_MAX_LEVELS, 0);
  hipError_t e = hipMemsetAsync(d_counts, 0, count_bytes, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_table, table.data(), table_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_residual_mask(d_table, (int)n_records, max_n, st);
  if (e == hipSuccess && counts) e = hipMemcpyAsync(h_counts.data(), d_counts, sizeof(unsigned) * kRmWords * n_records, hipMemcpyDeviceToHost, st);
  if (distance)
    for (int l = 0; l < references[0]->n_levels && e == hipSuccess; ++l)
      if (distance[l])
        e = hipMemcpyAsync(distance[l], d_distance + distance_at[l], sizeof(float) * (size_t)references[0]->lv[l].n, hipMemcpyDeviceToHost, st);
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
  if (d_distance) (void)hipFree(d_distance), d_distance = nullptr;
  for (int k = 0; k + 1 < n; ++k)
    for (int l = 0; l < made[(size_t)k]->levels; ++l) made[(size_t)k]->kept[l] = h_kept[(size_t)k * DVO_AMD_MAX_LEVELS + l];
  if (counts) {
    r = 0;
    for (int k = 0; k < n; ++k)
      for (int l = 0; l < made[(size_t)k]->levels; ++l, ++r) {
        long long *c = counts + DVO_AMD_RESIDUAL_MASK_COUNTS * r;
        const unsigned *h = h_counts.data() + kRmWords * r;
        c[0] = h[kRmEvaluated], c[1] = h[kRmInvalid], c[2] = h[kRmInlier], c[3] = h[kRmOutlier], c[4] = made[(size_t)k]->kept[l];
      }
  }
  for (int k = 0; k < n; ++k) out[k] = made[(size_t)k];
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_residual_mask_options(dvo_amd_residual_mask_options *opt) {
  if (!opt) return;
  for (int l = 0; l < DVO_AMD_MAX_LEVELS; ++l) {
    for (int i = 0; i < 4; ++i) opt->precision[l][i] = 0.0f;
    opt->max_distance[l] = 9.2103f;  // -2 ln 0.01: the 99 % point of chi-square with two degrees of freedom
  }
  opt->invalid_keep = 0, opt->unevaluated_keep = 0;
}

int dvo_amd_mask_from_residuals_many(dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                                     const dvo_amd_pyramid *const *currents, const double *T, const dvo_amd_residual_mask_options *opts,
                                     dvo_amd_mask **out, long long *counts) {
  return from_residuals_many("dvo_amd_mask_from_residuals_many", ctx, n, references, currents, T, opts, out, counts, nullptr);
}

int dvo_amd_mask_from_residuals(dvo_amd_context *ctx, const dvo_amd_pyramid *reference, const dvo_amd_pyramid *current, const double *T,
                                const dvo_amd_residual_mask_options *opt, dvo_amd_mask **out, long long *counts, float *const *distance) {
  static const char *entry = "dvo_amd_mask_from_residuals";
  if (out) *out = nullptr;
  if (!ctx || !reference || !current || !T || !opt || !out) return invalid(entry, "a NULL pointer");
  return from_residuals_many(entry, ctx, 1, &reference, &current, T, opt, out, counts, distance);
}

}  // extern "C"
