// Pose scoring: dvo_amd_score_poses / _many evaluate many candidate transformations of a pair at one coarse level and return, per
// hypothesis, the integer sums a ranking needs -- the step between "looks alike" (the place index) and "align from here" (match,
// the validator).  dvo_amd_pose_grid builds the usual hypothesis set, dvo_amd_rank_poses picks the best few; both are host-only.
// The rule is pinned in include/dvo_amd.h under "Pose scoring"; tests/pose_score_ref.py restates what is new in it.
//
// The kernels, k_score_q3 and k_score_poses, live in dvo_kernels.hip next to the residual stage they call.  This file is the host
// side, modelled on dvo_mask_residual.cpp: the argument checks, then one kept per-device area holding the zeroed sums, the
// (reference, level) entries, the record table, the item table and the K T tables of the call; ONE memset, ONE upload, the two
// launches and ONE copy back on the device's prep stream, ONE synchronisation.  A context gives its device and its reciprocal
// mode; no tracker slot is used, no selection is built or looked up, and the context's queue may be busy.
#include "dvo_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <utility>

using namespace dvo_amd;
using namespace dvo_amd::host;

static_assert(sizeof(dvo_amd_pose_score) == 48, "four counts and two sums of 64 bits");

namespace {

constexpr float kMaxMaxDistance = 1024.0f;  // q(max_distance) <= 2^20: a lane's four costs and a wave's sum stay inside 32 bits
constexpr size_t kMaxHypotheses = (size_t)1 << 22;  // of a call: 80 bytes each in the kept area

DeviceBuf g_area[kMaxDevices];

// q(x) = (uint32) floor(x * 1024.0f) in fp32 for 0 <= x <= 1024: the product is exact
unsigned q_of(float x) { return (unsigned)std::floor(x * 1024.0f); }

int score_many(const char *entry, dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
               const dvo_amd_pyramid *const *currents, const int *m, const double *T, const dvo_amd_pose_score_options *opts,
               dvo_amd_pose_score *scores) {
  if (n < 0) return invalid(entry, "a negative count (n < 0)");
  if (!ctx || !references || !currents || !m || !T || !opts || !scores) return invalid(entry, "a NULL pointer");
  size_t total = 0, n_items = 0;
  bool mismatch = false;
  for (int k = 0; k < n; ++k) {
    const std::string pair = "pair " + std::to_string(k);
    const dvo_amd_pyramid *ref = references[k], *cur = currents[k];
    if (!ref || !cur) return invalid(entry, pair + ": a NULL pyramid");
    if (m[k] < 1) return invalid(entry, pair + ": m = " + std::to_string(m[k]) + " hypotheses (at least 1)");
    const dvo_amd_pose_score_options &o = opts[k];
    const int l = o.level;
    if (l < 0 || l >= DVO_AMD_MAX_LEVELS || l >= ref->n_levels || l >= cur->n_levels)
      return invalid(entry, pair + ": level " + std::to_string(l) + " is out of range (the reference has " + std::to_string(ref->n_levels) +
                                " levels, the current " + std::to_string(cur->n_levels) + ")");
    const int rc = check_level_pair(ctx, ref, cur, l);  // what dvo_amd_residuals asks of a level pair
    if (rc == DVO_AMD_ERR_DEVICE_MISMATCH) mismatch = true;  // (reported behind every argument error; the sizes are still looked at)
    if (rc == DVO_AMD_ERR_INVALID_ARGUMENT || ref->lv[l].w != cur->lv[l].w || ref->lv[l].h != cur->lv[l].h)
      return invalid(entry, pair + ": level " + std::to_string(l) + " is " + std::to_string(ref->lv[l].w) + "x" + std::to_string(ref->lv[l].h) +
                                " in the reference but " + std::to_string(cur->lv[l].w) + "x" + std::to_string(cur->lv[l].h) + " in the current");
    if (!finite_all(o.precision, 4)) return invalid(entry, pair + ": the precision has a non-finite entry");
    if (o.precision[0] == 0.0f && o.precision[1] == 0.0f && o.precision[2] == 0.0f && o.precision[3] == 0.0f)
      return invalid(entry, pair + ": precision not set (all zero)");
    if (!std::isfinite(o.max_distance) || !(o.max_distance > 0.0f) || o.max_distance > kMaxMaxDistance)
      return invalid(entry, pair + ": max_distance must be finite, > 0 and <= 1024");
    if (std::isnan(o.invalid_distance) || std::isinf(o.invalid_distance) || o.invalid_distance > o.max_distance)
      return invalid(entry, pair + ": invalid_distance must be finite and <= max_distance (negative: = max_distance)");
    if (total + (size_t)m[k] > kMaxHypotheses) return invalid(entry, "more than 2^22 hypotheses in one call");
    if (!finite_all(T + 16 * total, 16 * m[k])) return invalid(entry, pair + ": a transformation has a non-finite entry");
    total += (size_t)m[k];
    n_items += ((size_t)m[k] + kPoseScoreTile - 1) / kPoseScoreTile;
  }
  if (ctx->rcp.table)
    return invalid(entry, "the context is in the host-rcpps reciprocal mode, which this entry does not cover (dvo_amd_set_reciprocal_mode)");
  if (mismatch) return DVO_AMD_ERR_DEVICE_MISMATCH;
  int rc = have_device();
  if (rc) return rc;
  if (n == 0) return DVO_AMD_OK;

  const int device = ctx->device;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  rc = device_prep_stream(device, &st);
  if (rc) return rc;

  // the (reference, level) entries of the call: one per distinct pair of the two, whatever number of records score it
  std::map<std::pair<const dvo_amd_pyramid *, int>, int> level_of;
  std::vector<int> record_level((size_t)n);
  for (int k = 0; k < n; ++k) {
    const auto key = std::make_pair(references[k], opts[k].level);
    const auto at = level_of.find(key);
    record_level[(size_t)k] = at != level_of.end() ? at->second : (level_of[key] = (int)level_of.size());
  }
  const size_t n_levels = level_of.size();
  // the area: the sums lead it (zeroed as one block), then what is uploaded as one block
  const size_t sums_bytes = align_up(sizeof(unsigned long long) * kPsWords * total, 256);
  const size_t levels_at = 0, records_at = align_up(sizeof(PoseScoreLevel) * n_levels, 256);
  const size_t items_at = records_at + align_up(sizeof(PoseScoreRecord) * (size_t)n, 256);
  const size_t kt_at = items_at + align_up(sizeof(int2) * n_items, 256);
  const size_t upload_bytes = kt_at + sizeof(float) * 12 * total;
  std::vector<char> staged(upload_bytes, 0);
  PoseScoreLevel *h_levels = (PoseScoreLevel *)(staged.data() + levels_at);
  PoseScoreRecord *h_records = (PoseScoreRecord *)(staged.data() + records_at);
  int2 *h_items = (int2 *)(staged.data() + items_at);
  float *h_kt = (float *)(staged.data() + kt_at);

  std::unique_lock<std::mutex> area_lock(device_mutex(device));
  DeviceBuf &area = g_area[device];
  rc = grow(area, sums_bytes + upload_bytes, 1 << 16, "pose score area");
  if (rc) return rc;
  unsigned long long *d_sums = (unsigned long long *)area.p;
  char *d_upload = (char *)area.p + sums_bytes;
  PoseScoreLevel *d_levels = (PoseScoreLevel *)(d_upload + levels_at);
  const float *d_kt = (const float *)(d_upload + kt_at);

  int max_n = 1;
  size_t first = 0, item = 0;
  for (int k = 0; k < n; ++k) {
    const dvo_amd_pose_score_options &o = opts[k];
    const LevelData &A = references[k]->lv[o.level], &C = currents[k]->lv[o.level];
    PoseScoreLevel &L = h_levels[record_level[(size_t)k]];
    L.z = A.z_plane, L.zd = A.c_b, L.n = A.n, L.q3 = -1;
    PoseScoreRecord &R = h_records[k];
    R.z = A.z_plane, R.zd = A.c_b, R.ri = A.r_i, R.tx = A.tx, R.ty = A.ty;
    R.cur = currents[k]->cur_desc + o.level;
    R.level = d_levels + record_level[(size_t)k];
    R.kt = d_kt + 12 * first;
    R.sums = d_sums + kPsWords * first;
    R.w = A.w, R.n = A.n, R.m = m[k];
    for (int i = 0; i < 4; ++i) R.P[i] = o.precision[i];
    R.max_distance = o.max_distance;
    R.q_max = q_of(o.max_distance);
    max_n = std::max(max_n, R.n);
    for (int j = 0; j < m[k]; ++j) {
      float Tf[16];
      for (int i = 0; i < 16; ++i) Tf[i] = (float)T[16 * (first + (size_t)j) + i];  // transformation.cast<float>(), as dvo_amd_mask_from_residuals
      kt_from_float_transform(C, Tf, h_kt + 12 * (first + (size_t)j));
    }
    for (int j = 0; j < m[k]; j += kPoseScoreTile) h_items[item++] = make_int2(k, j);
    first += (size_t)m[k];
  }
  std::vector<unsigned long long> h_sums(kPsWords * total);
  hipError_t e = hipMemsetAsync(d_sums, 0, sums_bytes, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_upload, staged.data(), upload_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = launch_score_poses(d_levels, (int)n_levels, (const PoseScoreRecord *)(d_upload + records_at), (const int2 *)(d_upload + items_at),
                           (int)n_items, max_n, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_sums.data(), d_sums, sizeof(unsigned long long) * kPsWords * total, hipMemcpyDeviceToHost, st);
  area_lock.unlock();  // (a later call's work on the area is enqueued behind this one's, on the same stream)
  const hipError_t es = hipStreamSynchronize(st);  // (also after a failed enqueue: h_sums and staged outlive what was enqueued)
  if (e != hipSuccess) return fail_hip("pose scoring (enqueue)", e);
  if (es != hipSuccess) return fail_hip("hipStreamSynchronize (pose scoring)", es);

  first = 0;
  for (int k = 0; k < n; ++k) {
    const dvo_amd_pose_score_options &o = opts[k];
    const unsigned long long q_invalid = q_of(o.invalid_distance < 0.0f ? o.max_distance : o.invalid_distance);
    for (int j = 0; j < m[k]; ++j) {
      const unsigned long long *s = h_sums.data() + kPsWords * (first + (size_t)j);
      dvo_amd_pose_score &out = scores[first + (size_t)j];
      out.invalid = (long long)s[kPsInvalid], out.inlier = (long long)s[kPsInlier], out.outlier = (long long)s[kPsOutlier];
      out.evaluated = out.invalid + out.inlier + out.outlier;
      out.cost = s[kPsCost];
      out.total = out.cost + s[kPsInvalid] * q_invalid;
    }
    first += (size_t)m[k];
  }
  return DVO_AMD_OK;
}

}  // namespace

extern "C" {

void dvo_amd_default_pose_score_options(dvo_amd_pose_score_options *opt) {
  if (!opt) return;
  opt->level = 0;
  for (int i = 0; i < 4; ++i) opt->precision[i] = 0.0f;
  opt->max_distance = 9.2103f;  // -2 ln 0.01, as dvo_amd_default_residual_mask_options
  opt->invalid_distance = -1.0f;  // negative: = max_distance
}

int dvo_amd_score_poses_many(dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references, const dvo_amd_pyramid *const *currents,
                             const int *m, const double *T, const dvo_amd_pose_score_options *opts, dvo_amd_pose_score *scores) {
  return score_many("dvo_amd_score_poses_many", ctx, n, references, currents, m, T, opts, scores);
}

int dvo_amd_score_poses(dvo_amd_context *ctx, const dvo_amd_pyramid *reference, const dvo_amd_pyramid *current, int m, const double *T,
                        const dvo_amd_pose_score_options *opt, dvo_amd_pose_score *scores) {
  static const char *entry = "dvo_amd_score_poses";
  if (!ctx || !reference || !current || !T || !opt || !scores) return invalid(entry, "a NULL pointer");
  return score_many(entry, ctx, 1, &reference, &current, &m, T, opt, scores);
}

int dvo_amd_rank_poses(const dvo_amd_pose_score *scores, int m, int k, int *order, int *n_out) {
  static const char *entry = "dvo_amd_rank_poses";
  if (n_out) *n_out = 0;
  if (!scores || !order || !n_out) return invalid(entry, "a NULL pointer");
  if (m < 0 || k < 0) return invalid(entry, "a negative count");
  std::vector<int> all((size_t)m);
  std::iota(all.begin(), all.end(), 0);
  const int keep = std::min(k, m);
  std::partial_sort(all.begin(), all.begin() + keep, all.end(), [&](int a, int b) {
    return scores[a].total != scores[b].total ? scores[a].total < scores[b].total : a < b;  // ties go to the lower index
  });
  std::copy(all.begin(), all.begin() + keep, order);
  *n_out = keep;
  return DVO_AMD_OK;
}

int dvo_amd_pose_grid(const dvo_amd_pose_grid_options *opt, const double *T_centre, double *T_out, int capacity, int *n_out) {
  static const char *entry = "dvo_amd_pose_grid";
  if (n_out) *n_out = 0;
  if (!opt || !T_centre || !n_out) return invalid(entry, "a NULL pointer");
  if (capacity < 0) return invalid(entry, "a negative capacity");
  long long count = 1;
  for (int a = 0; a < 6; ++a) {
    if (opt->count[a] < 1 || opt->count[a] % 2 == 0)
      return invalid(entry, "count[" + std::to_string(a) + "] = " + std::to_string(opt->count[a]) + " (odd and at least 1)");
    if (!std::isfinite(opt->step[a])) return invalid(entry, "step[" + std::to_string(a) + "] is not finite");
    count *= opt->count[a];
    if (count > (long long)kMaxHypotheses) return invalid(entry, "more than 2^22 hypotheses");
  }
  if (!finite_all(T_centre, 16)) return invalid(entry, "the centre has a non-finite entry");
  *n_out = (int)count;
  if (!T_out) return DVO_AMD_OK;  // (the count alone)
  if ((long long)capacity < count)
    return invalid(entry, "capacity " + std::to_string(capacity) + " is less than the " + std::to_string(count) + " hypotheses of the grid");
  int idx[6] = {0, 0, 0, 0, 0, 0};  // (vx, vy, vz, wx, wy, wz): the last runs fastest
  for (long long j = 0; j < count; ++j) {
    double xi[6];
    bool centre = true;
    for (int a = 0; a < 6; ++a) {
      const int s = idx[a] - (opt->count[a] - 1) / 2;
      xi[a] = (double)s * opt->step[a];
      centre = centre && s == 0;
    }
    double *out = T_out + 16 * j;
    if (centre) {
      std::memcpy(out, T_centre, sizeof(double) * 16);  // the centre itself, bit for bit
    } else {
      double E[16];
      se3_matrix(se3_exp(xi), E);
      for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
          double s = 0.0;
          for (int i = 0; i < 4; ++i) s += E[i * 4 + r] * T_centre[c * 4 + i];
          out[c * 4 + r] = s;
        }
    }
    for (int a = 5; a >= 0; --a) {
      if (++idx[a] < opt->count[a]) break;
      idx[a] = 0;
    }
  }
  return DVO_AMD_OK;
}

}  // extern "C"
