// Host-only rules every launcher of libdvo_amd.so shares: the rows of a two-dimensional grid, and the float rows 0..2 that the
// kernels take of a column-major double transformation.  No HIP header: tests/launch_rules_main.cpp compiles this file alone.
#pragma once
#include <algorithm>

namespace dvo_amd {
namespace host {

// gridDim.y of a launch of `gx` columns of `block` threads over n records: a launch holds fewer than 2^31 threads and at most
// 65535 rows of blocks, and a block takes further records in steps of gridDim.y
inline unsigned grid_rows(long long n, unsigned gx, int block) {
  return (unsigned)std::max<long long>(1, std::min<long long>(std::min<long long>(n, 65535), (1ll << 31) / ((long long)gx * block)));
}

// rows 0..2 of a column-major transformation, row-major, cast to float; NULL: the identity
inline void rows_from_column_major(const double *T, float M[12]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) M[r * 4 + c] = T ? (float)T[c * 4 + r] : (r == c ? 1.0f : 0.0f);
}

// rows 0..2 of the rigid inverse of a column-major transformation, every product and sum rounded on its own in index order, then
// cast to float; NULL: the identity.  R[i][r] = T[r * 4 + i]: row r of R^T is column r of R.
inline void inverse_rows(const double *T, float M[12]) {
  if (!T) return rows_from_column_major(nullptr, M);
  const double t0 = T[12], t1 = T[13], t2 = T[14];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M[r * 4 + c] = (float)T[r * 4 + c];
    M[r * 4 + 3] = (float)(-((T[r * 4 + 0] * t0 + T[r * 4 + 1] * t1) + T[r * 4 + 2] * t2));
  }
}

// rows 0..2 of B^-1 * A in double, the inverse taken as rigid, every product and sum rounded on its own in index order, then cast
// to float (dvo_amd.h, covisibility rule 1).  Column-major poses: R[i][j] = P[j * 4 + i], t[i] = P[12 + i].
inline void relative_rows(const double *A, const double *B, float T[12]) {
  for (int r = 0; r < 3; ++r) {
    const double i0 = B[r * 4 + 0], i1 = B[r * 4 + 1], i2 = B[r * 4 + 2];  // row r of Rb^T
    const double ti = -((i0 * B[12] + i1 * B[13]) + i2 * B[14]);
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)((i0 * A[c * 4 + 0] + i1 * A[c * 4 + 1]) + i2 * A[c * 4 + 2]);
    T[r * 4 + 3] = (float)(((i0 * A[12] + i1 * A[13]) + i2 * A[14]) + ti);
  }
}

}  // namespace host
}  // namespace dvo_amd
