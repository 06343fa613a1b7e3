// Device functions of the pose-graph optimizers (dvo_amd.h: dvo_amd_optimize_graph, dvo_amd_optimize_graphs_batch), fp64: the
// SE3 algebra, the edge error, the Cauchy kernel, the linearisation of one edge into its record and the pose update.  Shared by
// the kernels of dvo_graph.cpp (one big graph) and dvo_graph_batch.cpp (many small graphs, one workgroup each), so that both
// evaluate an edge with the same operations in the same order.
#ifndef DVO_AMD_GRAPH_DEVICE_H
#define DVO_AMD_GRAPH_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/dvo_amd.h"

namespace dvo_amd {
namespace graph {

constexpr int kRecord = 132;      // doubles per edge record (linearise_edge)

// edge record layout
constexpr int kE = 0, kChi2 = 6, kRho0 = 7, kRho1 = 8, kAff = 9, kAtt = 45, kAft = 81, kGf = 117, kGt = 123;

struct Pose {  // rotation row-major, translation
  double R[9], t[3];
};

__device__ __host__ inline Pose load_pose(const double *T) {  // column-major 4x4
  Pose p;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.R[r * 3 + c] = T[c * 4 + r];
    p.t[r] = T[12 + r];
  }
  return p;
}

__device__ inline Pose inverse(const Pose &a) {
  Pose o;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o.R[r * 3 + c] = a.R[c * 3 + r];
  for (int r = 0; r < 3; ++r) o.t[r] = -((o.R[r * 3 + 0] * a.t[0] + o.R[r * 3 + 1] * a.t[1]) + o.R[r * 3 + 2] * a.t[2]);
  return o;
}

__device__ inline Pose compose(const Pose &a, const Pose &b) {
  Pose o;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      o.R[r * 3 + c] = (a.R[r * 3 + 0] * b.R[0 * 3 + c] + a.R[r * 3 + 1] * b.R[1 * 3 + c]) + a.R[r * 3 + 2] * b.R[2 * 3 + c];
    o.t[r] = ((a.R[r * 3 + 0] * b.t[0] + a.R[r * 3 + 1] * b.t[1]) + a.R[r * 3 + 2] * b.t[2]) + a.t[r];
  }
  return o;
}

// Eigen's Quaternion(Matrix3) (Shepperd), normalised, sign with w >= 0: q = (w, x, y, z)
__device__ inline void quaternion(const double *m, double q[4]) {
  const double tr = (m[0] + m[4]) + m[8];
  double w, v[3];
  if (tr > 0.0) {
    double t = sqrt(tr + 1.0);
    w = 0.5 * t;
    t = 0.5 / t;
    v[0] = (m[7] - m[5]) * t;
    v[1] = (m[2] - m[6]) * t;
    v[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = sqrt(((m[i * 3 + i] - m[j * 3 + j]) - m[k * 3 + k]) + 1.0);
    v[i] = 0.5 * t;
    t = 0.5 / t;
    w = (m[k * 3 + j] - m[j * 3 + k]) * t;
    v[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
    v[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
  }
  const double nrm = sqrt(((w * w + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2]);
  double s = 1.0 / nrm;
  if (w < 0.0) s = -s;
  q[0] = w * s;
  q[1] = v[0] * s;
  q[2] = v[1] * s;
  q[3] = v[2] * s;
}

// inc(d): translation d[0..2], rotation of (sqrt(1 - |d[3..5]|^2), d[3..5]) (identity when 1 - |q|^2 < 0)
__device__ inline Pose increment(const double *d) {
  Pose p;
  const double x = d[3], y = d[4], z = d[5];
  const double w2 = 1.0 - ((x * x + y * y) + z * z);
  if (w2 < 0.0) {
    for (int i = 0; i < 9; ++i) p.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  } else {
    const double w = sqrt(w2);
    p.R[0] = 1.0 - 2.0 * (y * y + z * z);
    p.R[1] = 2.0 * (x * y - z * w);
    p.R[2] = 2.0 * (x * z + y * w);
    p.R[3] = 2.0 * (x * y + z * w);
    p.R[4] = 1.0 - 2.0 * (x * x + z * z);
    p.R[5] = 2.0 * (y * z - x * w);
    p.R[6] = 2.0 * (x * z - y * w);
    p.R[7] = 2.0 * (y * z + x * w);
    p.R[8] = 1.0 - 2.0 * (x * x + y * y);
  }
  p.t[0] = d[0];
  p.t[1] = d[1];
  p.t[2] = d[2];
  return p;
}

// Delta = Z^-1 * (X_from^-1 * X_to), e = (t, q_xyz), chi2 = e^T O e
struct EdgeEval {
  Pose Zi, D;
  double q[4], e[6], chi2;
};

__device__ inline void eval_edge(const dvo_amd_graph_edge &E, const double *poses, EdgeEval &v) {
  const Pose Xf = load_pose(poses + 16 * (size_t)E.from), Xt = load_pose(poses + 16 * (size_t)E.to);
  v.Zi = inverse(load_pose(E.measurement));
  v.D = compose(v.Zi, compose(inverse(Xf), Xt));
  quaternion(v.D.R, v.q);
  for (int i = 0; i < 3; ++i) {
    v.e[i] = v.D.t[i];
    v.e[3 + i] = v.q[1 + i];
  }
  double chi2 = 0.0;
  for (int i = 0; i < 6; ++i) {
    double oe = 0.0;
    for (int j = 0; j < 6; ++j) oe += E.information[j * 6 + i] * v.e[j];
    chi2 += v.e[i] * oe;
  }
  v.chi2 = chi2;
}

__device__ inline void robust(double chi2, double delta, double *rho0, double *rho1) {
  if (delta > 0.0) {
    const double dsqr = delta * delta;
    const double aux = (1.0 / dsqr) * chi2 + 1.0;
    *rho0 = dsqr * log(aux);
    *rho1 = 1.0 / aux;
  } else {
    *rho0 = chi2;
    *rho1 = 1.0;
  }
}
// one edge at the current estimate into its record o[kRecord]: error, chi2, the Cauchy weights, the three 6x6 products of the
// analytic Jacobians with rho1 Omega and the two gradient 6-vectors
__device__ inline void linearise_edge(const dvo_amd_graph_edge &E, const double *poses, double delta, double *o) {
  EdgeEval v;
  eval_edge(E, poses, v);
  double r0, r1;
  robust(v.chi2, delta, &r0, &r1);
  for (int i = 0; i < 6; ++i) o[kE + i] = v.e[i];
  o[kChi2] = v.chi2;
  o[kRho0] = r0;
  o[kRho1] = r1;

  // Jacobians, row-major 6x6 (rows t, q_xyz; columns translation, quaternion part of the increment)
  double Jf[36], Jt[36];
  const double w = v.q[0], qv[3] = {v.q[1], v.q[2], v.q[3]};
  const double *R = v.D.R, *t = v.D.t;
  const double *RzT = v.Zi.R;  // rotation of Z^-1 = Rz^T
  const Pose Z = load_pose(E.measurement);
  const double *tz = Z.t;
  for (int i = 0; i < 36; ++i) Jf[i] = Jt[i] = 0.0;
  // J_to = [R 0; 0 wI + [v]x]
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Jt[r * 6 + c] = R[r * 3 + c];
  const double vx[9] = {0.0, -qv[2], qv[1], qv[2], 0.0, -qv[0], -qv[1], qv[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Jt[(3 + r) * 6 + 3 + c] = (r == c ? w : 0.0) + vx[r * 3 + c];
  // J_from = [-Rz^T  2([t]x Rz^T + Rz^T [tz]x); 0  -(wI - [v]x) Rz^T]
  const double txm[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};
  const double tzm[9] = {0.0, -tz[2], tz[1], tz[2], 0.0, -tz[0], -tz[1], tz[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      Jf[r * 6 + c] = -RzT[r * 3 + c];
      double a = 0.0, b = 0.0, m = 0.0;
      for (int p = 0; p < 3; ++p) {
        a += txm[r * 3 + p] * RzT[p * 3 + c];
        b += RzT[r * 3 + p] * tzm[p * 3 + c];
        m += ((r == p ? w : 0.0) - vx[r * 3 + p]) * RzT[p * 3 + c];
      }
      Jf[r * 6 + 3 + c] = 2.0 * (a + b);
      Jf[(3 + r) * 6 + 3 + c] = -m;
    }
  // W = rho1 Omega (Omega column-major, symmetric); WJ = W J; products J_a^T W J_b; g = -J^T W e
  double W[36], We[6];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) W[r * 6 + c] = r1 * E.information[c * 6 + r];
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
    for (int c = 0; c < 6; ++c) s += W[r * 6 + c] * v.e[c];
    We[r] = s;
  }
  double WJ[36];
  for (int which = 0; which < 2; ++which) {
    const double *J = which ? Jt : Jf;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
        for (int p = 0; p < 6; ++p) s += W[r * 6 + p] * J[p * 6 + c];
        WJ[r * 6 + c] = s;
      }
    // which = 0: Aff = Jf^T W Jf; which = 1: Att = Jt^T W Jt and Aft = Jf^T W Jt
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
        for (int p = 0; p < 6; ++p) s += J[p * 6 + r] * WJ[p * 6 + c];
        o[(which ? kAtt : kAff) + r * 6 + c] = s;
        if (which) {
          double u = 0.0;
          for (int p = 0; p < 6; ++p) u += Jf[p * 6 + r] * WJ[p * 6 + c];
          o[kAft + r * 6 + c] = u;
        }
      }
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
      for (int p = 0; p < 6; ++p) s += J[p * 6 + r] * We[p];
      o[(which ? kGt : kGf) + r] = -s;
    }
  }
}

// X <- X * inc(d) on a column-major 4x4
__device__ inline void apply_increment(double *T, const double *d) {
  const Pose X = load_pose(T), D = increment(d);
  const Pose Y = compose(X, D);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = Y.R[r * 3 + c];
    T[12 + r] = Y.t[r];
  }
}

}  // namespace graph
}  // namespace dvo_amd
#endif
