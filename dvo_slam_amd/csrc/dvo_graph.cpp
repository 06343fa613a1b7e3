// The pose-graph optimizer (dvo_amd.h: dvo_amd_optimize_graph), fp64 throughout:
//   k_linearise    one thread per edge: error, chi2, the Cauchy weights, both analytic Jacobians, the edge's three 6x6 products
//                  and two 6-vectors into an edge-indexed record (linearise_edge, dvo_graph_device.h)
//   k_objective    one thread per edge: chi2, rho0, rho1 at the current estimate (F = the fixed-shape sum of rho0)
//   k_assemble_H   one 64-lane group per 6x6 block of H (both mirror images are assembled, so H is stored full): 36 lanes own
//                  one entry each and sum its contributors in edge order from the host's CSR list
//   k_assemble_b   one thread per entry of b, contributors in edge order
//   k_damp_copy    working copy of H with lambda on the diagonal (H itself stays undamped)
//   k_potrf_panel  blocked right-looking Cholesky, 64 x 64 tiles: the diagonal tile in one workgroup (LDS); the first pivot
//                  <= 0 is written to one device word and every later kernel of the factorization and solve returns at once
//   k_trsm         the tiles below the diagonal tile: X L^T = A
//   k_syrk         the trailing update A_ij -= A_ik A_jk^T with v_mfma_f64_16x16x4_f64
//   k_trsv         forward and back substitution in one workgroup (the right-hand side in LDS)
//   k_matvec       y = H v, one wave per row, a fixed butterfly across the wave
//   k_dots         fixed-shape dot products (one workgroup each)
//   k_update       X <- X * inc(x) for every free vertex
// Every sum has one fixed order and there are no floating-point atomics: the result is bit-identical from run to run.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <optional>

#include "dvo_graph_device.h"
#include "dvo_graph_host.h"

namespace dvo_amd {
namespace graph {

constexpr int kTile = 64;         // Cholesky tile
constexpr int kLds = kTile + 1;   // LDS row stride of a tile (odd in doubles)
constexpr int kBlock = 256;
constexpr int kMaxN = 6 * DVO_AMD_GRAPH_MAX_FREE_VERTICES;
constexpr int kDotThreads = 256;
constexpr int kMaxDots = 8;

__global__ void k_objective(int n_edges, const dvo_amd_graph_edge *__restrict__ edges, const double *__restrict__ poses,
                            double delta, double *__restrict__ rho0, double *__restrict__ chi2, double *__restrict__ rho1) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_edges) return;
  EdgeEval v;
  eval_edge(edges[k], poses, v);
  double r0, r1;
  robust(v.chi2, delta, &r0, &r1);
  rho0[k] = r0;
  chi2[k] = v.chi2;
  rho1[k] = r1;
}

__global__ void __launch_bounds__(64) k_linearise(int n_edges, const dvo_amd_graph_edge *__restrict__ edges,
                                                  const double *__restrict__ poses, double delta, double *__restrict__ rec) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_edges) return;
  linearise_edge(edges[k], poses, delta, rec + (size_t)k * kRecord);
}

// contributor codes: edge * 4 + kind; kind 0 Aff, 1 Att, 2 Aft, 3 Aft^T
__global__ void __launch_bounds__(64) k_assemble_H(const int2 *__restrict__ block_rc, const int *__restrict__ ptr,
                                                   const int *__restrict__ contrib, const double *__restrict__ rec,
                                                   double *__restrict__ H, int N) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  if (lane >= 36) return;
  const int r = lane / 6, c = lane % 6;
  double s = 0.0;
  for (int p = ptr[blk]; p < ptr[blk + 1]; ++p) {
    const int code = contrib[p], kind = code & 3;
    const double *o = rec + (size_t)(code >> 2) * kRecord;
    const double v = kind == 0 ? o[kAff + r * 6 + c] : kind == 1 ? o[kAtt + r * 6 + c] : kind == 2 ? o[kAft + r * 6 + c]
                                                                                                   : o[kAft + c * 6 + r];
    s += v;
  }
  const int2 rc = block_rc[blk];
  H[(size_t)(6 * rc.x + r) * N + 6 * rc.y + c] = s;
}

// contributor codes: edge * 2 + (0 from, 1 to)
__global__ void k_assemble_b(int n, const int *__restrict__ ptr, const int *__restrict__ contrib,
                             const double *__restrict__ rec, double *__restrict__ b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int slot = i / 6, r = i % 6;
  double s = 0.0;
  for (int p = ptr[slot]; p < ptr[slot + 1]; ++p) {
    const int code = contrib[p];
    s += rec[(size_t)(code >> 1) * kRecord + ((code & 1) ? kGt : kGf) + r];
  }
  b[i] = s;
}

__global__ void k_pad_diag(double *H, int N, int n) {
  const int i = n + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) H[(size_t)i * N + i] = 1.0;
}

__global__ void k_damp_copy(const double *__restrict__ H, double *__restrict__ L, int N, int n, double lambda, int damp) {
  const size_t total = (size_t)N * N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    double v = H[i];
    const size_t r = i / N, c = i % N;
    if (damp && r == c && r < (size_t)n) v = v + lambda;
    L[i] = v;
  }
}

__global__ void k_max_diag(const double *__restrict__ H, int N, int n, double *out) {
  __shared__ double red[kBlock];
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) m = fmax(m, fabs(H[(size_t)i * N + i]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

// diagonal tile k: unblocked right-looking Cholesky in LDS
__global__ void __launch_bounds__(kBlock) k_potrf_panel(double *L, int N, int k, int *flag) {
  if (*(volatile int *)flag >= 0) return;
  __shared__ double A[kTile * kLds];
  __shared__ int bad;
  const int tid = threadIdx.x, base = k * kTile;
  for (int e = tid; e < kTile * kTile; e += kBlock) {
    const int r = e / kTile, c = e % kTile;
    A[r * kLds + c] = L[(size_t)(base + r) * N + base + c];
  }
  if (tid == 0) bad = -1;
  __syncthreads();
  for (int j = 0; j < kTile; ++j) {
    const double piv = A[j * kLds + j];
    if (!(piv > 0.0)) {  // uniform: every thread read the same LDS word
      if (tid == 0) *flag = base + j;
      return;
    }
    const double d = sqrt(piv);
    __syncthreads();  // everyone has read the pivot before it is overwritten
    if (tid == 0) A[j * kLds + j] = d;
    if (tid > j && tid < kTile) A[tid * kLds + j] = A[tid * kLds + j] / d;
    __syncthreads();
    const int rem = kTile - 1 - j;
    for (int e = tid; e < rem * rem; e += kBlock) {
      const int r = j + 1 + e / rem, c = j + 1 + e % rem;
      if (c <= r) A[r * kLds + c] = A[r * kLds + c] - A[r * kLds + j] * A[c * kLds + j];
    }
    __syncthreads();
  }
  (void)bad;
  for (int e = tid; e < kTile * kTile; e += kBlock) {
    const int r = e / kTile, c = e % kTile;
    if (c <= r) L[(size_t)(base + r) * N + base + c] = A[r * kLds + c];
  }
}

// tiles (i, k), i > k: X L_kk^T = A_ik
__global__ void __launch_bounds__(kBlock) k_trsm(double *L, int N, int k, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double D[kTile * kLds];
  __shared__ double A[kTile * kLds];
  const int tid = threadIdx.x, kb = k * kTile, ib = (k + 1 + blockIdx.x) * kTile;
  for (int e = tid; e < kTile * kTile; e += kBlock) {
    const int r = e / kTile, c = e % kTile;
    D[r * kLds + c] = L[(size_t)(kb + r) * N + kb + c];
    A[r * kLds + c] = L[(size_t)(ib + r) * N + kb + c];
  }
  __syncthreads();
  for (int j = 0; j < kTile; ++j) {
    if (tid < kTile) A[tid * kLds + j] = A[tid * kLds + j] / D[j * kLds + j];
    __syncthreads();
    const int rem = kTile - 1 - j;
    for (int e = tid; e < kTile * rem; e += kBlock) {
      const int r = e / rem, c = j + 1 + e % rem;
      A[r * kLds + c] = A[r * kLds + c] - A[r * kLds + j] * D[c * kLds + j];
    }
    __syncthreads();
  }
  for (int e = tid; e < kTile * kTile; e += kBlock) {
    const int r = e / kTile, c = e % kTile;
    L[(size_t)(ib + r) * N + kb + c] = A[r * kLds + c];
  }
}

typedef double double4_t __attribute__((ext_vector_type(4)));

// tiles (i, j), k < j <= i: A_ij -= A_ik A_jk^T.  4 waves, each a 32 x 32 quarter = 2 x 2 MFMA 16x16 tiles; K in two halves.
// v_mfma_f64_16x16x4_f64: lane l gives A[row l&15][k l>>4] and B[k l>>4][col l&15]; D[row (l>>4) + 4 reg][col l&15].
__global__ void __launch_bounds__(kBlock) k_syrk(double *L, int N, int k, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  const int j = k + 1 + blockIdx.x, i = k + 1 + blockIdx.y;
  if (j > i) return;
  constexpr int kHalf = kTile / 2, kS = kHalf + 1;
  __shared__ double Ai[kTile * kS];
  __shared__ double Aj[kTile * kS];
  const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int kb = k * kTile, ib = i * kTile, jb = j * kTile;
  const int r0 = 32 * (wave >> 1), c0 = 32 * (wave & 1);
  double4_t acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
    for (int e = tid; e < kTile * kHalf; e += kBlock) {
      const int r = e / kHalf, c = e % kHalf;
      Ai[r * kS + c] = L[(size_t)(ib + r) * N + kb + h * kHalf + c];
      Aj[r * kS + c] = L[(size_t)(jb + r) * N + kb + h * kHalf + c];
    }
    __syncthreads();
    for (int kk = 0; kk < kHalf; kk += 4) {
      const int kl = kk + (lane >> 4);
      for (int a = 0; a < 2; ++a) {
        const double av = Ai[(r0 + 16 * a + (lane & 15)) * kS + kl];
        for (int b = 0; b < 2; ++b) {
          const double bv = Aj[(c0 + 16 * b + (lane & 15)) * kS + kl];
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[a][b], 0, 0, 0);
        }
      }
    }
  }
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int reg = 0; reg < 4; ++reg) {
        const int r = r0 + 16 * a + (lane >> 4) + 4 * reg, c = c0 + 16 * b + (lane & 15);
        double *p = L + (size_t)(ib + r) * N + jb + c;
        *p = *p - acc[a][b][reg];
      }
}

// L y = b, L^T x = y in one workgroup; x may alias nothing else.  The right-hand side lives in LDS.
constexpr int kSolveThreads = 1024;
__global__ void __launch_bounds__(kSolveThreads) k_trsv(const double *__restrict__ L, int N, const double *__restrict__ b,
                                                        double *__restrict__ x, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double r[kMaxN + kTile];
  const int tid = threadIdx.x, lane = tid % 64, T = N / kTile;
  for (int i = tid; i < N; i += kSolveThreads) r[i] = b[i];
  __syncthreads();
  for (int k = 0; k < T; ++k) {  // forward
    const int kb = k * kTile;
    if (tid < 64) {
      double ri = r[kb + lane];
      for (int j = 0; j < kTile; ++j) {
        if (lane == j) ri = ri / L[(size_t)(kb + j) * N + kb + j];
        const double yj = __shfl(ri, j);
        if (lane > j) ri = ri - L[(size_t)(kb + lane) * N + kb + j] * yj;
      }
      r[kb + lane] = ri;
    }
    __syncthreads();
    for (int i = kb + kTile + tid; i < N; i += kSolveThreads) {
      double s = r[i];
      const double *row = L + (size_t)i * N + kb;
      for (int p = 0; p < kTile; ++p) s = s - row[p] * r[kb + p];
      r[i] = s;
    }
    __syncthreads();
  }
  for (int k = T - 1; k >= 0; --k) {  // backward
    const int kb = k * kTile;
    if (tid < 64) {
      double ri = r[kb + lane];
      for (int j = kTile - 1; j >= 0; --j) {
        if (lane == j) ri = ri / L[(size_t)(kb + j) * N + kb + j];
        const double yj = __shfl(ri, j);
        if (lane < j) ri = ri - L[(size_t)(kb + j) * N + kb + lane] * yj;
      }
      r[kb + lane] = ri;
    }
    __syncthreads();
    for (int i = tid; i < kb; i += kSolveThreads) {
      double s = r[i];
      for (int p = 0; p < kTile; ++p) s = s - L[(size_t)(kb + p) * N + i] * r[kb + p];
      r[i] = s;
    }
    __syncthreads();
  }
  for (int i = tid; i < N; i += kSolveThreads) x[i] = r[i];
}

// y = H v over the n real rows (H stored full); one wave per row, lanes stride the columns, then a fixed butterfly
__global__ void __launch_bounds__(kBlock) k_matvec(const double *__restrict__ H, int N, int n, const double *__restrict__ v,
                                                   double *__restrict__ y) {
  const int row = blockIdx.x * (kBlock / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (row >= n) return;
  const double *h = H + (size_t)row * N;
  double s = 0.0;
  for (int c = lane; c < n; c += 64) s += h[c] * v[c];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) y[row] = s;
}

struct DotArgs {
  const double *a[kMaxDots], *b[kMaxDots];  // b null: sum of a; b == a: squared norm
  double lambda[kMaxDots];                  // mode 1 entries: sum a (lambda a + b)
  int mode[kMaxDots];
  int n[kMaxDots];
};

__global__ void __launch_bounds__(kDotThreads) k_dots(DotArgs args, double *out) {
  __shared__ double red[kDotThreads];
  const int d = blockIdx.x, tid = threadIdx.x, n = args.n[d];
  const double *a = args.a[d], *b = args.b[d];
  double s = 0.0;
  for (int i = tid; i < n; i += kDotThreads) {
    if (args.mode[d] == 1)
      s += a[i] * (args.lambda[d] * a[i] + b[i]);
    else
      s += b ? a[i] * b[i] : a[i];
  }
  red[tid] = s;
  __syncthreads();
  for (int h = kDotThreads / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] = red[tid] + red[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[d] = red[0];
}

// out = alpha x (mode 0), x + beta (y - x) (mode 1), x - y (mode 2)
__global__ void k_vec(int n, int mode, double alpha, const double *__restrict__ x, const double *__restrict__ y,
                      double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = mode == 0 ? alpha * x[i] : mode == 1 ? x[i] + alpha * (y[i] - x[i]) : x[i] - y[i];
}

// X <- X * inc(x) for every free vertex (skipped when the solve behind x failed)
__global__ void k_update(int m, const int *__restrict__ vertex_of, const double *__restrict__ x, double *__restrict__ poses,
                         const int *flag) {
  if (flag && *(volatile const int *)flag >= 0) return;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m) return;
  double *T = poses + 16 * (size_t)vertex_of[s];
  const Pose X = load_pose(T), D = increment(x + 6 * s);
  const Pose Y = compose(X, D);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = Y.R[r * 3 + c];
    T[12 + r] = Y.t[r];
  }
}

inline int grid_for(size_t n, int block) { return (int)std::max<size_t>(1, (n + block - 1) / block); }

// ---- the sparse solver (DVO_AMD_GRAPH_SOLVER_SPARSE): multifrontal Cholesky over the nested-dissection assembly tree -------
//   H is stored as its nonzero 6x6 blocks (row-major 36 doubles each, both mirror images), sorted by (row, col) slot: the same
//   contributor lists and k_assemble_H as the dense path, pointed at block k with block_rc = (k, 0) and N = 6.
//   A front is dense, row-major, lower triangle used: local blocks are its pivots (p, in elimination order) then its update set
//   (u, in elimination order).  Pivot block i sits at scalar 6i, update block j at ppad + 6j.  Small fronts have ppad = 6p and
//   ld = 6(p + u); wide fronts pad ppad and ld to kTile (pad pivots are the identity) and go through the dense path's
//   k_potrf_panel / k_trsm / k_syrk with the front as the matrix, over the pivot tiles only.  After the factorization the
//   trailing ld - ppad rows and columns of a front hold its update matrix C - L21 L21^T, which the parent gathers.
//   Per level (leaves first): k_front_assemble (H blocks + lambda + the children's update matrices, children in a fixed order),
//   then k_front_factor (one workgroup per small front) and the tiled kernels per wide front.  Forward substitution bottom-up
//   (each front's update vector sits behind its pivots in its vector slot), backward top-down (a gather of the ancestors'
//   solved entries).  Dependencies between fronts are kernel boundaries; the failure word stops every later kernel.
constexpr int kFrontThreads = 256;
constexpr int kSmallMaxLd = 1024;   // a small front's column lives in LDS
constexpr int kWidePivots = 192;    // 6p above this (32 vertices): the tiled path

struct Front {
  long long a_off, hmap_off;  // front matrix (ld x ld doubles); (p + u) x p H-block indices (-1: none)
  int v_off, ld, p, u, ppad;  // vector slot (ld doubles)
  int loc_off;                // slots of the p + u local blocks
  int inv_off;                // this front as a child: parent-local block -> index in this front's update set, or -1
  int ch_begin, ch_end;       // children (front ids) in child_list
};

// scalar index i of a front -> local block (or -1 for padding) and the entry within it
__device__ inline int local_block(const Front &F, int i, int *w) {
  *w = i % 6;
  if (i < 6 * F.p) return i / 6;
  if (i >= F.ppad && i < F.ppad + 6 * F.u) {
    *w = (i - F.ppad) % 6;
    return F.p + (i - F.ppad) / 6;
  }
  return -1;
}

// the lower triangle of each front of the level: H blocks + lambda on the diagonal, then the children's update matrices in order
__global__ void __launch_bounds__(kBlock) k_front_assemble(const Front *__restrict__ fronts, const int *__restrict__ ids,
                                                           const double *__restrict__ Hs, const int *__restrict__ hmap,
                                                           const int *__restrict__ inv, const int *__restrict__ child_list,
                                                           double *__restrict__ A, double lambda, int damp, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  const Front F = fronts[ids[blockIdx.y]];
  const long long total = (long long)F.ld * F.ld;
  double *a = A + F.a_off;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(e / F.ld), c = (int)(e % F.ld);
    if (c > r) continue;
    int wr, wc;
    const int br = local_block(F, r, &wr), bc = local_block(F, c, &wc);
    double v = 0.0;
    if (br < 0 || bc < 0) {
      v = (r == c && r < F.ppad) ? 1.0 : 0.0;  // pad pivots: the identity
    } else {
      if (bc < F.p) {
        const int hb = hmap[F.hmap_off + (long long)br * F.p + bc];
        if (hb >= 0) v = Hs[36 * (size_t)hb + 6 * wr + wc];
        if (damp && r == c) v = v + lambda;
      }
      for (int q = F.ch_begin; q < F.ch_end; ++q) {
        const Front C = fronts[child_list[q]];
        const int jr = inv[C.inv_off + br], jc = inv[C.inv_off + bc];
        if (jr >= 0 && jc >= 0)
          v = v + A[C.a_off + (long long)(C.ppad + 6 * jr + wr) * C.ld + C.ppad + 6 * jc + wc];
      }
    }
    a[(long long)r * F.ld + c] = v;
  }
}

// partial Cholesky of a small front (its first 6p columns) in one workgroup, right-looking, one vertex (6 columns) at a time:
// the panel's columns are factorized one by one (each kept in LDS), then the lower triangle behind the panel gets the rank-6
// update in one pass, one wave per row.  Every entry subtracts the six products in column order, as six rank-1 steps would.
__global__ void __launch_bounds__(kFrontThreads) k_front_factor(const Front *__restrict__ fronts, const int *__restrict__ ids,
                                                                double *__restrict__ A, int *flag) {
  if (*(volatile int *)flag >= 0) return;
  __shared__ double col[6][kSmallMaxLd];
  const Front F = fronts[ids[blockIdx.x]];
  double *a = A + F.a_off;
  const int ld = F.ld, np = 6 * F.p, tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  for (int j0 = 0; j0 < np; j0 += 6) {
    for (int q = 0; q < 6; ++q) {
      const int j = j0 + q;
      const double piv = a[(long long)j * ld + j];
      if (!(piv > 0.0)) {  // uniform: every thread read the same word after the last barrier
        if (tid == 0) atomicMax(flag, j);
        return;
      }
      const double d = sqrt(piv);
      for (int i = j + 1 + tid; i < ld; i += kFrontThreads) {
        const double v = a[(long long)i * ld + j] / d;
        a[(long long)i * ld + j] = v;
        col[q][i] = v;
      }
      __syncthreads();  // everyone has read the pivot, and the column is in LDS
      if (tid == 0) a[(long long)j * ld + j] = d;
      const int w = 5 - q;  // the panel's columns behind j
      if (w > 0) {
        for (int e = tid; e < (ld - j - 1) * w; e += kFrontThreads) {
          const int r = j + 1 + e / w, c = j + 1 + e % w;
          if (c <= r) a[(long long)r * ld + c] = a[(long long)r * ld + c] - col[q][r] * col[q][c];
        }
        __syncthreads();
      }
    }
    const int j1 = j0 + 6;
    for (int r = j1 + wave; r < ld; r += kFrontThreads / 64) {
      double lr[6];
      for (int q = 0; q < 6; ++q) lr[q] = col[q][r];
      double *row = a + (long long)r * ld;
      for (int c = j1 + lane; c <= r; c += 64) {
        double v = row[c];
        for (int q = 0; q < 6; ++q) v = v - lr[q] * col[q][c];
        row[c] = v;
      }
    }
    __syncthreads();
  }
}

// forward substitution of the level's fronts: the right-hand side (b on the pivots, the children's update vectors added in
// order), L11 y = r1 in place, then r2 -= L21 y: the front's update vector
__global__ void __launch_bounds__(kFrontThreads) k_front_forward(const Front *__restrict__ fronts, const int *__restrict__ ids,
                                                                 const double *__restrict__ A, const int *__restrict__ loc,
                                                                 const int *__restrict__ inv,
                                                                 const int *__restrict__ child_list,
                                                                 const double *__restrict__ b, double *__restrict__ V,
                                                                 const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  const Front F = fronts[ids[blockIdx.x]];
  const double *a = A + F.a_off;
  double *r = V + F.v_off;
  const int ld = F.ld, np = 6 * F.p, nu = 6 * F.u, tid = threadIdx.x;
  for (int i = tid; i < ld; i += kFrontThreads) {
    int w;
    const int blk = local_block(F, i, &w);
    double v = 0.0;
    if (blk >= 0) {
      if (blk < F.p) v = b[6 * (size_t)loc[F.loc_off + blk] + w];
      for (int q = F.ch_begin; q < F.ch_end; ++q) {
        const Front C = fronts[child_list[q]];
        const int j = inv[C.inv_off + blk];
        if (j >= 0) v = v + V[C.v_off + C.ppad + 6 * j + w];
      }
    }
    r[i] = v;
  }
  __syncthreads();
  for (int j = 0; j < np; ++j) {
    const double y = r[j] / a[(long long)j * ld + j];
    __syncthreads();
    if (tid == 0) r[j] = y;
    const int below = np - j - 1;
    for (int t = tid; t < below + nu; t += kFrontThreads) {
      const int i = t < below ? j + 1 + t : F.ppad + (t - below);
      r[i] = r[i] - a[(long long)i * ld + j] * y;
    }
    __syncthreads();
  }
}

// backward substitution of the level's fronts: z = y - L21^T x2 (x2 = the ancestors' solved entries), L11^T x1 = z
__global__ void __launch_bounds__(kFrontThreads) k_front_backward(const Front *__restrict__ fronts, const int *__restrict__ ids,
                                                                  const double *__restrict__ A, const int *__restrict__ loc,
                                                                  double *__restrict__ V, double *__restrict__ x,
                                                                  const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  const Front F = fronts[ids[blockIdx.x]];
  const double *a = A + F.a_off;
  double *r = V + F.v_off;
  const int ld = F.ld, np = 6 * F.p, nu = 6 * F.u, tid = threadIdx.x;
  for (int j = tid; j < np; j += kFrontThreads) {
    double s = r[j];
    for (int t = 0; t < nu; ++t)
      s = s - a[(long long)(F.ppad + t) * ld + j] * x[6 * (size_t)loc[F.loc_off + F.p + t / 6] + t % 6];
    r[j] = s;
  }
  __syncthreads();
  for (int j = np - 1; j >= 0; --j) {
    const double xj = r[j] / a[(long long)j * ld + j];
    __syncthreads();
    if (tid == 0) r[j] = xj;
    for (int i = tid; i < j; i += kFrontThreads) r[i] = r[i] - a[(long long)j * ld + i] * xj;
    __syncthreads();
  }
  for (int i = tid; i < np; i += kFrontThreads) x[6 * (size_t)loc[F.loc_off + i / 6] + i % 6] = r[i];
}

// y = H v over the stored blocks: one thread per row, blocks of the block row in column order, entries in column order
__global__ void k_bsr_matvec(int n, const int *__restrict__ row_ptr, const int2 *__restrict__ rc,
                             const double *__restrict__ Hs, const double *__restrict__ v, double *__restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = i / 6, w = i % 6;
  double acc = 0.0;
  for (int k = row_ptr[s]; k < row_ptr[s + 1]; ++k) {
    const double *h = Hs + 36 * (size_t)k + 6 * w;
    const double *x = v + 6 * (size_t)rc[k].y;
    for (int c = 0; c < 6; ++c) acc += h[c] * x[c];
  }
  y[i] = acc;
}

// max |diag(H)| over the diagonal blocks (fmax is exact: any order gives the same value)
__global__ void k_max_diag_blocks(int n, const int *__restrict__ diag_block, const double *__restrict__ Hs, double *out) {
  __shared__ double red[kBlock];
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) m = fmax(m, fabs(Hs[36 * (size_t)diag_block[i / 6] + 7 * (i % 6)]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

// ---- marginal covariances (dvo_amd_graph_marginals): entries of Z = H^-1 by selected inversion -----------------------------
//   With H = L L^T, Z L = L^-T gives, for a pivot (block) column t and the rows R behind it, Z_Rt = -Z_RR Y and
//   Z_tt = L_tt^-T L_tt^-1 - Y^T Z_Rt with Y = L_Rt L_tt^-1: column t needs only entries of Z inside the column's own row
//   structure, so the recurrence runs front by front down the assembly tree (root first).  A front's Z lives in a second arena
//   with the factor's layout; its trailing part (Z22, the inverse over the update set) is a gather from the parent's finished Z.
//   Small fronts: one workgroup, one scalar column at a time, Z kept full (both mirror images are the same bits).  Wide fronts
//   and the dense solver (one front holding everything, so Z is the whole inverse): 64 x 64 tiles, lower triangle only, with
//   v_mfma_f64_16x16x4_f64; every reader takes entry (max, min), which is what makes Z exactly symmetric.
constexpr int kSelThreads = 512;
enum { kLoadPlain = 0, kLoadTrans = 1, kLoadSym = 2 };  // kLoadSym: a diagonal tile of which the lower triangle is stored

struct SelInfo {
  long long parent_a_off;  // the parent's front (-1: a root)
  int parent_ld, up_off;   // up[up_off + j]: the parent's scalar index of update block j
};

struct MargReq {
  long long base;  // the front's offset in Z
  int ld, r0, c0, out;
};

struct ColReq {
  int row, out, transposed;  // the other vertex's first unknown, the output block, 1: the solved vertex is the block's row
};

__device__ inline double tile_at(const double *X, int ld, int mode, int r, int k) {
  if (mode == kLoadTrans || (mode == kLoadSym && k > r)) return X[(size_t)k * ld + r];
  return X[(size_t)r * ld + k];
}

// acc[r][c] += sum over k of X(r, k) Y(c, k) for two 64 x 64 tiles, K in two halves through LDS, k ascending; the waves'
// quarters and the MFMA operand layout are k_syrk's
__device__ inline void tile_mac(double4_t (&acc)[2][2], const double *X, int ldx, int xm, const double *Y, int ldy, int ym,
                                double *Xs, double *Ys) {
  constexpr int kHalf = kTile / 2, kS = kHalf + 1;
  const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int r0 = 32 * (wave >> 1), c0 = 32 * (wave & 1);
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
    for (int e = tid; e < kTile * kHalf; e += kBlock) {
      int r = e / kHalf, c = e % kHalf;
      if (xm == kLoadTrans) c = e / kTile, r = e % kTile;  // along the stored rows
      Xs[r * kS + c] = tile_at(X, ldx, xm, r, h * kHalf + c);
      r = e / kHalf, c = e % kHalf;
      if (ym == kLoadTrans) c = e / kTile, r = e % kTile;
      Ys[r * kS + c] = tile_at(Y, ldy, ym, r, h * kHalf + c);
    }
    __syncthreads();
    for (int kk = 0; kk < kHalf; kk += 4) {
      const int kl = kk + (lane >> 4);
      for (int a = 0; a < 2; ++a) {
        const double av = Xs[(r0 + 16 * a + (lane & 15)) * kS + kl];
        for (int b = 0; b < 2; ++b) {
          const double bv = Ys[(c0 + 16 * b + (lane & 15)) * kS + kl];
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[a][b], 0, 0, 0);
        }
      }
    }
  }
}

// f(row, column, value) for the entries of the tile this lane holds (k_syrk's layout of the accumulators)
template <class F>
__device__ inline void tile_each(const double4_t (&acc)[2][2], F f) {
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int g = 0; g < 4; ++g)
        f(32 * (wave >> 1) + 16 * a + (lane >> 4) + 4 * g, 32 * (wave & 1) + 16 * b + (lane & 15), acc[a][b][g]);
}

// W = L_tt^-1 (lower triangular, the upper triangle written as zeros): one thread per column, forward substitution in LDS.
// Column c of W is thread c's own: it keeps W[r][c], r > c, in the tile's unused upper triangle at [c][r].
__global__ void __launch_bounds__(kBlock) k_tile_inverse(const double *__restrict__ L, int ld, int t, double *__restrict__ Wt,
                                                         const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double A[kTile * kLds];
  const int tid = threadIdx.x, base = t * kTile;
  for (int e = tid; e < kTile * kTile; e += kBlock) {
    const int r = e / kTile, c = e % kTile;
    if (c <= r) A[r * kLds + c] = L[(size_t)(base + r) * ld + base + c];
  }
  __syncthreads();
  if (tid < kTile) {
    const int c = tid;
    const double wcc = 1.0 / A[c * kLds + c];
    for (int r = c + 1; r < kTile; ++r) {
      double s = A[r * kLds + c] * wcc;
      for (int k = c + 1; k < r; ++k) s += A[r * kLds + k] * A[c * kLds + k];
      A[c * kLds + r] = -(s / A[r * kLds + r]);
    }
  }
  __syncthreads();
  for (int e = tid; e < kTile * kTile; e += kBlock) {
    const int r = e / kTile, c = e % kTile;
    Wt[e] = r > c ? A[c * kLds + r] : r == c ? 1.0 / A[r * kLds + r] : 0.0;
  }
}

// Y_i = L_it W for the tile rows i behind t (Y: consecutive 64 x 64 tiles, row-major)
__global__ void __launch_bounds__(kBlock) k_tile_y(const double *__restrict__ L, int ld, int t, const double *__restrict__ Wt,
                                                   double *__restrict__ Y, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double Xs[kTile * (kTile / 2 + 1)];
  __shared__ double Ys[kTile * (kTile / 2 + 1)];
  const int i = t + 1 + blockIdx.x;
  double4_t acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
  tile_mac(acc, L + (size_t)i * kTile * ld + (size_t)t * kTile, ld, kLoadPlain, Wt, kTile, kLoadTrans, Xs, Ys);
  double *y = Y + (size_t)blockIdx.x * kTile * kTile;
  tile_each(acc, [&](int r, int c, double v) { y[r * kTile + c] = v; });
}

// Z_it = -sum over the tile rows k behind t (ascending) of Z_ik Y_k, Z_ik read from the stored lower triangle
__global__ void __launch_bounds__(kBlock) k_tile_zcol(double *Z, int ld, int t, int T, const double *__restrict__ Y,
                                                      const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double Xs[kTile * (kTile / 2 + 1)];
  __shared__ double Ys[kTile * (kTile / 2 + 1)];
  const int i = t + 1 + blockIdx.x;
  double4_t acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int k = t + 1; k < T; ++k) {
    const double *z = k <= i ? Z + (size_t)i * kTile * ld + (size_t)k * kTile : Z + (size_t)k * kTile * ld + (size_t)i * kTile;
    tile_mac(acc, z, ld, k < i ? kLoadPlain : k == i ? kLoadSym : kLoadTrans, Y + (size_t)(k - t - 1) * kTile * kTile, kTile,
             kLoadTrans, Xs, Ys);
  }
  double *out = Z + (size_t)i * kTile * ld + (size_t)t * kTile;
  tile_each(acc, [&](int r, int c, double v) { out[(size_t)r * ld + c] = -v; });
}

// Z_tt = W^T W - sum over k (ascending) of Z_kt^T Y_k; the lower triangle is stored
__global__ void __launch_bounds__(kBlock) k_tile_zdiag(double *Z, int ld, int t, int T, const double *__restrict__ Wt,
                                                       const double *__restrict__ Y, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double Xs[kTile * (kTile / 2 + 1)];
  __shared__ double Ys[kTile * (kTile / 2 + 1)];
  double4_t ww[2][2], zy[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) ww[a][b] = zy[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
  tile_mac(ww, Wt, kTile, kLoadTrans, Wt, kTile, kLoadTrans, Xs, Ys);
  for (int k = t + 1; k < T; ++k)
    tile_mac(zy, Z + (size_t)k * kTile * ld + (size_t)t * kTile, ld, kLoadTrans, Y + (size_t)(k - t - 1) * kTile * kTile, kTile,
             kLoadTrans, Xs, Ys);
  double *out = Z + (size_t)t * kTile * ld + (size_t)t * kTile;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) ww[a][b] = ww[a][b] - zy[a][b];
  tile_each(ww, [&](int r, int c, double v) {
    if (c <= r) out[(size_t)r * ld + c] = v;
  });
}

// the trailing part of each front of the level: Z over its update set, from the parent's Z (padding: zeros)
__global__ void __launch_bounds__(kBlock) k_front_gather_z22(const Front *__restrict__ fronts, const int *__restrict__ ids,
                                                             const SelInfo *__restrict__ info, const int *__restrict__ up,
                                                             double *Z, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  const int id = ids[blockIdx.y];
  const Front F = fronts[id];
  const SelInfo I = info[id];
  const int w = F.ld - F.ppad;
  const long long total = (long long)w * w;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(e / w), c = (int)(e % w);
    double v = 0.0;
    if (r < 6 * F.u && c < 6 * F.u && I.parent_a_off >= 0) {
      const int pr = up[I.up_off + r / 6] + r % 6, pc = up[I.up_off + c / 6] + c % 6;
      v = Z[I.parent_a_off + (long long)max(pr, pc) * I.parent_ld + min(pr, pc)];
    }
    Z[F.a_off + (long long)(F.ppad + r) * F.ld + F.ppad + c] = v;
  }
}

// a small front in one workgroup, pivot columns last to first: z_Rj = -(Z_RR l_Rj) / l_jj (one wave per row, a fixed butterfly),
// z_jj = (1 / l_jj - l_Rj . z_Rj) / l_jj; both mirror images of the column are written
__global__ void __launch_bounds__(kSelThreads) k_front_selinv(const Front *__restrict__ fronts, const int *__restrict__ ids,
                                                              const double *__restrict__ A, double *Z, const int *flag) {
  if (*(volatile const int *)flag >= 0) return;
  __shared__ double col[kSmallMaxLd];
  __shared__ double zc[kSmallMaxLd];
  const Front F = fronts[ids[blockIdx.x]];
  const double *a = A + F.a_off;
  double *z = Z + F.a_off;
  const int ld = F.ld, np = 6 * F.p, tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  for (int j = np - 1; j >= 0; --j) {
    const double d = a[(long long)j * ld + j];
    for (int i = j + 1 + tid; i < ld; i += kSelThreads) col[i] = a[(long long)i * ld + j];
    __syncthreads();
    for (int i = j + 1 + wave; i < ld; i += kSelThreads / 64) {
      const double *zr = z + (long long)i * ld;
      double s = 0.0;
      for (int k = j + 1 + lane; k < ld; k += 64) s += zr[k] * col[k];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) zc[i] = -(s / d);
    }
    __syncthreads();
    if (wave == 0) {
      double s = 0.0;
      for (int k = j + 1 + lane; k < ld; k += 64) s += zc[k] * col[k];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) z[(long long)j * ld + j] = (1.0 / d - s) / d;
    }
    for (int i = j + 1 + tid; i < ld; i += kSelThreads) {
      z[(long long)i * ld + j] = zc[i];
      z[(long long)j * ld + i] = zc[i];
    }
    __syncthreads();
  }
}

// requested blocks whose two vertices meet in one front (the dense solver: always), column-major, from entry (max, min)
__global__ void k_marg_gather(int n, const MargReq *__restrict__ req, const double *__restrict__ Z, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 36 * n) return;
  const MargReq q = req[i / 36];
  const int e = i % 36, r = q.r0 + e % 6, c = q.c0 + e / 6;
  out[36 * (size_t)q.out + e] = Z[q.base + (long long)max(r, c) * q.ld + min(r, c)];
}

// requested blocks read from the six solved columns of one vertex (cols: 6 x n)
__global__ void k_marg_columns(int n_req, const ColReq *__restrict__ req, const double *__restrict__ cols, int n,
                               double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 36 * n_req) return;
  const ColReq q = req[i / 36];
  const int e = i % 36, r = e % 6, c = e / 6;
  out[36 * (size_t)q.out + e] = q.transposed ? cols[(size_t)r * n + q.row + c] : cols[(size_t)c * n + q.row + r];
}

__global__ void k_unit_vector(double *b, int n, int at) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = i == at ? 1.0 : 0.0;
}

}  // namespace graph

namespace host {

// Every device buffer of the workspace is named once, in one of three lists: the sparse memory check estimates the "held" ones
// and adds what the context already holds of them to the free memory; the plain list's O(m + edges) buffers it leaves out.
#define GRAPH_BUFS_PLAIN(X)                                                                                                  \
  X(poses) X(saved) X(edges) X(rec) X(rho0) X(chi2) X(rho1) X(H) X(L) X(b) X(x) X(hsd) X(hdl) X(aux) X(block_rc)             \
  X(block_ptr) X(block_c) X(b_ptr) X(b_c) X(vertex_of) X(scalars) X(flag)                                                    \
  /* sparse: row pointers and (row, col) slots of the H blocks, the diagonal block of each slot, the level lists */          \
  X(bsr_ptr) X(bsr_rc) X(diag_block) X(child_list) X(level_ids) X(small_ids)                                                 \
  /* marginals: parents and child -> parent maps, a tile column of Y, a tile's inverse, requests, six columns, the output */ \
  X(sel_info) X(up) X(ytiles) X(wtile) X(mreq) X(creq) X(cols) X(mout)
// the sparse solver: the front matrices and vectors, the H blocks, the fronts' maps and records
#define GRAPH_BUFS_HELD_SPARSE(X) X(A) X(V) X(Hs) X(hmap) X(inv) X(loc) X(fronts)
// marginals: the fronts' Z (the factor's layout)
#define GRAPH_BUFS_HELD_INVERSE(X) X(Zinv)

#define GRAPH_BUFS(X) GRAPH_BUFS_PLAIN(X) GRAPH_BUFS_HELD_SPARSE(X) GRAPH_BUFS_HELD_INVERSE(X)
#define HELD_BYTES(name) held += (double)name.bytes;

struct GraphWorkspace {
  DEVICE_BUF_MEMBERS(GRAPH_BUFS)
  // the bytes held of the buffers the sparse memory check estimates (with_inverse: the marginals' arena too)
  double held_bytes(bool with_inverse) const {
    double held = 0.0;
    GRAPH_BUFS_HELD_SPARSE(HELD_BYTES)
    if (with_inverse) { GRAPH_BUFS_HELD_INVERSE(HELD_BYTES) }
    return held;
  }
  hipEvent_t ev[6] = {};
  double lin_ms = 0.0, fac_ms = 0.0;
  int n_padded = 0, factorizations = 0;
  // the last sparse call
  double sp_symbolic_ms = 0.0, sp_lin_ms = 0.0, sp_fac_ms = 0.0, sp_solve_ms = 0.0, sp_factor_doubles = 0.0, sp_flops = 0.0;
  int sp_fronts = 0, sp_levels = 0, sp_widest = 0;
};

namespace {

int grow(DeviceBuf &b, size_t bytes) { return grow(b, bytes, kGraphBufStep, "graph workspace"); }

int workspace(dvo_amd_context *ctx, GraphWorkspace **out) {
  if (!ctx->graph_ws) {
    GraphWorkspace *w = new GraphWorkspace();
    ctx->graph_ws = w;
    for (hipEvent_t &e : w->ev) HIP_TRY(hipEventCreate(&e));
  }
  *out = ctx->graph_ws;
  return DVO_AMD_OK;
}

}  // namespace

int graph_check_arguments(const char *entry, int n_vertices, const double *poses, int n_edges, const dvo_amd_graph_edge *edges,
                          const dvo_amd_graph_options *opt) {
  auto bad = [entry](const std::string &why) {
    g_last_error = std::string(entry) + ": " + why;
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  };
  if (n_vertices < 0 || n_edges < 0 || !opt || (n_vertices > 0 && !poses) || (n_edges > 0 && !edges))
    return bad("null pointer or negative count");
  if (opt->algorithm != DVO_AMD_GRAPH_LEVENBERG && opt->algorithm != DVO_AMD_GRAPH_DOGLEG) return bad("unknown algorithm");
  if (opt->solver != DVO_AMD_GRAPH_SOLVER_DENSE && opt->solver != DVO_AMD_GRAPH_SOLVER_SPARSE) return bad("unknown solver");
  if (opt->max_iterations < 0 || opt->max_trials < 1) return bad("max_iterations < 0 or max_trials < 1");
  if (!std::isfinite(opt->robust_delta) || !std::isfinite(opt->initial_lambda) || !std::isfinite(opt->initial_delta))
    return bad("non-finite option");
  for (int v = 0; v < n_vertices; ++v)
    if (!finite_all(poses + 16 * (size_t)v, 16)) return bad("non-finite pose of vertex " + std::to_string(v));
  for (int k = 0; k < n_edges; ++k) {
    const dvo_amd_graph_edge &E = edges[k];
    const std::string id = " (edge " + std::to_string(k) + ")";
    if (E.from < 0 || E.from >= n_vertices || E.to < 0 || E.to >= n_vertices) return bad("vertex index out of range" + id);
    if (E.from == E.to) return bad("from == to" + id);
    if (!finite_all(E.measurement, 16) || !finite_all(E.information, 36)) return bad("non-finite measurement or information" + id);
    for (int r = 0; r < 6; ++r)
      for (int c = r + 1; c < 6; ++c) {
        const double a = E.information[c * 6 + r], b = E.information[r * 6 + c];
        if (std::fabs(a - b) > 1e-9 * std::max(std::max(std::fabs(a), std::fabs(b)), 1e-300))
          return bad("information matrix not symmetric" + id);
      }
  }
  return DVO_AMD_OK;
}

namespace {

// ---- the sparse solver's symbolic phase (host, once per call): nested dissection on the m x m block pattern ---------------
constexpr int kLeafVertices = 16;

struct Symbolic {
  int m = 0, n_fronts = 0, n_levels = 0, widest = 0;
  std::vector<int> perm, pos;                    // perm[k] = the slot eliminated k-th; pos = its inverse
  std::vector<int> parent, level;                // per front (postorder: children before parents); level 0 = leaves
  std::vector<int> piv_ptr, piv, upd_ptr, upd;   // CSR: pivot slots, update slots (both in elimination order)
  std::vector<int> child_ptr, child;             // CSR: children in a fixed order
  double factor_doubles = 0.0, flops = 0.0, front_doubles = 0.0;
  double vector_doubles = 0.0, map_ints = 0.0;  // the fronts' vectors; hmap + inv + loc entries
  std::vector<int> ld, ppad;                     // the device layout of each front
};

// adjacency of the free active slots (sorted, without repeats)
std::vector<std::vector<int>> block_adjacency(int m, const std::vector<int> &slot, int n_edges, const dvo_amd_graph_edge *edges) {
  std::vector<std::vector<int>> adj(m);
  for (int k = 0; k < n_edges; ++k) {
    const int f = slot[edges[k].from], t = slot[edges[k].to];
    if (f >= 0 && t >= 0) adj[f].push_back(t), adj[t].push_back(f);
  }
  for (auto &a : adj) {
    std::sort(a.begin(), a.end());
    a.erase(std::unique(a.begin(), a.end()), a.end());
  }
  return adj;
}

struct Dissection {
  const std::vector<std::vector<int>> &adj;
  std::vector<int> owner, seen, dist;  // owner: the set a slot belongs to now; seen: BFS stamps
  int sets = 0, stamp = 0;
  std::vector<std::vector<int>> piv, children;  // per front, in creation order (= postorder)

  explicit Dissection(const std::vector<std::vector<int>> &a)
      : adj(a), owner(a.size(), -1), seen(a.size(), -1), dist(a.size(), 0) {}

  int front(std::vector<int> p, std::vector<int> ch) {
    piv.push_back(std::move(p));
    children.push_back(std::move(ch));
    return (int)piv.size() - 1;
  }

  // BFS inside set `id` from r: the vertices in BFS order (neighbours in slot order), dist[] their levels
  void bfs(int r, int id, std::vector<int> &order) {
    ++stamp;
    order.clear();
    order.push_back(r);
    seen[r] = stamp;
    dist[r] = 0;
    for (size_t h = 0; h < order.size(); ++h) {
      const int v = order[h];
      for (int w : adj[v])
        if (owner[w] == id && seen[w] != stamp) {
          seen[w] = stamp;
          dist[w] = dist[v] + 1;
          order.push_back(w);
        }
    }
  }

  int degree_in(int v, int id) const {
    int d = 0;
    for (int w : adj[v]) d += owner[w] == id;
    return d;
  }

  // the roots of the fronts made for `verts` (sorted slots)
  std::vector<int> run(std::vector<int> verts) {
    if ((int)verts.size() <= kLeafVertices) return {front(std::move(verts), {})};
    const int id = sets++;
    for (int v : verts) owner[v] = id;
    // components, by their smallest slot
    std::vector<std::vector<int>> comps;
    std::vector<int> order;
    {
      const int cstamp = ++stamp;
      std::vector<int> queue;
      for (int v : verts) {
        if (seen[v] == cstamp) continue;
        queue.assign(1, v);
        seen[v] = cstamp;
        for (size_t h = 0; h < queue.size(); ++h)
          for (int w : adj[queue[h]])
            if (owner[w] == id && seen[w] != cstamp) seen[w] = cstamp, queue.push_back(w);
        std::sort(queue.begin(), queue.end());
        comps.push_back(queue);
      }
    }
    if (comps.size() > 1) {  // a forest: small components share a leaf front, large ones are dissected on their own
      std::vector<int> roots, bin;
      for (auto &c : comps) {
        if ((int)c.size() > kLeafVertices) {
          for (int r : run(std::move(c))) roots.push_back(r);
          continue;
        }
        if ((int)(bin.size() + c.size()) > kLeafVertices) {
          std::sort(bin.begin(), bin.end());
          roots.push_back(front(std::move(bin), {}));
          bin.clear();
        }
        bin.insert(bin.end(), c.begin(), c.end());
      }
      if (!bin.empty()) {
        std::sort(bin.begin(), bin.end());
        roots.push_back(front(std::move(bin), {}));
      }
      return roots;
    }
    // a pseudo-peripheral vertex: from the smallest slot, move to a vertex of the last level of least degree while the
    // eccentricity grows
    int r = verts[0];
    bfs(r, id, order);
    for (int round = 0; round < 8; ++round) {
      const int ecc = dist[order.back()];
      int best = -1;
      for (int i = (int)order.size() - 1; i >= 0 && dist[order[i]] == ecc; --i) {
        const int v = order[i];
        if (best < 0 || degree_in(v, id) < degree_in(best, id) || (degree_in(v, id) == degree_in(best, id) && v < best))
          best = v;
      }
      std::vector<int> o2;
      bfs(best, id, o2);
      if (dist[o2.back()] <= ecc) {
        bfs(r, id, order);  // restore r's levels
        break;
      }
      r = best;
      order.swap(o2);
    }
    const int depth = dist[order.back()];
    if (depth < 2) return {front(std::move(verts), {})};  // no level separates anything: one dense front
    std::vector<int> count(depth + 1, 0), sep_count(depth + 1, 0);
    for (int v : order) {
      ++count[dist[v]];
      for (int w : adj[v])
        if (owner[w] == id && dist[w] == dist[v] + 1) {
          ++sep_count[dist[v]];
          break;
        }
    }
    // the separator: the vertices of one level with a neighbour in the next.  Among levels that leave both sides at least a
    // quarter of the set, the smallest separator, then the better balance, then the lower level; without such a level the
    // least |separator| x larger side
    const long long total = (long long)verts.size();
    int pick = -1;
    long long best_key[3] = {0, 0, 0};
    bool balanced_found = false;
    long long below_prefix = 0;
    for (int i = 1; i < depth; ++i) {
      below_prefix += count[i - 1];
      const long long sep = sep_count[i], below = below_prefix + count[i] - sep, above = total - below_prefix - count[i];
      const bool balanced = 4 * std::min(below, above) >= total;
      const long long key[3] = {balanced ? sep : sep * std::max(below, above), std::max(below, above), i};
      if (balanced && !balanced_found) balanced_found = true, pick = -1;
      if (balanced_found && !balanced) continue;
      if (pick < 0 || std::lexicographical_compare(key, key + 3, best_key, best_key + 3)) {
        pick = i;
        std::copy(key, key + 3, best_key);
      }
    }
    std::vector<int> sep, below, above;
    for (int v : verts) {
      if (dist[v] > pick) {
        above.push_back(v);
      } else if (dist[v] < pick) {
        below.push_back(v);
      } else {
        bool cut = false;
        for (int w : adj[v]) cut = cut || (owner[w] == id && dist[w] == pick + 1);
        (cut ? sep : below).push_back(v);
      }
    }
    std::vector<int> roots = run(std::move(below));
    for (int x : run(std::move(above))) roots.push_back(x);
    return {front(std::move(sep), std::move(roots))};
  }
};

// ordering, assembly tree, update sets, levels, the device layout and the predicted storage and flops
Symbolic symbolic(const std::vector<std::vector<int>> &adj) {
  Symbolic S;
  const int m = (int)adj.size();
  S.m = m;
  if (m == 0) {
    S.piv_ptr = S.upd_ptr = S.child_ptr = {0};
    return S;
  }
  Dissection D(adj);
  std::vector<int> all(m);
  for (int s = 0; s < m; ++s) all[s] = s;
  D.run(std::move(all));
  const int nf = (int)D.piv.size();
  S.n_fronts = nf;
  S.pos.assign(m, -1);
  S.piv_ptr.assign(1, 0);
  for (int k = 0; k < nf; ++k) {
    for (int v : D.piv[k]) S.pos[v] = (int)S.perm.size(), S.perm.push_back(v);
    S.piv.insert(S.piv.end(), D.piv[k].begin(), D.piv[k].end());
    S.piv_ptr.push_back((int)S.piv.size());
  }
  S.parent.assign(nf, -1);
  S.level.assign(nf, 0);
  S.child_ptr.assign(1, 0);
  for (int k = 0; k < nf; ++k) {
    for (int c : D.children[k]) {
      S.parent[c] = k;
      S.level[k] = std::max(S.level[k], S.level[c] + 1);
    }
    S.child.insert(S.child.end(), D.children[k].begin(), D.children[k].end());
    S.child_ptr.push_back((int)S.child.size());
  }
  // update set: the later-eliminated neighbours of the pivots, and the children's update sets without this front's pivots
  std::vector<int> tag(m, -1);
  std::vector<std::vector<int>> upd(nf);
  for (int k = 0; k < nf; ++k) {
    const int end = S.pos[S.piv[S.piv_ptr[k + 1] - 1]] + 1;
    auto add = [&](int w) {
      if (S.pos[w] >= end && tag[w] != k) tag[w] = k, upd[k].push_back(w);
    };
    for (int q = S.piv_ptr[k]; q < S.piv_ptr[k + 1]; ++q)
      for (int w : adj[S.piv[q]]) add(w);
    for (int c : D.children[k])
      for (int w : upd[c]) add(w);
    std::sort(upd[k].begin(), upd[k].end(), [&](int a, int b) { return S.pos[a] < S.pos[b]; });
  }
  S.upd_ptr.assign(1, 0);
  for (int k = 0; k < nf; ++k) {
    S.upd.insert(S.upd.end(), upd[k].begin(), upd[k].end());
    S.upd_ptr.push_back((int)S.upd.size());
    const double p = 6.0 * (S.piv_ptr[k + 1] - S.piv_ptr[k]), u = 6.0 * upd[k].size();
    S.factor_doubles += p * (p + 1) / 2 + u * p;
    S.flops += p * p * p / 3.0 + u * p * p + u * u * p;  // potrf, trsm, the update matrix
    S.n_levels = std::max(S.n_levels, S.level[k] + 1);
    S.widest = std::max(S.widest, (int)(p + u));
    const int np = (int)p, nu = (int)u;
    const bool wide = np > graph::kWidePivots || np + nu > graph::kSmallMaxLd;
    const int pp = wide ? (int)align_up(np, graph::kTile) : np;
    const int ld = wide ? (int)align_up(pp + nu, graph::kTile) : np + nu;
    S.ppad.push_back(pp);
    S.ld.push_back(ld);
    S.front_doubles += (double)ld * ld;
    S.vector_doubles += ld;
    S.map_ints += (double)(np + nu) / 6 * (np / 6) + (np + nu) / 6;  // hmap, loc
  }
  for (int k = 0; k < nf; ++k)
    if (S.parent[k] >= 0) {
      const int q = S.parent[k];
      S.map_ints += (S.piv_ptr[q + 1] - S.piv_ptr[q]) + (S.upd_ptr[q + 1] - S.upd_ptr[q]);  // inv
    }
  return S;
}

// one call: the device state and the host's view of the scalars
struct Solver {
  GraphWorkspace &W;
  hipStream_t st;
  int n_vertices, n_edges, m, n, N, nblocks;
  double delta;
  int cholesky_failures = 0;
  bool timed_lin = false, timed_fac = false;
  // the sparse solver's schedule (null: the dense path)
  struct SparsePlan {  // the fronts' device records and maps, and the launch schedule
    std::vector<int> level_begin, small_begin, small_count;  // per level: its fronts in level_ids, its small fronts in small_ids
    std::vector<std::vector<int>> wide;                      // per level: the wide fronts' ids
    std::vector<int> max_ld;                                 // per level
    std::vector<graph::Front> fronts;                        // host copy (wide fronts' offsets)
    // what the sparse path uploads besides the contributor lists
    std::vector<int2> slot_rc;  // (row, col) slots of the stored blocks
    std::vector<int> bsr_ptr, diag_block, hmap, inv, child_list, loc, level_ids, small_ids;
  };
  const SparsePlan *sp = nullptr;

  double *poses() { return (double *)W.poses.p; }
  double *H() { return (double *)W.H.p; }
  double *L() { return (double *)W.L.p; }
  double *b() { return (double *)W.b.p; }
  double *x() { return (double *)W.x.p; }
  double *hsd() { return (double *)W.hsd.p; }
  double *hdl() { return (double *)W.hdl.p; }
  double *aux() { return (double *)W.aux.p; }
  int *flag() { return (int *)W.flag.p; }
  double *scalars() { return (double *)W.scalars.p; }

  int objective_enqueue() {
    if (n_edges > 0)
      hipLaunchKernelGGL(graph::k_objective, dim3(graph::grid_for(n_edges, 64)), dim3(64), 0, st, n_edges,
                         (const dvo_amd_graph_edge *)W.edges.p, poses(), delta, (double *)W.rho0.p, (double *)W.chi2.p,
                         (double *)W.rho1.p);
    HIP_TRY(hipGetLastError());
    return DVO_AMD_OK;
  }

  // up to kMaxDots reductions into scalars[slot..]; {a, b, mode, lambda}
  struct Dot {
    const double *a, *b;
    int mode;
    double lambda;
    int n;
  };
  int dots_enqueue(std::initializer_list<Dot> list, int first_slot) {
    graph::DotArgs args;
    std::memset(&args, 0, sizeof(args));
    int d = 0;
    for (const Dot &x : list) {
      args.a[d] = x.a;
      args.b[d] = x.b;
      args.mode[d] = x.mode;
      args.lambda[d] = x.lambda;
      args.n[d] = x.n;
      ++d;
    }
    hipLaunchKernelGGL(graph::k_dots, dim3(d), dim3(graph::kDotThreads), 0, st, args, scalars() + first_slot);
    HIP_TRY(hipGetLastError());
    return DVO_AMD_OK;
  }

  // reads scalars[0..count) and the factorization flag
  int read(double *s, int count, int *flag_out) {
    if (count > 0) HIP_TRY(hipMemcpyAsync(s, scalars(), sizeof(double) * count, hipMemcpyDeviceToHost, st));
    int f = -1;
    if (flag_out) HIP_TRY(hipMemcpyAsync(&f, flag(), sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (flag_out) *flag_out = f;
    return DVO_AMD_OK;
  }

  // F at the current estimate
  int objective(double *F) {
    int rc = objective_enqueue();
    if (!rc) rc = dots_enqueue({{(const double *)W.rho0.p, nullptr, 0, 0.0, n_edges}}, 0);
    if (!rc) rc = read(F, 1, nullptr);
    return rc;
  }

  int linearise() {
    if (!timed_lin) HIP_TRY(hipEventRecord(W.ev[0], st));
    hipLaunchKernelGGL(graph::k_linearise, dim3(graph::grid_for(n_edges, 64)), dim3(64), 0, st, n_edges,
                       (const dvo_amd_graph_edge *)W.edges.p, poses(), delta, (double *)W.rec.p);
    // the sparse path stores block k at Hs + 36 k: block_rc holds (k, 0) and the row stride is 6
    hipLaunchKernelGGL(graph::k_assemble_H, dim3(nblocks), dim3(64), 0, st, (const int2 *)W.block_rc.p,
                       (const int *)W.block_ptr.p, (const int *)W.block_c.p, (const double *)W.rec.p,
                       sp ? (double *)W.Hs.p : H(), sp ? 6 : N);
    hipLaunchKernelGGL(graph::k_assemble_b, dim3(graph::grid_for(n, 256)), dim3(256), 0, st, n, (const int *)W.b_ptr.p,
                       (const int *)W.b_c.p, (const double *)W.rec.p, b());
    HIP_TRY(hipGetLastError());
    if (!timed_lin) HIP_TRY(hipEventRecord(W.ev[1], st));
    return DVO_AMD_OK;
  }

  // max |diag(H)| into scalars[0]
  int max_diag_enqueue() {
    if (sp)
      hipLaunchKernelGGL(graph::k_max_diag_blocks, dim3(1), dim3(graph::kBlock), 0, st, n, (const int *)W.diag_block.p,
                         (const double *)W.Hs.p, scalars());
    else
      hipLaunchKernelGGL(graph::k_max_diag, dim3(1), dim3(graph::kBlock), 0, st, (const double *)H(), N, n, scalars());
    HIP_TRY(hipGetLastError());
    return DVO_AMD_OK;
  }

  // blocked right-looking Cholesky of the leading P tile columns of a (ld x ld): the dense L (P = all tiles) or a wide front
  // (P = its pivot tiles; the trailing tiles are left holding the update matrix)
  void tiled_cholesky_enqueue(double *a, int ld, int P) {
    const int T = ld / graph::kTile;
    for (int t = 0; t < P; ++t) {
      hipLaunchKernelGGL(graph::k_potrf_panel, dim3(1), dim3(graph::kBlock), 0, st, a, ld, t, flag());
      if (t + 1 < T) {
        hipLaunchKernelGGL(graph::k_trsm, dim3(T - t - 1), dim3(graph::kBlock), 0, st, a, ld, t, (const int *)flag());
        hipLaunchKernelGGL(graph::k_syrk, dim3(T - t - 1, T - t - 1), dim3(graph::kBlock), 0, st, a, ld, t, (const int *)flag());
      }
    }
  }

  // the factorized fronts applied to `rhs`: forward substitution leaves first, backward root first, the solution into `out`
  void sparse_solve_enqueue(const double *rhs, double *out) {
    const graph::Front *fr = (const graph::Front *)W.fronts.p;
    const int *ids = (const int *)W.level_ids.p;
    const double *A = (const double *)W.A.p;
    double *V = (double *)W.V.p;
    const int levels = (int)sp->level_begin.size() - 1;
    for (int l = 0; l < levels; ++l)
      hipLaunchKernelGGL(graph::k_front_forward, dim3(sp->level_begin[l + 1] - sp->level_begin[l]), dim3(graph::kFrontThreads),
                         0, st, fr, ids + sp->level_begin[l], A, (const int *)W.loc.p, (const int *)W.inv.p,
                         (const int *)W.child_list.p, rhs, V, (const int *)flag());
    for (int l = levels - 1; l >= 0; --l)
      hipLaunchKernelGGL(graph::k_front_backward, dim3(sp->level_begin[l + 1] - sp->level_begin[l]),
                         dim3(graph::kFrontThreads), 0, st, fr, ids + sp->level_begin[l], A, (const int *)W.loc.p, V, out,
                         (const int *)flag());
  }

  int sparse_factor_solve_enqueue(bool damp, double lambda, double *out) {
    const graph::Front *fr = (const graph::Front *)W.fronts.p;
    const int *ids = (const int *)W.level_ids.p, *small = (const int *)W.small_ids.p;
    double *A = (double *)W.A.p;
    if (!timed_fac) HIP_TRY(hipEventRecord(W.ev[2], st));
    HIP_TRY(hipMemsetAsync(flag(), 0xff, sizeof(int), st));
    const int levels = (int)sp->level_begin.size() - 1;
    for (int l = 0; l < levels; ++l) {
      const int count = sp->level_begin[l + 1] - sp->level_begin[l];
      const int gx = std::min(64, graph::grid_for((size_t)sp->max_ld[l] * sp->max_ld[l], graph::kBlock));
      hipLaunchKernelGGL(graph::k_front_assemble, dim3(gx, count), dim3(graph::kBlock), 0, st, fr, ids + sp->level_begin[l],
                         (const double *)W.Hs.p, (const int *)W.hmap.p, (const int *)W.inv.p, (const int *)W.child_list.p,
                         A, lambda, damp ? 1 : 0, (const int *)flag());
      if (sp->small_count[l])
        hipLaunchKernelGGL(graph::k_front_factor, dim3(sp->small_count[l]), dim3(graph::kFrontThreads), 0, st, fr,
                           small + sp->small_begin[l], A, flag());
      for (int k : sp->wide[l])  // the dense path's tiled kernels on the front, over its pivot tiles
        tiled_cholesky_enqueue(A + sp->fronts[k].a_off, sp->fronts[k].ld, sp->fronts[k].ppad / graph::kTile);
    }
    HIP_TRY(hipGetLastError());
    if (!timed_fac) HIP_TRY(hipEventRecord(W.ev[3], st));
    sparse_solve_enqueue(b(), out);
    HIP_TRY(hipGetLastError());
    if (!timed_fac) HIP_TRY(hipEventRecord(W.ev[4], st));
    ++W.factorizations;
    return DVO_AMD_OK;
  }

  // (H + lambda I) x = b (damp) or H x = b into `out`; the flag word says whether a pivot failed (read by the caller)
  int factor_solve_enqueue(bool damp, double lambda, double *out) {
    if (sp) return sparse_factor_solve_enqueue(damp, lambda, out);
    if (!timed_fac) HIP_TRY(hipEventRecord(W.ev[2], st));
    HIP_TRY(hipMemsetAsync(flag(), 0xff, sizeof(int), st));
    hipLaunchKernelGGL(graph::k_damp_copy, dim3(std::min(4096, graph::grid_for((size_t)N * N, 256))), dim3(256), 0, st,
                       (const double *)H(), L(), N, n, lambda, damp ? 1 : 0);
    tiled_cholesky_enqueue(L(), N, N / graph::kTile);
    HIP_TRY(hipGetLastError());
    if (!timed_fac) HIP_TRY(hipEventRecord(W.ev[3], st));
    hipLaunchKernelGGL(graph::k_trsv, dim3(1), dim3(graph::kSolveThreads), 0, st, (const double *)L(), N,
                       (const double *)b(), out, (const int *)flag());
    HIP_TRY(hipGetLastError());
    ++W.factorizations;
    return DVO_AMD_OK;
  }

  void note_failure(int f) {
    if (f >= 0) ++cholesky_failures;
  }

  int push() {
    HIP_TRY(hipMemcpyAsync(W.saved.p, W.poses.p, 16 * sizeof(double) * (size_t)n_vertices, hipMemcpyDeviceToDevice, st));
    return DVO_AMD_OK;
  }
  int pop() {
    HIP_TRY(hipMemcpyAsync(W.poses.p, W.saved.p, 16 * sizeof(double) * (size_t)n_vertices, hipMemcpyDeviceToDevice, st));
    return DVO_AMD_OK;
  }
  int update_enqueue(const double *step, bool guarded) {
    hipLaunchKernelGGL(graph::k_update, dim3(graph::grid_for(m, 64)), dim3(64), 0, st, m, (const int *)W.vertex_of.p, step,
                       poses(), guarded ? (const int *)flag() : nullptr);
    HIP_TRY(hipGetLastError());
    return DVO_AMD_OK;
  }
  int vec(int mode, double alpha, const double *x_, const double *y_, double *out) {
    hipLaunchKernelGGL(graph::k_vec, dim3(graph::grid_for(n, 256)), dim3(256), 0, st, n, mode, alpha, x_, y_, out);
    HIP_TRY(hipGetLastError());
    return DVO_AMD_OK;
  }
  int matvec(const double *v, double *y) {
    if (sp)
      hipLaunchKernelGGL(graph::k_bsr_matvec, dim3(graph::grid_for(n, 256)), dim3(256), 0, st, n, (const int *)W.bsr_ptr.p,
                         (const int2 *)W.bsr_rc.p, (const double *)W.Hs.p, v, y);
    else
      hipLaunchKernelGGL(graph::k_matvec, dim3(graph::grid_for(n, graph::kBlock / 64)), dim3(graph::kBlock), 0, st,
                         (const double *)H(), N, n, v, y);
    HIP_TRY(hipGetLastError());
    return DVO_AMD_OK;
  }
};

// one graph as an entry was given it; `entry` prefixes dvo_amd_last_error()
struct Problem {
  const char *entry;
  int n_vertices;
  const double *poses;
  const int *fixed;
  int n_edges;
  const dvo_amd_graph_edge *edges;
};

// prepare()'s result: the device holds the problem, the objective at the given estimate is known, nothing is linearised yet.
// It owns every host array an asynchronous upload reads, so it lives until its driver's final synchronize.
struct Prepared {
  Unknowns U;
  Contributors C;
  Symbolic sym;     // sparse only
  Solver::SparsePlan plan;  // sparse only
  std::optional<Solver> solver;
  double F0 = 0.0;  // the objective at the given estimate
};

// dvo_amd_graph_marginals: the requests between free active vertices, and what the device stage reports
struct MargJob {
  int n = 0;
  const int *a = nullptr, *b = nullptr;  // vertex indices
  double *out = nullptr;                 // 36 n: block k column-major at out + 36 k
  int failed_pivot = -1, solved_columns = 0;
};

// one front's tile columns, last pivot tile first (the dense solver: the whole matrix, P = T)
int tiled_selinv_enqueue(Solver &S, const double *L, double *Z, int ld, int P) {
  const int T = ld / graph::kTile;
  double *Wt = (double *)S.W.wtile.p, *Y = (double *)S.W.ytiles.p;
  for (int t = P - 1; t >= 0; --t) {
    hipLaunchKernelGGL(graph::k_tile_inverse, dim3(1), dim3(graph::kBlock), 0, S.st, L, ld, t, Wt, (const int *)S.flag());
    if (t + 1 < T) {
      hipLaunchKernelGGL(graph::k_tile_y, dim3(T - t - 1), dim3(graph::kBlock), 0, S.st, L, ld, t, (const double *)Wt, Y,
                         (const int *)S.flag());
      hipLaunchKernelGGL(graph::k_tile_zcol, dim3(T - t - 1), dim3(graph::kBlock), 0, S.st, Z, ld, t, T, (const double *)Y,
                         (const int *)S.flag());
    }
    hipLaunchKernelGGL(graph::k_tile_zdiag, dim3(1), dim3(graph::kBlock), 0, S.st, Z, ld, t, T, (const double *)Wt,
                       (const double *)Y, (const int *)S.flag());
  }
  HIP_TRY(hipGetLastError());
  return DVO_AMD_OK;
}

// after a successful undamped factorization: Z by selected inversion, then the requested blocks
int marginals_stage(Prepared &P, MargJob &J) {
  Solver &S = *P.solver;
  const std::vector<int> &slot = P.U.slot, &loc = P.plan.loc;
  const Symbolic *sym = &P.sym;
  GraphWorkspace &W = S.W;
  const hipStream_t st = S.st;
  const int n = S.n, N = S.N, m = S.m;
  auto upload = [&](DeviceBuf &b, const void *src, size_t bytes) {
    return grow_upload(b, src, bytes, st, "graph workspace", "marginals");
  };
  GRAPH_TRY(grow(W.wtile, sizeof(double) * graph::kTile * graph::kTile));
  GRAPH_TRY(grow(W.mout, sizeof(double) * 36 * std::max(J.n, 1)));
  std::vector<graph::MargReq> zreq;
  struct Column {
    int slot;
    std::vector<graph::ColReq> req;
  };
  std::map<int, Column> columns;  // by solved slot
  const double *Z = nullptr;
  // host-side index vectors must outlive the asynchronous uploads: they live until the final synchronize below
  std::vector<graph::SelInfo> info;
  std::vector<int> up;
  std::vector<graph::ColReq> all;
  if (!S.sp) {
    GRAPH_TRY(grow(W.ytiles, sizeof(double) * (size_t)N * graph::kTile));
    GRAPH_TRY(tiled_selinv_enqueue(S, S.L(), S.H(), N, N / graph::kTile));
    Z = S.H();
    for (int k = 0; k < J.n; ++k) zreq.push_back({0, N, 6 * slot[J.a[k]], 6 * slot[J.b[k]], k});
  } else {
    const std::vector<graph::Front> &fr = S.sp->fronts;
    const int nf = (int)fr.size();
    auto scalar_of = [](const graph::Front &F, int local) { return local < F.p ? 6 * local : F.ppad + 6 * (local - F.p); };
    info.assign(nf, graph::SelInfo{-1, 0, 0});
    std::vector<int> where(m, -1), front_of(m, -1);
    int widest = graph::kTile;
    for (int k = 0; k < nf; ++k) {
      const graph::Front &P = fr[k];
      widest = std::max(widest, P.ld);
      for (int b = 0; b < P.p; ++b) front_of[loc[P.loc_off + b]] = k;
      for (int b = 0; b < P.p + P.u; ++b) where[loc[P.loc_off + b]] = scalar_of(P, b);
      for (int q = sym->child_ptr[k]; q < sym->child_ptr[k + 1]; ++q) {
        const int c = sym->child[q];
        info[c] = graph::SelInfo{P.a_off, P.ld, (int)up.size()};
        for (int j = 0; j < fr[c].u; ++j) up.push_back(where[loc[fr[c].loc_off + fr[c].p + j]]);
      }
      for (int b = 0; b < P.p + P.u; ++b) where[loc[P.loc_off + b]] = -1;
    }
    if (up.empty()) up.push_back(0);
    GRAPH_TRY(grow(W.Zinv, sizeof(double) * (size_t)sym->front_doubles));
    GRAPH_TRY(grow(W.ytiles, sizeof(double) * (size_t)widest * graph::kTile));
    GRAPH_TRY(upload(W.sel_info, info.data(), sizeof(graph::SelInfo) * info.size()));
    GRAPH_TRY(upload(W.up, up.data(), sizeof(int) * up.size()));
    const graph::Front *dfr = (const graph::Front *)W.fronts.p;
    const int *ids = (const int *)W.level_ids.p, *small = (const int *)W.small_ids.p;
    double *Zd = (double *)W.Zinv.p;
    const int levels = (int)S.sp->level_begin.size() - 1;
    for (int l = levels - 1; l >= 0; --l) {
      const int count = S.sp->level_begin[l + 1] - S.sp->level_begin[l];
      const int gx = std::min(64, graph::grid_for((size_t)S.sp->max_ld[l] * S.sp->max_ld[l], graph::kBlock));
      hipLaunchKernelGGL(graph::k_front_gather_z22, dim3(gx, count), dim3(graph::kBlock), 0, st, dfr,
                         ids + S.sp->level_begin[l], (const graph::SelInfo *)W.sel_info.p, (const int *)W.up.p, Zd,
                         (const int *)S.flag());
      if (S.sp->small_count[l])
        hipLaunchKernelGGL(graph::k_front_selinv, dim3(S.sp->small_count[l]), dim3(graph::kSelThreads), 0, st, dfr,
                           small + S.sp->small_begin[l], (const double *)W.A.p, Zd, (const int *)S.flag());
      HIP_TRY(hipGetLastError());
      for (int k : S.sp->wide[l])
        GRAPH_TRY(tiled_selinv_enqueue(S, (const double *)W.A.p + fr[k].a_off, Zd + fr[k].a_off, fr[k].ld,
                                       fr[k].ppad / graph::kTile));
    }
    Z = Zd;
    // a pair meets in the front of whichever of the two is eliminated first, if it meets anywhere
    for (int k = 0; k < J.n; ++k) {
      const int sa = slot[J.a[k]], sb = slot[J.b[k]];
      const graph::Front &F = fr[front_of[sym->pos[sa] <= sym->pos[sb] ? sa : sb]];
      int la = -1, lb = -1;
      for (int b = 0; b < F.p + F.u; ++b) {
        if (loc[F.loc_off + b] == sa) la = b;
        if (loc[F.loc_off + b] == sb) lb = b;
      }
      if (la >= 0 && lb >= 0) {
        zreq.push_back({F.a_off, F.ld, scalar_of(F, la), scalar_of(F, lb), k});
      } else {  // the slow path: the block column of the lower slot, whichever order the pair was asked in
        Column &C = columns[std::min(sa, sb)];
        C.slot = std::min(sa, sb);
        C.req.push_back({6 * std::max(sa, sb), k, sa < sb ? 1 : 0});
      }
    }
  }
  if (!zreq.empty()) {
    GRAPH_TRY(upload(W.mreq, zreq.data(), sizeof(graph::MargReq) * zreq.size()));
    hipLaunchKernelGGL(graph::k_marg_gather, dim3(graph::grid_for(36 * zreq.size(), 256)), dim3(256), 0, st, (int)zreq.size(),
                       (const graph::MargReq *)W.mreq.p, Z, (double *)W.mout.p);
    HIP_TRY(hipGetLastError());
  }
  if (!columns.empty()) {
    GRAPH_TRY(grow(W.cols, sizeof(double) * 6 * (size_t)n));
    for (const auto &kv : columns) all.insert(all.end(), kv.second.req.begin(), kv.second.req.end());
    GRAPH_TRY(upload(W.creq, all.data(), sizeof(graph::ColReq) * all.size()));
    size_t first = 0;
    for (const auto &kv : columns) {
      for (int q = 0; q < 6; ++q) {
        hipLaunchKernelGGL(graph::k_unit_vector, dim3(graph::grid_for(n, 256)), dim3(256), 0, st, S.b(), n, 6 * kv.first + q);
        S.sparse_solve_enqueue(S.b(), (double *)W.cols.p + (size_t)q * n);
      }
      const int cnt = (int)kv.second.req.size();
      hipLaunchKernelGGL(graph::k_marg_columns, dim3(graph::grid_for(36 * (size_t)cnt, 256)), dim3(256), 0, st, cnt,
                         (const graph::ColReq *)W.creq.p + first, (const double *)W.cols.p, n, (double *)W.mout.p);
      HIP_TRY(hipGetLastError());
      first += cnt;
    }
    J.solved_columns = (int)columns.size();
  }
  if (J.n) HIP_TRY(hipMemcpyAsync(J.out, W.mout.p, sizeof(double) * 36 * (size_t)J.n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DVO_AMD_OK;
}

void record(dvo_amd_graph_iteration *iterations, int capacity, int it, double F, double step, double lambda, double delta,
            int trials, int accepted) {
  if (iterations && it < capacity) iterations[it] = dvo_amd_graph_iteration{F, step, lambda, delta, trials, accepted};
}

// OptimizationAlgorithmLevenberg::solve, max_iterations times
int run_levenberg(Solver &S, const dvo_amd_graph_options &opt, double *F, dvo_amd_graph_iteration *iterations, int capacity,
                  dvo_amd_graph_stats &stats) {
  double lambda = 0.0, nu = 2.0;
  for (int it = 0; it < opt.max_iterations; ++it) {
    GRAPH_TRY(S.linearise());
    if (it == 0) {
      if (opt.initial_lambda > 0.0) {
        lambda = opt.initial_lambda;
      } else {
        GRAPH_TRY(S.max_diag_enqueue());
        double md = 0.0;
        GRAPH_TRY(S.read(&md, 1, nullptr));
        lambda = 1e-5 * md;
      }
      nu = 2.0;
    }
    int trials = 0;
    double rho = 0.0, step = 0.0;
    int accepted = 0;
    do {
      GRAPH_TRY(S.push());
      GRAPH_TRY(S.factor_solve_enqueue(true, lambda, S.x()));
      GRAPH_TRY(S.update_enqueue(S.x(), true));
      GRAPH_TRY(S.objective_enqueue());
      GRAPH_TRY(S.dots_enqueue({{(const double *)S.W.rho0.p, nullptr, 0, 0.0, S.n_edges},
                                {S.x(), S.b(), 1, lambda, S.n},
                                {S.x(), S.x(), 0, 0.0, S.n}},
                               0));
      double s[3];
      int f = -1;
      GRAPH_TRY(S.read(s, 3, &f));
      S.timed_lin = S.timed_fac = true;
      S.note_failure(f);
      const bool ok = f < 0;
      const double Fp = ok ? s[0] : std::numeric_limits<double>::infinity();
      rho = ok ? (*F - Fp) / (s[1] + 1e-3) : -std::numeric_limits<double>::infinity();
      if (rho > 0.0 && std::isfinite(Fp)) {
        const double alpha = std::min(1.0 - std::pow(2.0 * rho - 1.0, 3), 2.0 / 3.0);
        lambda *= std::max(1.0 / 3.0, alpha);
        nu = 2.0;
        *F = Fp;
        step = std::sqrt(s[2]);
        accepted = 1;
      } else {
        lambda *= nu;
        nu *= 2.0;
        if (ok) GRAPH_TRY(S.pop());
        if (!std::isfinite(lambda)) break;  // before the attempt is counted, as g2o does
      }
      ++trials;
    } while (rho < 0.0 && trials < opt.max_trials);
    record(iterations, capacity, it, *F, step, lambda, 0.0, trials, accepted);
    stats.iterations = it + 1;
    if (trials == opt.max_trials || rho == 0.0 || !std::isfinite(lambda)) {
      stats.termination = DVO_AMD_GRAPH_TERMINATE;
      break;
    }
  }
  stats.lambda = lambda;
  return DVO_AMD_OK;
}

// OptimizationAlgorithmDogleg::solve, max_iterations times
int run_dogleg(Solver &S, const dvo_amd_graph_options &opt, double *F, dvo_amd_graph_iteration *iterations, int capacity,
               dvo_amd_graph_stats &stats) {
  double Delta = opt.initial_delta, lambda = opt.initial_lambda;
  bool was_pd = true;
  const int n = S.n;
  for (int it = 0; it < opt.max_iterations; ++it) {
    GRAPH_TRY(S.linearise());
    // alpha = |b|^2 / b^T H b, h_sd = alpha b
    GRAPH_TRY(S.matvec(S.b(), S.aux()));
    GRAPH_TRY(S.dots_enqueue({{S.b(), S.b(), 0, 0.0, n}, {S.aux(), S.b(), 0, 0.0, n}}, 0));
    double s[4];
    GRAPH_TRY(S.read(s, 2, nullptr));
    const double alpha = s[0] / s[1];
    GRAPH_TRY(S.vec(0, alpha, S.b(), nullptr, S.hsd()));
    GRAPH_TRY(S.dots_enqueue({{S.hsd(), S.hsd(), 0, 0.0, n}}, 0));
    GRAPH_TRY(S.read(s, 1, nullptr));
    const double hsd_sq = s[0], hsd_norm = std::sqrt(hsd_sq);
    double hgn_norm = -1.0, step = 0.0;
    bool solved_gn = false, good = false;
    int trials = 0;
    do {
      ++trials;
      if (!solved_gn) {
        solved_gn = true;
        bool ok = false;
        while (!ok) {
          GRAPH_TRY(S.factor_solve_enqueue(!was_pd, lambda, S.x()));
          GRAPH_TRY(S.dots_enqueue({{S.x(), S.x(), 0, 0.0, n}}, 0));
          int f = -1;
          GRAPH_TRY(S.read(s, 1, &f));
          S.timed_lin = S.timed_fac = true;
          S.note_failure(f);
          ok = f < 0;
          was_pd = was_pd && ok;
          if (!was_pd) {
            if (ok) {
              lambda = std::max(1e-12, lambda / (0.5 * 10.0));
            } else {
              lambda *= 10.0;
              if (lambda > 1e3) {
                lambda = 1e3;
                record(iterations, capacity, it, *F, 0.0, lambda, Delta, trials, 0);
                stats.iterations = it + 1;
                stats.termination = DVO_AMD_GRAPH_FAIL;
                stats.lambda = lambda;
                stats.delta = Delta;
                return DVO_AMD_OK;
              }
            }
          }
        }
        hgn_norm = std::sqrt(s[0]);
      }
      if (hgn_norm < Delta) {
        HIP_TRY(hipMemcpyAsync(S.hdl(), S.x(), sizeof(double) * n, hipMemcpyDeviceToDevice, S.st));
      } else if (hsd_norm > Delta) {
        GRAPH_TRY(S.vec(0, Delta / hsd_norm, S.hsd(), nullptr, S.hdl()));
      } else {
        GRAPH_TRY(S.vec(2, 0.0, S.x(), S.hsd(), S.aux()));  // aux = h_gn - h_sd
        GRAPH_TRY(S.dots_enqueue({{S.hsd(), S.aux(), 0, 0.0, n}, {S.aux(), S.aux(), 0, 0.0, n}}, 0));
        GRAPH_TRY(S.read(s, 2, nullptr));
        const double c = s[0], bma = s[1];
        double beta;
        if (c <= 0.0)
          beta = (-c + std::sqrt(c * c + bma * (Delta * Delta - hsd_sq))) / bma;
        else
          beta = (Delta * Delta - hsd_sq) / (c + std::sqrt(c * c + bma * (Delta * Delta - hsd_sq)));
        GRAPH_TRY(S.vec(1, beta, S.hsd(), S.x(), S.hdl()));
      }
      // linear gain 2 b^T h - h^T H h; then the trial
      GRAPH_TRY(S.matvec(S.hdl(), S.aux()));
      GRAPH_TRY(S.push());
      GRAPH_TRY(S.update_enqueue(S.hdl(), false));
      GRAPH_TRY(S.objective_enqueue());
      GRAPH_TRY(S.dots_enqueue({{S.aux(), S.hdl(), 0, 0.0, n},
                                {S.b(), S.hdl(), 0, 0.0, n},
                                {S.hdl(), S.hdl(), 0, 0.0, n},
                                {(const double *)S.W.rho0.p, nullptr, 0, 0.0, S.n_edges}},
                               0));
      GRAPH_TRY(S.read(s, 4, nullptr));
      double gain = -1.0 * s[0] + 2.0 * s[1];
      const double Fp = s[3], hdl_norm = std::sqrt(s[2]);
      if (std::fabs(gain) < 1e-12) gain = 1e-12;
      const double rho = (*F - Fp) / gain;
      if (rho > 0.0) {
        good = true;
        *F = Fp;
        step = hdl_norm;
      } else {
        GRAPH_TRY(S.pop());
      }
      if (rho > 0.75)
        Delta = std::max(Delta, 3.0 * hdl_norm);
      else if (rho < 0.25)
        Delta *= 0.5;
    } while (!good && trials < opt.max_trials);
    record(iterations, capacity, it, *F, step, lambda, Delta, trials, good ? 1 : 0);
    stats.iterations = it + 1;
    if (trials == opt.max_trials || !good) {
      stats.termination = DVO_AMD_GRAPH_TERMINATE;
      break;
    }
  }
  stats.lambda = lambda;
  stats.delta = Delta;
  return DVO_AMD_OK;
}

// the unknowns of a single-graph entry, refused beyond the solver's capacity
int checked_unknowns(const Problem &P, const dvo_amd_graph_options &opt, Unknowns &U) {
  U = free_unknowns(P.n_vertices, P.fixed, P.n_edges, P.edges);
  const bool sparse = opt.solver == DVO_AMD_GRAPH_SOLVER_SPARSE;
  return check_capacity(P.entry, U.m, sparse ? DVO_AMD_GRAPH_MAX_FREE_VERTICES_SPARSE : DVO_AMD_GRAPH_MAX_FREE_VERTICES,
                        sparse ? "the sparse solver" : "the dense solver");
}

// What the sparse path grows with the problem: fronts, vectors, H blocks, maps, front records (its other buffers are O(m +
// edges)).  marginal_requests >= 0 adds the inverse: a second arena of fronts, a tile column, six columns, maps, the blocks.
double sparse_bytes_needed(const Symbolic &sym, size_t n_blocks, int m, int marginal_requests) {
  double need = sizeof(double) * (sym.front_doubles + sym.vector_doubles + 36.0 * n_blocks) + sizeof(int) * sym.map_ints +
                sizeof(graph::Front) * (double)sym.n_fronts;
  if (marginal_requests >= 0) {
    const int widest_ld = sym.ld.empty() ? 0 : *std::max_element(sym.ld.begin(), sym.ld.end());
    need += sizeof(double) * (sym.front_doubles + (double)graph::kTile * (widest_ld + graph::kTile) + 36.0 * m +
                              36.0 * marginal_requests) +
            (sizeof(graph::SelInfo) + sizeof(int)) * (double)sym.n_fronts + sizeof(int) * (double)sym.upd.size() +
            sizeof(graph::MargReq) * (double)marginal_requests;
  }
  return need;
}

// The fronts' device records and maps and the level schedule.  block_rc (the sorted (row, col) slots of the stored blocks) is
// kept as slot_rc and rewritten in place to (k, 0): k_assemble_H then writes block k at Hs + 36 k with a row stride of 6.
Solver::SparsePlan build_sparse_plan(const Symbolic &sym, std::vector<int2> &block_rc, int m) {
  Solver::SparsePlan P;
  Solver::SparsePlan &sched = P;
  std::vector<int> &loc = P.loc, &hmap = P.hmap, &inv = P.inv, &child_list = P.child_list;
  P.slot_rc = block_rc;
  P.bsr_ptr.assign(m + 1, 0);
  P.diag_block.assign(m, -1);
  std::map<long long, int> block_index;
  for (int k = 0; k < (int)block_rc.size(); ++k) {
    ++P.bsr_ptr[block_rc[k].x + 1];
    if (block_rc[k].x == block_rc[k].y) P.diag_block[block_rc[k].x] = k;
    block_index[(long long)block_rc[k].x * m + block_rc[k].y] = k;
    block_rc[k] = make_int2(k, 0);
  }
  for (int s = 0; s < m; ++s) P.bsr_ptr[s + 1] += P.bsr_ptr[s];
  const int nf = sym.n_fronts;
  sched.fronts.resize(nf);
  long long a_off = 0, h_off = 0;
  int v_off = 0;
  for (int k = 0; k < nf; ++k) {
    graph::Front &F = sched.fronts[k];
    F.p = sym.piv_ptr[k + 1] - sym.piv_ptr[k];
    F.u = sym.upd_ptr[k + 1] - sym.upd_ptr[k];
    F.ld = sym.ld[k];
    F.ppad = sym.ppad[k];
    F.a_off = a_off;
    F.v_off = v_off;
    F.hmap_off = h_off;
    F.loc_off = (int)loc.size();
    a_off += (long long)F.ld * F.ld;
    v_off += F.ld;
    loc.insert(loc.end(), sym.piv.begin() + sym.piv_ptr[k], sym.piv.begin() + sym.piv_ptr[k + 1]);
    loc.insert(loc.end(), sym.upd.begin() + sym.upd_ptr[k], sym.upd.begin() + sym.upd_ptr[k + 1]);
    const int f = F.p + F.u;
    hmap.resize(h_off + (long long)f * F.p, -1);
    for (int r = 0; r < f; ++r)
      for (int c = 0; c < F.p && c <= r; ++c) {
        const auto it = block_index.find((long long)loc[F.loc_off + r] * m + loc[F.loc_off + c]);
        if (it != block_index.end()) hmap[h_off + (long long)r * F.p + c] = it->second;
      }
    h_off += (long long)f * F.p;
    F.ch_begin = (int)child_list.size();
    child_list.insert(child_list.end(), sym.child.begin() + sym.child_ptr[k], sym.child.begin() + sym.child_ptr[k + 1]);
    F.ch_end = (int)child_list.size();
  }
  // each child's map from its parent's local blocks into its own update set
  std::vector<int> where(m, -1);
  for (int k = 0; k < nf; ++k) {
    const graph::Front &Pa = sched.fronts[k];
    for (int q = sym.child_ptr[k]; q < sym.child_ptr[k + 1]; ++q) {
      graph::Front &C = sched.fronts[sym.child[q]];
      for (int j = 0; j < C.u; ++j) where[loc[C.loc_off + C.p + j]] = j;
      C.inv_off = (int)inv.size();
      for (int b = 0; b < Pa.p + Pa.u; ++b) inv.push_back(where[loc[Pa.loc_off + b]]);
      for (int j = 0; j < C.u; ++j) where[loc[C.loc_off + C.p + j]] = -1;
    }
  }
  for (int k = 0; k < nf; ++k)
    if (sym.parent[k] < 0) sched.fronts[k].inv_off = 0;  // roots have no parent and an empty update set
  if (inv.empty()) inv.push_back(-1);
  // the level schedule: fronts by level (leaves first), in front order within a level
  const int L = sym.n_levels;
  sched.level_begin.assign(1, 0);
  sched.small_begin.assign(1, 0);
  sched.small_count.assign(L, 0);
  sched.wide.assign(L, {});
  sched.max_ld.assign(L, 0);
  for (int l = 0; l < L; ++l) {
    for (int k = 0; k < nf; ++k) {
      if (sym.level[k] != l) continue;
      P.level_ids.push_back(k);
      sched.max_ld[l] = std::max(sched.max_ld[l], sched.fronts[k].ld);
      const bool wide = sched.fronts[k].ppad != 6 * sched.fronts[k].p || sched.fronts[k].ld > graph::kSmallMaxLd ||
                        6 * sched.fronts[k].p > graph::kWidePivots;
      if (wide)
        sched.wide[l].push_back(k);
      else
        P.small_ids.push_back(k), ++sched.small_count[l];
    }
    sched.level_begin.push_back((int)P.level_ids.size());
    sched.small_begin.push_back((int)P.small_ids.size());
  }
  return P;
}

// Puts the problem on the device for the unknowns U (checked by the caller): contributor lists; sparse: the symbolic phase, the
// memory check and the plan; workspace growth, uploads, the cleared H and b, a Solver, the objective at the given estimate.
int prepare(dvo_amd_context *ctx, const Problem &P, const dvo_amd_graph_options &opt, int marginal_requests, Unknowns &&U,
            Prepared &out) {
  out.U = std::move(U);
  out.C = contributor_lists(out.U, P.n_edges, P.edges, false);
  const bool sparse = opt.solver == DVO_AMD_GRAPH_SOLVER_SPARSE;
  const int m = out.U.m, n = 6 * m, N = sparse ? n : std::max(graph::kTile, (int)align_up((size_t)n, graph::kTile));
  const int n_vertices = P.n_vertices, n_edges = P.n_edges;
  Contributors &C = out.C;
  const Symbolic &sym = out.sym;
  Solver::SparsePlan &plan = out.plan;
  double symbolic_ms = 0.0;
  HIP_TRY(hipSetDevice(ctx->device));
  if (sparse) {
    const auto t0 = std::chrono::steady_clock::now();
    out.sym = symbolic(block_adjacency(m, out.U.slot, n_edges, P.edges));
    symbolic_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // against 90 % of the free memory plus what the context already holds of the estimated buffers
    const double held = ctx->graph_ws ? ctx->graph_ws->held_bytes(marginal_requests >= 0) : 0.0;
    const double need = sparse_bytes_needed(sym, C.block_rc.size(), m, marginal_requests);
    if (need > ((double)free_b + held) * 0.9) {
      g_last_error = std::string(P.entry) + ": the sparse factorization needs " +
                     std::to_string((long long)(need / 1048576.0)) + " MiB of device storage";
      return DVO_AMD_ERR_OUT_OF_MEMORY;
    }
    plan = build_sparse_plan(sym, C.block_rc, m);
  }
  GraphWorkspace *Wp = nullptr;
  GRAPH_TRY(workspace(ctx, &Wp));
  GraphWorkspace &W = *Wp;
  const size_t E = std::max(n_edges, 1);
  const std::vector<int> &vertex_of = out.U.vertex_of;
  const struct {
    DeviceBuf &buf;
    const void *src;
    size_t bytes;
  } uploads[] = {{W.poses, P.poses, 16 * sizeof(double) * n_vertices}, {W.edges, P.edges, sizeof(dvo_amd_graph_edge) * n_edges},
                 {W.block_rc, C.block_rc.data(), sizeof(int2) * C.block_rc.size()},
                 {W.block_ptr, C.block_ptr.data(), sizeof(int) * C.block_ptr.size()},
                 {W.block_c, C.block_c.data(), sizeof(int) * C.block_c.size()},
                 {W.b_ptr, C.b_ptr.data(), sizeof(int) * C.b_ptr.size()}, {W.b_c, C.b_c.data(), sizeof(int) * C.b_c.size()},
                 {W.vertex_of, vertex_of.data(), sizeof(int) * vertex_of.size()}};
  for (const auto &u : uploads) GRAPH_TRY(grow(u.buf, std::max<size_t>(1, u.bytes)));
  GRAPH_TRY(grow(W.saved, 16 * sizeof(double) * std::max(n_vertices, 1)));
  GRAPH_TRY(grow(W.rec, sizeof(double) * graph::kRecord * E));
  for (DeviceBuf *b : {&W.rho0, &W.chi2, &W.rho1}) GRAPH_TRY(grow(*b, sizeof(double) * E));
  if (!sparse) {
    GRAPH_TRY(grow(W.H, sizeof(double) * (size_t)N * N));
    GRAPH_TRY(grow(W.L, sizeof(double) * (size_t)N * N));
  }
  // at least one double: a sparse call with no free active vertex has N = 0 and still clears b
  for (DeviceBuf *b : {&W.b, &W.x, &W.hsd, &W.hdl, &W.aux}) GRAPH_TRY(grow(*b, sizeof(double) * std::max(N, 1)));
  GRAPH_TRY(grow(W.scalars, sizeof(double) * graph::kMaxDots));
  GRAPH_TRY(grow(W.flag, sizeof(int)));
  W.n_padded = N;
  W.factorizations = 0;
  W.lin_ms = W.fac_ms = 0.0;
  const hipStream_t st = ctx->stream;
  if (sparse) {
    auto grow_up = [&](DeviceBuf &b, const void *src, size_t bytes) {
      return grow_upload(b, src, bytes, st, "graph workspace", "sparse maps");
    };
    GRAPH_TRY(grow(W.Hs, sizeof(double) * 36 * std::max<size_t>(1, C.block_rc.size())));
    GRAPH_TRY(grow_up(W.bsr_ptr, plan.bsr_ptr.data(), sizeof(int) * plan.bsr_ptr.size()));
    GRAPH_TRY(grow_up(W.bsr_rc, plan.slot_rc.data(), sizeof(int2) * plan.slot_rc.size()));
    GRAPH_TRY(grow_up(W.diag_block, plan.diag_block.data(), sizeof(int) * plan.diag_block.size()));
    GRAPH_TRY(grow_up(W.fronts, plan.fronts.data(), sizeof(graph::Front) * plan.fronts.size()));
    GRAPH_TRY(grow_up(W.hmap, plan.hmap.data(), sizeof(int) * plan.hmap.size()));
    GRAPH_TRY(grow_up(W.inv, plan.inv.data(), sizeof(int) * plan.inv.size()));
    GRAPH_TRY(grow_up(W.child_list, plan.child_list.data(), sizeof(int) * plan.child_list.size()));
    GRAPH_TRY(grow_up(W.loc, plan.loc.data(), sizeof(int) * plan.loc.size()));
    GRAPH_TRY(grow_up(W.level_ids, plan.level_ids.data(), sizeof(int) * plan.level_ids.size()));
    GRAPH_TRY(grow_up(W.small_ids, plan.small_ids.data(), sizeof(int) * plan.small_ids.size()));
    GRAPH_TRY(grow(W.A, sizeof(double) * (size_t)sym.front_doubles));
    GRAPH_TRY(grow(W.V, sizeof(double) * (size_t)sym.vector_doubles));
    W.sp_symbolic_ms = symbolic_ms;
    W.sp_lin_ms = W.sp_fac_ms = W.sp_solve_ms = 0.0;
    W.sp_fronts = sym.n_fronts;
    W.sp_levels = sym.n_levels;
    W.sp_widest = sym.widest;
    W.sp_factor_doubles = sym.factor_doubles;
    W.sp_flops = sym.flops;
  }
  for (const auto &u : uploads)
    if (u.bytes) HIP_TRY(hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, st));
  // blocks no edge touches stay zero; the padding is the identity (its unknowns solve to 0)
  if (!sparse) HIP_TRY(hipMemsetAsync(W.H.p, 0, sizeof(double) * (size_t)N * N, st));
  HIP_TRY(hipMemsetAsync(W.b.p, 0, sizeof(double) * std::max(N, 1), st));
  if (N > n) hipLaunchKernelGGL(graph::k_pad_diag, dim3(graph::grid_for(N - n, 64)), dim3(64), 0, st, (double *)W.H.p, N, n);
  HIP_TRY(hipGetLastError());
  out.solver.emplace(Solver{W, st, n_vertices, n_edges, m, n, N, (int)C.block_rc.size(), opt.robust_delta});
  if (sparse) out.solver->sp = &plan;
  return out.solver->objective(&out.F0);
}

// dvo_amd_optimize_graph: LM or dogleg from the given estimate; the free active vertices' poses are written back
int optimize(dvo_amd_context *ctx, const Problem &P, double *poses, const dvo_amd_graph_options &opt, double *edge_chi2,
             double *edge_weight, int capacity, dvo_amd_graph_iteration *iterations, dvo_amd_graph_stats &stats) {
  Unknowns U;
  const int refused = checked_unknowns(P, opt, U);
  stats.n_free = U.m;
  if (refused) return refused;
  Prepared R;
  GRAPH_TRY(prepare(ctx, P, opt, -1, std::move(U), R));
  Solver &S = *R.solver;
  GraphWorkspace &W = S.W;
  const hipStream_t st = S.st;
  const int n_vertices = P.n_vertices, n_edges = P.n_edges;
  double F = R.F0;
  stats.initial_objective = F;
  stats.termination = DVO_AMD_GRAPH_ITERATIONS_EXHAUSTED;
  stats.delta = opt.algorithm == DVO_AMD_GRAPH_DOGLEG ? opt.initial_delta : 0.0;
  stats.lambda = opt.algorithm == DVO_AMD_GRAPH_DOGLEG ? opt.initial_lambda : 0.0;
  if (S.m > 0) {
    if (opt.algorithm == DVO_AMD_GRAPH_LEVENBERG)
      GRAPH_TRY(run_levenberg(S, opt, &F, iterations, capacity, stats));
    else
      GRAPH_TRY(run_dogleg(S, opt, &F, iterations, capacity, stats));
  }
  stats.cholesky_failures = S.cholesky_failures;
  // the final estimate's per-edge chi2 / rho1, and F from the same evaluation
  double Ff = 0.0;
  GRAPH_TRY(S.objective(&Ff));
  stats.final_objective = Ff;
  if (edge_chi2 && n_edges) HIP_TRY(hipMemcpyAsync(edge_chi2, W.chi2.p, sizeof(double) * n_edges, hipMemcpyDeviceToHost, st));
  if (edge_weight && n_edges)
    HIP_TRY(hipMemcpyAsync(edge_weight, W.rho1.p, sizeof(double) * n_edges, hipMemcpyDeviceToHost, st));
  // only the free active vertices change: copy those back, the others stay the caller's bits
  std::vector<double> out(16 * (size_t)std::max(n_vertices, 1));
  if (n_vertices) HIP_TRY(hipMemcpyAsync(out.data(), W.poses.p, 16 * sizeof(double) * n_vertices, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int v : R.U.vertex_of) std::memcpy(poses + 16 * (size_t)v, out.data() + 16 * (size_t)v, 16 * sizeof(double));
  if (S.timed_lin) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, W.ev[0], W.ev[1]) == hipSuccess) W.lin_ms = ms;
    if (hipEventElapsedTime(&ms, W.ev[2], W.ev[3]) == hipSuccess) W.fac_ms = ms;
    if (S.sp) {
      W.sp_lin_ms = W.lin_ms;
      W.sp_fac_ms = W.fac_ms;
      if (hipEventElapsedTime(&ms, W.ev[3], W.ev[4]) == hipSuccess) W.sp_solve_ms = ms;
    }
  }
  return DVO_AMD_OK;
}

// the system at the given estimate and its undamped solve H x = b into x; *failed_pivot >= 0: H was not positive definite
int undamped_system(Solver &S, int *failed_pivot) {
  GRAPH_TRY(S.linearise());
  GRAPH_TRY(S.factor_solve_enqueue(false, 0.0, S.x()));
  return S.read(nullptr, 0, failed_pivot);
}

// dvo_amd_debug_graph_system and _sparse: the outputs of the first linear system (null: not wanted)
struct FirstSystem {
  double *H, *b, *x, *F;
  int *n_free, *failed_pivot;
  // the sparse entry: the stored blocks (row, col slots; 36 doubles each, row-major), capacity in / count out
  int *block_rc = nullptr;
  double *blocks = nullptr;
  int block_capacity = 0;
  int *n_blocks = nullptr;
};

int first_system(dvo_amd_context *ctx, const Problem &P, const dvo_amd_graph_options &opt, const FirstSystem &out) {
  Unknowns U;
  const int refused = checked_unknowns(P, opt, U);
  if (out.n_free) *out.n_free = U.m;
  if (refused) return refused;
  Prepared R;
  GRAPH_TRY(prepare(ctx, P, opt, -1, std::move(U), R));
  Solver &S = *R.solver;
  GraphWorkspace &W = S.W;
  const int n = S.n;
  if (out.F) *out.F = R.F0;
  if (S.m == 0) return DVO_AMD_OK;
  int f = -1;
  GRAPH_TRY(undamped_system(S, &f));
  if (out.failed_pivot) *out.failed_pivot = f;
  if (S.sp) {
    const std::vector<int2> &slot_rc = R.plan.slot_rc;
    const int nb = (int)slot_rc.size();
    if (out.n_blocks) *out.n_blocks = nb;
    if (out.block_rc && nb <= out.block_capacity)
      for (int k = 0; k < nb; ++k) out.block_rc[2 * k] = slot_rc[k].x, out.block_rc[2 * k + 1] = slot_rc[k].y;
    if (out.blocks && nb <= out.block_capacity)
      HIP_TRY(hipMemcpyAsync(out.blocks, W.Hs.p, sizeof(double) * 36 * nb, hipMemcpyDeviceToHost, S.st));
  } else if (out.H)
    HIP_TRY(hipMemcpy2DAsync(out.H, sizeof(double) * n, W.H.p, sizeof(double) * S.N, sizeof(double) * n, n,
                             hipMemcpyDeviceToHost, S.st));
  if (out.b) HIP_TRY(hipMemcpyAsync(out.b, W.b.p, sizeof(double) * n, hipMemcpyDeviceToHost, S.st));
  if (out.x) HIP_TRY(hipMemcpyAsync(out.x, W.x.p, sizeof(double) * n, hipMemcpyDeviceToHost, S.st));
  HIP_TRY(hipStreamSynchronize(S.st));
  return DVO_AMD_OK;
}

// dvo_amd_graph_marginals: the undamped factorization at the given estimate, then J's blocks of H^-1 (none if a pivot failed)
int marginals(dvo_amd_context *ctx, const Problem &P, const dvo_amd_graph_options &opt, Unknowns &&U, MargJob &J) {
  Prepared R;
  GRAPH_TRY(prepare(ctx, P, opt, J.n, std::move(U), R));
  if (R.U.m == 0) return DVO_AMD_OK;
  GRAPH_TRY(undamped_system(*R.solver, &J.failed_pivot));
  if (J.failed_pivot >= 0) return DVO_AMD_OK;
  return marginals_stage(R, J);
}

}  // namespace

void graph_workspace_release(dvo_amd_context *ctx) {
  GraphWorkspace *w = ctx->graph_ws;
  if (!w) return;
  w->each_buf([](DeviceBuf &b) {
    if (b.p) (void)hipFree(b.p);
  });
  for (hipEvent_t e : w->ev)
    if (e) (void)hipEventDestroy(e);
  delete w;
  ctx->graph_ws = nullptr;
}

}  // namespace host
}  // namespace dvo_amd

extern "C" {

void dvo_amd_default_graph_options(int algorithm, dvo_amd_graph_options *opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof(*opt));
  opt->algorithm = algorithm;
  opt->robust_delta = 5.0;  // createRobustKernel: RobustKernelCauchy, delta 5 (keyframe_graph.cpp:840-852)
  if (algorithm == DVO_AMD_GRAPH_DOGLEG) {
    opt->max_iterations = 100;
    opt->max_trials = 100;
    opt->initial_lambda = 1e-7;
    opt->initial_delta = 1e4;
  } else {
    opt->max_iterations = 50;  // LocalMap::optimize (local_map.cpp:205-210)
    opt->max_trials = 10;
    opt->initial_lambda = 0.0;
    opt->initial_delta = 0.0;
  }
}

int dvo_amd_optimize_graph(dvo_amd_context *ctx, int n_vertices, double *poses, const int *fixed, int n_edges,
                           const dvo_amd_graph_edge *edges, const dvo_amd_graph_options *opt, double *edge_chi2,
                           double *edge_weight, int iteration_capacity, dvo_amd_graph_iteration *iterations,
                           dvo_amd_graph_stats *stats) {
  dvo_amd_graph_stats local;
  dvo_amd_graph_stats &s = stats ? *stats : local;
  std::memset(&s, 0, sizeof(s));
  int rc = host::graph_check_arguments("dvo_amd_optimize_graph", n_vertices, poses, n_edges, edges, opt);
  if (rc) return rc;
  rc = host::have_device();
  if (rc) return rc;
  if (!ctx || iteration_capacity < 0 || (iteration_capacity > 0 && !iterations)) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = queue_must_be_idle(ctx, "dvo_amd_optimize_graph");
  if (rc) return rc;
  const host::Problem P{"dvo_amd_optimize_graph", n_vertices, poses, fixed, n_edges, edges};
  return host::optimize(ctx, P, poses, *opt, edge_chi2, edge_weight, iteration_capacity, iterations, s);
}

int dvo_amd_graph_marginals(dvo_amd_context *ctx, int n_vertices, const double *poses, const int *fixed, int n_edges,
                            const dvo_amd_graph_edge *edges, const dvo_amd_graph_options *opt, int n_blocks, const int *block_a,
                            const int *block_b, double *blocks, dvo_amd_graph_marginal_stats *stats) {
  dvo_amd_graph_marginal_stats local;
  dvo_amd_graph_marginal_stats &s = stats ? *stats : local;
  std::memset(&s, 0, sizeof(s));
  int rc = host::graph_check_arguments("dvo_amd_graph_marginals", n_vertices, poses, n_edges, edges, opt);
  if (rc) return rc;
  auto bad = [](const std::string &why) {
    g_last_error = "dvo_amd_graph_marginals: " + why;
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  };
  if (n_blocks < 0) return bad("n_blocks < 0");
  if (n_blocks > 0 && (!block_a || !block_b || !blocks)) return bad("null block_a, block_b or blocks");
  for (int k = 0; k < n_blocks; ++k)
    if (block_a[k] < 0 || block_a[k] >= n_vertices || block_b[k] < 0 || block_b[k] >= n_vertices)
      return bad("vertex index out of range (block " + std::to_string(k) + ")");
  const host::Problem P{"dvo_amd_graph_marginals", n_vertices, poses, fixed, n_edges, edges};
  host::Unknowns U;
  rc = host::checked_unknowns(P, *opt, U);  // before the device is asked for: a graph beyond the capacity is refused anywhere
  if (rc) return rc;
  rc = host::have_device();
  if (rc) return rc;
  if (!ctx) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = queue_must_be_idle(ctx, "dvo_amd_graph_marginals");
  if (rc) return rc;
  // blocks that touch a fixed vertex are zeros, else those that touch an inactive one (no slot) NaN; the others go to the device
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int> kind(std::max(n_blocks, 1), 0), qa, qb, at;
  int n_fixed = 0, n_inactive = 0;
  for (int k = 0; k < n_blocks; ++k) {
    const int a = block_a[k], b = block_b[k];
    if (fixed && (fixed[a] || fixed[b])) {
      kind[k] = 1, ++n_fixed;
    } else if (U.slot[a] < 0 || U.slot[b] < 0) {
      kind[k] = 2, ++n_inactive;
    } else {
      qa.push_back(a), qb.push_back(b), at.push_back(k);
    }
  }
  std::vector<double> out(36 * std::max<size_t>(qa.size(), 1), nan);
  host::MargJob job;
  job.n = (int)qa.size();
  job.a = qa.data();
  job.b = qb.data();
  job.out = out.data();
  const int n_free = U.m;
  rc = host::marginals(ctx, P, *opt, std::move(U), job);
  if (rc) return rc;
  const bool ok = job.failed_pivot < 0;
  for (int k = 0; k < n_blocks; ++k)
    for (int e = 0; e < 36; ++e) blocks[36 * (size_t)k + e] = kind[k] == 1 ? 0.0 : nan;
  if (ok)
    for (size_t i = 0; i < at.size(); ++i) std::memcpy(blocks + 36 * (size_t)at[i], out.data() + 36 * i, 36 * sizeof(double));
  s.n_free = n_free;
  s.factorized = ok ? 1 : 0;
  s.fixed_blocks = n_fixed;
  s.inactive_blocks = n_inactive;
  s.solved_columns = ok ? job.solved_columns : 0;
  return DVO_AMD_OK;
}

// both first-system entries: dogleg's defaults with the given robust_delta and solver; their refusals carry the optimizer's name
static int debug_first_system(dvo_amd_context *ctx, const char *entry, int n_vertices, const double *poses, const int *fixed,
                              int n_edges, const dvo_amd_graph_edge *edges, double robust_delta, int solver,
                              const host::FirstSystem &out) {
  dvo_amd_graph_options opt;
  dvo_amd_default_graph_options(DVO_AMD_GRAPH_DOGLEG, &opt);
  opt.robust_delta = robust_delta;
  opt.solver = solver;
  const host::Problem P{"dvo_amd_optimize_graph", n_vertices, poses, fixed, n_edges, edges};
  int rc = host::graph_check_arguments(P.entry, n_vertices, poses, n_edges, edges, &opt);
  if (rc) return rc;
  if (out.block_capacity < 0) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = host::have_device();
  if (rc) return rc;
  if (!ctx) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = queue_must_be_idle(ctx, entry);
  if (rc) return rc;
  return host::first_system(ctx, P, opt, out);
}

int dvo_amd_debug_graph_system(dvo_amd_context *ctx, int n_vertices, const double *poses, const int *fixed, int n_edges,
                               const dvo_amd_graph_edge *edges, double robust_delta, double *H, double *b, double *x,
                               double *F, int *n_free, int *failed_pivot) {
  return debug_first_system(ctx, "dvo_amd_debug_graph_system", n_vertices, poses, fixed, n_edges, edges, robust_delta,
                            DVO_AMD_GRAPH_SOLVER_DENSE, host::FirstSystem{H, b, x, F, n_free, failed_pivot});
}

int dvo_amd_debug_graph_system_sparse(dvo_amd_context *ctx, int n_vertices, const double *poses, const int *fixed,
                                      int n_edges, const dvo_amd_graph_edge *edges, double robust_delta, int block_capacity,
                                      int *n_blocks, int *block_rc, double *blocks, double *b, double *x, double *F,
                                      int *n_free, int *failed_pivot) {
  int nb = 0;
  const host::FirstSystem out{nullptr, b, x, F, n_free, failed_pivot, block_rc, blocks, block_capacity, &nb};
  const int rc = debug_first_system(ctx, "dvo_amd_debug_graph_system_sparse", n_vertices, poses, fixed, n_edges, edges,
                                    robust_delta, DVO_AMD_GRAPH_SOLVER_SPARSE, out);
  if (n_blocks) *n_blocks = nb;
  if (!rc && nb > block_capacity && (block_rc || blocks)) return DVO_AMD_ERR_CAPACITY;
  return rc;
}

int dvo_amd_debug_graph_symbolic(int n_vertices, const int *fixed, int n_edges, const dvo_amd_graph_edge *edges,
                                 int capacity, int *n_free, int *n_fronts, int *n_update, int *n_levels, int *widest,
                                 int *perm, int *parent, int *level, int *pivot_ptr, int *pivot, int *update_ptr, int *update,
                                 double *factor_doubles, double *flops) {
  if (n_vertices < 0 || n_edges < 0 || capacity < 0 || (n_edges > 0 && !edges)) return DVO_AMD_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n_edges; ++k)
    if (edges[k].from < 0 || edges[k].from >= n_vertices || edges[k].to < 0 || edges[k].to >= n_vertices ||
        edges[k].from == edges[k].to)
      return DVO_AMD_ERR_INVALID_ARGUMENT;
  const host::Unknowns U = host::free_unknowns(n_vertices, fixed, n_edges, edges);
  const int m = U.m;
  if (n_free) *n_free = m;
  if (m > DVO_AMD_GRAPH_MAX_FREE_VERTICES_SPARSE) return DVO_AMD_ERR_CAPACITY;
  const host::Symbolic S = host::symbolic(host::block_adjacency(m, U.slot, n_edges, edges));
  const int nf = S.n_fronts, nu = (int)S.upd.size();
  if (n_fronts) *n_fronts = nf;
  if (n_update) *n_update = nu;
  if (n_levels) *n_levels = S.n_levels;
  if (widest) *widest = S.widest;
  if (factor_doubles) *factor_doubles = S.factor_doubles;
  if (flops) *flops = S.flops;
  if (std::max(std::max(m, nf + 1), nu) > capacity) return DVO_AMD_ERR_CAPACITY;
  auto put = [](int *dst, const std::vector<int> &src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), sizeof(int) * src.size());
  };
  put(perm, S.perm);
  put(parent, S.parent);
  put(level, S.level);
  put(pivot_ptr, S.piv_ptr);
  put(pivot, S.piv);
  put(update_ptr, S.upd_ptr);
  put(update, S.upd);
  return DVO_AMD_OK;
}

int dvo_amd_debug_graph_sparse_timing(dvo_amd_context *ctx, double *symbolic_ms, double *linearise_ms, double *factorize_ms,
                                      double *solve_ms, int *fronts, int *levels, int *widest, double *factor_doubles,
                                      double *flops) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!ctx) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const host::GraphWorkspace *W = ctx->graph_ws;
  if (symbolic_ms) *symbolic_ms = W ? W->sp_symbolic_ms : 0.0;
  if (linearise_ms) *linearise_ms = W ? W->sp_lin_ms : 0.0;
  if (factorize_ms) *factorize_ms = W ? W->sp_fac_ms : 0.0;
  if (solve_ms) *solve_ms = W ? W->sp_solve_ms : 0.0;
  if (fronts) *fronts = W ? W->sp_fronts : 0;
  if (levels) *levels = W ? W->sp_levels : 0;
  if (widest) *widest = W ? W->sp_widest : 0;
  if (factor_doubles) *factor_doubles = W ? W->sp_factor_doubles : 0.0;
  if (flops) *flops = W ? W->sp_flops : 0.0;
  return DVO_AMD_OK;
}

int dvo_amd_debug_graph_timing(dvo_amd_context *ctx, double *linearise_ms, double *factorize_ms, int *n_padded,
                               int *factorizations) {
  int rc = host::have_device();
  if (rc) return rc;
  if (!ctx) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const host::GraphWorkspace *W = ctx->graph_ws;
  if (linearise_ms) *linearise_ms = W ? W->lin_ms : 0.0;
  if (factorize_ms) *factorize_ms = W ? W->fac_ms : 0.0;
  if (n_padded) *n_padded = W ? W->n_padded : 0;
  if (factorizations) *factorizations = W ? W->factorizations : 0;
  return DVO_AMD_OK;
}

}  // extern "C"
