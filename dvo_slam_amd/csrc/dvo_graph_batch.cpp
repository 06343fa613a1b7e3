// Many small pose graphs in one call (dvo_amd.h: dvo_amd_optimize_graphs_batch), fp64 throughout.
//   k_optimize_batch   one workgroup (256 threads) per graph, blockIdx.x = graph; the whole optimization -- linearise, assemble,
//                      damp, factor, solve, apply, evaluate, accept or reject, next iteration -- runs inside this one launch.
//                      Workgroups never talk to each other: a graph that finishes early simply exits.
// Where things live, per graph (n = 6m unknowns, m <= 32 free active vertices):
//   H        lower triangle, packed by rows (entry (r, c), c <= r, at r (r + 1) / 2 + c), undamped, in the context's global
//            scratch (at most 148 KB a graph: it stays in L2); blocks no edge touches are zero from the call's memset
//   L        the working copy H (+ lambda I) and then its Cholesky factor, packed the same way, in LDS; the launch declares
//            n_max (n_max + 1) / 2 doubles of dynamic LDS for the largest graph of the batch: 32 KB a workgroup for a batch
//            of 15-vertex local maps, 145 KB only for a batch that holds a 32-vertex graph.  (The registers of the edge
//            linearisation, 448 of 512, hold the kernel to one workgroup a CU either way: 256 graphs run side by side.)
//   b, x, h_sd, h_dl, aux   LDS, 192 doubles each
//   poses, the saved estimate, the edge records of the linearisation, chi2 / rho1 per edge   global, at the graph's offset
// Summation order (fixed; results are a function of the graph and the options alone, not of the batch around it):
//   H, b     contributors in edge order, as dvo_graph.cpp's k_assemble_H / k_assemble_b (the blocks are the same bits)
//   factor   right-looking by vertex (6 columns): thread 0 factors the 6 x 6 diagonal block column by column; every row below
//            solves its 6 entries against it (column 0 to 5); every trailing entry subtracts its 6 products in column order
//   solve    forward by vertex: thread 0 solves the 6 unknowns of the block (each subtracts the earlier ones in order, then
//            divides), every later row subtracts its 6 products in column order; backward the mirror image (the block's
//            unknowns from the last to the first, each subtracting the later ones in increasing order)
//   sums     F over edges and the dot products: thread t adds its terms t, t + 256, ... in order, a butterfly over the wave
//            (xor 32, 16, 8, 4, 2, 1), then ((w0 + w1) + w2) + w3 over the four waves
//   H v      one wave per row: lane l adds columns l, l + 64, l + 128 in order, then the same butterfly
// No floating-point atomics, no communication between workgroups.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dvo_graph_device.h"
#include "dvo_graph_host.h"

namespace dvo_amd {
namespace graph_batch {

using namespace ::dvo_amd::graph;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxN = 6 * DVO_AMD_GRAPH_BATCH_MAX_FREE_VERTICES;
constexpr int kMaxRecords = 256;  // iteration records kept per graph for dvo_amd_debug_graph_batch_records

struct Item {
  long long h_off;  // packed H, in doubles
  int n_vertices, n_edges, m, nblocks;
  int pose_off;     // vertices before this graph
  int edge_off;     // edges before this graph
  int slot_off;     // free slots before this graph (vertex_of)
  int block_off;    // lower blocks before this graph (block_rc)
  int bptr_off;     // this graph's nblocks + 1 entries of block_ptr (absolute positions in block_c)
  int gptr_off;     // this graph's m + 1 entries of b_ptr (absolute positions in b_c)
};

struct Out {
  double initial_objective, final_objective, lambda, delta;
  int iterations, termination, cholesky_failures, reserved;
};

struct Params {
  int algorithm, max_iterations, max_trials, record_stride;
  double robust_delta, initial_lambda, initial_delta;
};

struct Buffers {
  const Item *items;
  const dvo_amd_graph_edge *edges;
  double *poses, *saved, *rec, *chi2, *rho1, *H;
  const int2 *block_rc;
  const int *block_ptr, *block_c, *b_ptr, *b_c, *vertex_of;
  Out *out;
  dvo_amd_graph_iteration *records;
};

// one workgroup's view of its graph
struct G {
  int tid, lane, wave;
  int n_edges, m, n, nblocks;
  double delta;
  const dvo_amd_graph_edge *edges;
  double *poses, *saved, *rec, *chi2, *rho1, *H;
  const int2 *block_rc;
  const int *block_ptr, *block_c, *b_ptr, *b_c, *vertex_of;
  double *L, *b, *x, *hsd, *hdl, *aux, *red;  // LDS
  int *fail;                                  // LDS
};

__device__ inline int tri(int r) { return r * (r + 1) / 2; }

// K sums at once, the total in every thread.  The leading barrier also orders what the callers wrote before it.
template <int K>
__device__ inline void block_sums(const G &g, double (&v)[K]) {
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  __syncthreads();
  if (g.lane == 0)
    for (int k = 0; k < K; ++k) g.red[k * kWaves + g.wave] = v[k];
  __syncthreads();
  for (int k = 0; k < K; ++k)
    v[k] = ((g.red[k * kWaves + 0] + g.red[k * kWaves + 1]) + g.red[k * kWaves + 2]) + g.red[k * kWaves + 3];
}

__device__ inline double block_max(const G &g, double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __syncthreads();
  if (g.lane == 0) g.red[g.wave] = v;
  __syncthreads();
  return fmax(fmax(g.red[0], g.red[1]), fmax(g.red[2], g.red[3]));
}

// F at the current estimate; chi2 and rho1 per edge
__device__ inline double objective(const G &g) {
  double s[1] = {0.0};
  for (int k = g.tid; k < g.n_edges; k += kThreads) {
    EdgeEval v;
    eval_edge(g.edges[k], g.poses, v);
    double r0, r1;
    robust(v.chi2, g.delta, &r0, &r1);
    g.chi2[k] = v.chi2;
    g.rho1[k] = r1;
    s[0] += r0;
  }
  block_sums<1>(g, s);
  return s[0];
}

// the edge records, then the lower blocks of H (global, packed) and b (LDS), contributors in edge order
__device__ inline void linearise_assemble(const G &g) {
  for (int k = g.tid; k < g.n_edges; k += kThreads)
    linearise_edge(g.edges[k], g.poses, g.delta, g.rec + (size_t)k * kRecord);
  __syncthreads();
  for (int e = g.tid; e < g.nblocks * 36; e += kThreads) {
    const int blk = e / 36, r = (e % 36) / 6, c = e % 6;
    const int2 rc = g.block_rc[blk];
    if (rc.x == rc.y && c > r) continue;
    double s = 0.0;
    for (int p = g.block_ptr[blk]; p < g.block_ptr[blk + 1]; ++p) {
      const int code = g.block_c[p], kind = code & 3;
      const double *o = g.rec + (size_t)(code >> 2) * kRecord;
      const double v = kind == 0 ? o[kAff + r * 6 + c] : kind == 1 ? o[kAtt + r * 6 + c] : kind == 2 ? o[kAft + r * 6 + c]
                                                                                                     : o[kAft + c * 6 + r];
      s += v;
    }
    g.H[tri(6 * rc.x + r) + 6 * rc.y + c] = s;
  }
  for (int i = g.tid; i < g.n; i += kThreads) {
    const int slot = i / 6, r = i % 6;
    double s = 0.0;
    for (int p = g.b_ptr[slot]; p < g.b_ptr[slot + 1]; ++p) {
      const int code = g.b_c[p];
      s += g.rec[(size_t)(code >> 1) * kRecord + ((code & 1) ? kGt : kGf) + r];
    }
    g.b[i] = s;
  }
  __syncthreads();
}

__device__ inline double max_diag(const G &g) {
  double m = 0.0;
  for (int i = g.tid; i < g.n; i += kThreads) m = fmax(m, fabs(g.H[tri(i) + i]));
  return block_max(g, m);
}

// L = chol(H + lambda I) (damp) or chol(H) in LDS; false when a pivot is <= 0 or NaN (block-uniform)
__device__ inline bool factor(const G &g, bool damp, double lambda) {
  const int n = g.n, total = tri(n);
  double *L = g.L;
  __syncthreads();  // everyone is done with the last factor and its failure word
  for (int e = g.tid; e < total; e += kThreads) L[e] = g.H[e];
  if (g.tid == 0) *g.fail = -1;
  __syncthreads();
  if (damp)
    for (int i = g.tid; i < n; i += kThreads) L[tri(i) + i] = L[tri(i) + i] + lambda;
  __syncthreads();
  for (int j0 = 0; j0 < n; j0 += 6) {
    if (g.tid == 0) {  // the 6 x 6 diagonal block, right-looking, in registers
      double a[6][6];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) a[r][c] = L[tri(j0 + r) + j0 + c];
      int bad = -1;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const double piv = a[q][q];
        if (bad < 0 && !(piv > 0.0)) bad = j0 + q;
        const double d = sqrt(piv);
        a[q][q] = d;
#pragma unroll
        for (int r = q + 1; r < 6; ++r) a[r][q] = a[r][q] / d;
#pragma unroll
        for (int c = q + 1; c < 6; ++c)
#pragma unroll
          for (int r = c; r < 6; ++r) a[r][c] = a[r][c] - a[r][q] * a[c][q];
      }
      if (bad >= 0) {
        *g.fail = bad;
      } else {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c <= r; ++c) L[tri(j0 + r) + j0 + c] = a[r][c];
      }
    }
    __syncthreads();
    if (*g.fail >= 0) return false;
    const int j1 = j0 + 6;
    if (j1 >= n) break;
    for (int r = j1 + g.tid; r < n; r += kThreads) {  // the rows below: X L11^T = A21, one row a thread
      double *row = L + tri(r) + j0;
      double a[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) a[q] = row[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        a[q] = a[q] / L[tri(j0 + q) + j0 + q];
#pragma unroll
        for (int c = q + 1; c < 6; ++c) a[c] = a[c] - a[q] * L[tri(j0 + c) + j0 + q];
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) row[q] = a[q];
    }
    __syncthreads();
    // the trailing lower triangle: entry (rr, cc) of it is element e = tri(rr) + cc; thread t owns e = t, t + 256, ...
    const int rem = n - j1, count = tri(rem);
    int rr = 0, cc = g.tid;
    while (cc > rr) cc -= rr + 1, ++rr;
    for (int e = g.tid; e < count; e += kThreads) {
      const double *lr = L + tri(j1 + rr) + j0, *lc = L + tri(j1 + cc) + j0;
      double v = L[tri(j1 + rr) + j1 + cc];
#pragma unroll
      for (int q = 0; q < 6; ++q) v = v - lr[q] * lc[q];
      L[tri(j1 + rr) + j1 + cc] = v;
      cc += kThreads;
      while (cc > rr) cc -= rr + 1, ++rr;
    }
    __syncthreads();
  }
  return true;
}

// L y = b, L^T x = y; the result in `out` (LDS)
__device__ inline void solve(const G &g, double *out) {
  const int n = g.n;
  const double *L = g.L;
  for (int i = g.tid; i < n; i += kThreads) out[i] = g.b[i];
  __syncthreads();
  for (int j0 = 0; j0 < n; j0 += 6) {  // forward
    if (g.tid == 0) {
      for (int q = 0; q < 6; ++q) {
        double s = out[j0 + q];
        for (int p = 0; p < q; ++p) s = s - L[tri(j0 + q) + j0 + p] * out[j0 + p];
        out[j0 + q] = s / L[tri(j0 + q) + j0 + q];
      }
    }
    __syncthreads();
    for (int r = j0 + 6 + g.tid; r < n; r += kThreads) {
      double s = out[r];
      for (int q = 0; q < 6; ++q) s = s - L[tri(r) + j0 + q] * out[j0 + q];
      out[r] = s;
    }
    __syncthreads();
  }
  for (int j0 = n - 6; j0 >= 0; j0 -= 6) {  // backward
    if (g.tid == 0) {
      for (int q = 5; q >= 0; --q) {
        double s = out[j0 + q];
        for (int p = q + 1; p < 6; ++p) s = s - L[tri(j0 + p) + j0 + q] * out[j0 + p];
        out[j0 + q] = s / L[tri(j0 + q) + j0 + q];
      }
    }
    __syncthreads();
    for (int i = g.tid; i < j0; i += kThreads) {
      double s = out[i];
      for (int q = 0; q < 6; ++q) s = s - L[tri(j0 + q) + i] * out[j0 + q];
      out[i] = s;
    }
    __syncthreads();
  }
}

// y = H v (both in LDS) from the packed lower triangle
__device__ inline void matvec(const G &g, const double *v, double *y) {
  for (int row = g.wave; row < g.n; row += kWaves) {
    double s = 0.0;
    for (int c = g.lane; c < g.n; c += 64) {
      const double h = c <= row ? g.H[tri(row) + c] : g.H[tri(c) + row];
      s += h * v[c];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (g.lane == 0) y[row] = s;
  }
  __syncthreads();
}

// the free vertices' poses: save / restore / X <- X * inc(step)
__device__ inline void push(const G &g) {
  for (int e = g.tid; e < 16 * g.m; e += kThreads) {
    const int at = 16 * g.vertex_of[e / 16] + e % 16;
    g.saved[at] = g.poses[at];
  }
  __syncthreads();
}
__device__ inline void pop(const G &g) {
  for (int e = g.tid; e < 16 * g.m; e += kThreads) {
    const int at = 16 * g.vertex_of[e / 16] + e % 16;
    g.poses[at] = g.saved[at];
  }
  __syncthreads();
}
__device__ inline void update(const G &g, const double *step) {
  for (int s = g.tid; s < g.m; s += kThreads) apply_increment(g.poses + 16 * (size_t)g.vertex_of[s], step + 6 * s);
  __syncthreads();
}

__device__ inline void record(const G &g, dvo_amd_graph_iteration *records, int stride, int it, double F, double step,
                              double lambda, double delta, int trials, int accepted) {
  if (g.tid != 0 || it >= stride) return;
  dvo_amd_graph_iteration &r = records[it];
  r.objective = F;
  r.step_norm = step;
  r.lambda = lambda;
  r.delta = delta;
  r.trials = trials;
  r.accepted = accepted;
}

// Every scalar below (F, lambda, nu, Delta, rho, the counters) is computed by every thread from block-wide sums that are the
// same bits in every thread, so all control flow is uniform across the workgroup and every barrier is reached by all of it.
__global__ void __launch_bounds__(kThreads) k_optimize_batch(Buffers B, Params P) {
  extern __shared__ double lds_factor[];
  __shared__ double lds_vec[5][kMaxN];
  __shared__ double lds_red[4 * kWaves];
  __shared__ int lds_fail;
  const Item I = B.items[blockIdx.x];
  G g;
  g.tid = threadIdx.x;
  g.lane = threadIdx.x % 64;
  g.wave = threadIdx.x / 64;
  g.n_edges = I.n_edges;
  g.m = I.m;
  g.n = 6 * I.m;
  g.nblocks = I.nblocks;
  g.delta = P.robust_delta;
  g.edges = B.edges + I.edge_off;
  g.poses = B.poses + 16 * (size_t)I.pose_off;
  g.saved = B.saved + 16 * (size_t)I.pose_off;
  g.rec = B.rec + (size_t)I.edge_off * kRecord;
  g.chi2 = B.chi2 + I.edge_off;
  g.rho1 = B.rho1 + I.edge_off;
  g.H = B.H + I.h_off;
  g.block_rc = B.block_rc + I.block_off;
  g.block_ptr = B.block_ptr + I.bptr_off;
  g.block_c = B.block_c;
  g.b_ptr = B.b_ptr + I.gptr_off;
  g.b_c = B.b_c;
  g.vertex_of = B.vertex_of + I.slot_off;
  g.L = lds_factor;
  g.b = lds_vec[0];
  g.x = lds_vec[1];
  g.hsd = lds_vec[2];
  g.hdl = lds_vec[3];
  g.aux = lds_vec[4];
  g.red = lds_red;
  g.fail = &lds_fail;
  dvo_amd_graph_iteration *records = B.records + (size_t)blockIdx.x * P.record_stride;
  const int n = g.n;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);

  double F = objective(g);
  const double F0 = F;
  const bool dogleg = P.algorithm == DVO_AMD_GRAPH_DOGLEG;
  int iterations = 0, termination = DVO_AMD_GRAPH_ITERATIONS_EXHAUSTED, failures = 0;
  double lambda = dogleg ? P.initial_lambda : 0.0, Delta = dogleg ? P.initial_delta : 0.0;

  if (g.m > 0 && !dogleg) {  // OptimizationAlgorithmLevenberg::solve, max_iterations times
    double nu = 2.0;
    for (int it = 0; it < P.max_iterations; ++it) {
      linearise_assemble(g);
      if (it == 0) {
        lambda = P.initial_lambda > 0.0 ? P.initial_lambda : 1e-5 * max_diag(g);
        nu = 2.0;
      }
      int trials = 0, accepted = 0;
      double rho = 0.0, step = 0.0;
      bool stop = false;
      do {
        push(g);
        const bool ok = factor(g, true, lambda);
        double Fp = inf;
        double s[2] = {0.0, 0.0};
        if (ok) {
          solve(g, g.x);
          update(g, g.x);
          Fp = objective(g);
          for (int i = g.tid; i < n; i += kThreads) {
            s[0] += g.x[i] * (lambda * g.x[i] + g.b[i]);
            s[1] += g.x[i] * g.x[i];
          }
          block_sums<2>(g, s);
        } else {
          ++failures;
        }
        rho = ok ? (F - Fp) / (s[0] + 1e-3) : -inf;
        if (rho > 0.0 && isfinite(Fp)) {
          const double t = 2.0 * rho - 1.0;
          const double alpha = fmin(1.0 - t * t * t, 2.0 / 3.0);
          lambda *= fmax(1.0 / 3.0, alpha);
          nu = 2.0;
          F = Fp;
          step = sqrt(s[1]);
          accepted = 1;
        } else {
          lambda *= nu;
          nu *= 2.0;
          if (ok) pop(g);
          if (!isfinite(lambda)) {  // before the attempt is counted
            stop = true;
            break;
          }
        }
        ++trials;
      } while (rho < 0.0 && trials < P.max_trials);
      record(g, records, P.record_stride, it, F, step, lambda, 0.0, trials, accepted);
      iterations = it + 1;
      if (stop || trials == P.max_trials || rho == 0.0 || !isfinite(lambda)) {
        termination = DVO_AMD_GRAPH_TERMINATE;
        break;
      }
    }
  } else if (g.m > 0) {  // OptimizationAlgorithmDogleg::solve, max_iterations times
    bool was_pd = true, failed = false;
    for (int it = 0; it < P.max_iterations && !failed; ++it) {
      linearise_assemble(g);
      matvec(g, g.b, g.aux);
      double s[3] = {0.0, 0.0, 0.0}, d[2] = {0.0, 0.0};
      for (int i = g.tid; i < n; i += kThreads) {
        d[0] += g.b[i] * g.b[i];
        d[1] += g.aux[i] * g.b[i];
      }
      block_sums<2>(g, d);
      const double alpha = d[0] / d[1];
      double q[1] = {0.0};
      for (int i = g.tid; i < n; i += kThreads) {
        const double h = alpha * g.b[i];
        g.hsd[i] = h;
        q[0] += h * h;
      }
      block_sums<1>(g, q);
      const double hsd_sq = q[0], hsd_norm = sqrt(hsd_sq);
      double hgn_norm = -1.0, step = 0.0;
      bool solved_gn = false, good = false;
      int trials = 0;
      do {
        ++trials;
        if (!solved_gn) {
          solved_gn = true;
          bool ok = false;
          while (!ok) {
            ok = factor(g, !was_pd, lambda);
            q[0] = 0.0;
            if (ok) {
              solve(g, g.x);
              for (int i = g.tid; i < n; i += kThreads) q[0] += g.x[i] * g.x[i];
              block_sums<1>(g, q);
            } else {
              ++failures;
            }
            was_pd = was_pd && ok;
            if (!was_pd) {
              if (ok) {
                lambda = fmax(1e-12, lambda / (0.5 * 10.0));
              } else {
                lambda *= 10.0;
                if (lambda > 1e3) {
                  lambda = 1e3;
                  failed = true;
                  break;
                }
              }
            }
          }
          if (failed) break;
          hgn_norm = sqrt(q[0]);
        }
        if (hgn_norm < Delta) {
          for (int i = g.tid; i < n; i += kThreads) g.hdl[i] = g.x[i];
        } else if (hsd_norm > Delta) {
          const double a = Delta / hsd_norm;
          for (int i = g.tid; i < n; i += kThreads) g.hdl[i] = a * g.hsd[i];
        } else {
          d[0] = d[1] = 0.0;
          for (int i = g.tid; i < n; i += kThreads) {
            const double a = g.x[i] - g.hsd[i];  // h_gn - h_sd
            g.aux[i] = a;
            d[0] += g.hsd[i] * a;
            d[1] += a * a;
          }
          block_sums<2>(g, d);
          const double c = d[0], bma = d[1];
          double beta;
          if (c <= 0.0)
            beta = (-c + sqrt(c * c + bma * (Delta * Delta - hsd_sq))) / bma;
          else
            beta = (Delta * Delta - hsd_sq) / (c + sqrt(c * c + bma * (Delta * Delta - hsd_sq)));
          for (int i = g.tid; i < n; i += kThreads) g.hdl[i] = g.hsd[i] + beta * (g.x[i] - g.hsd[i]);
        }
        __syncthreads();
        // linear gain 2 b^T h - h^T H h; then the trial
        matvec(g, g.hdl, g.aux);
        push(g);
        update(g, g.hdl);
        const double Fp = objective(g);
        s[0] = s[1] = s[2] = 0.0;
        for (int i = g.tid; i < n; i += kThreads) {
          s[0] += g.aux[i] * g.hdl[i];
          s[1] += g.b[i] * g.hdl[i];
          s[2] += g.hdl[i] * g.hdl[i];
        }
        block_sums<3>(g, s);
        double gain = -1.0 * s[0] + 2.0 * s[1];
        const double hdl_norm = sqrt(s[2]);
        if (fabs(gain) < 1e-12) gain = 1e-12;
        const double rho = (F - Fp) / gain;
        if (rho > 0.0) {
          good = true;
          F = Fp;
          step = hdl_norm;
        } else {
          pop(g);
        }
        if (rho > 0.75)
          Delta = fmax(Delta, 3.0 * hdl_norm);
        else if (rho < 0.25)
          Delta *= 0.5;
      } while (!good && trials < P.max_trials);
      iterations = it + 1;
      if (failed) {
        record(g, records, P.record_stride, it, F, 0.0, lambda, Delta, trials, 0);
        termination = DVO_AMD_GRAPH_FAIL;
        break;
      }
      record(g, records, P.record_stride, it, F, step, lambda, Delta, trials, good ? 1 : 0);
      if (trials == P.max_trials || !good) {
        termination = DVO_AMD_GRAPH_TERMINATE;
        break;
      }
    }
  }
  // chi2 / rho1 per edge at the final estimate, and F from the same evaluation
  const double Ff = objective(g);
  if (g.tid == 0) {
    Out &o = B.out[blockIdx.x];
    o.initial_objective = F0;
    o.final_objective = Ff;
    o.lambda = lambda;
    o.delta = Delta;
    o.iterations = iterations;
    o.termination = termination;
    o.cholesky_failures = failures;
    o.reserved = 0;
  }
}

}  // namespace graph_batch

namespace host {

#define GRAPH_BATCH_BUFS(X) \
  X(items) X(edges) X(poses) X(saved) X(rec) X(chi2) X(rho1) X(H) X(block_rc) X(block_ptr) X(block_c) X(b_ptr) X(b_c) \
  X(vertex_of) X(out) X(records)

struct GraphBatchWorkspace {
  DEVICE_BUF_MEMBERS(GRAPH_BATCH_BUFS)
  // the last call, for dvo_amd_debug_graph_batch_records
  int last_graphs = 0, last_stride = 0;
  std::vector<int> last_iterations;
  size_t lds_allowed = 0;  // the dynamic LDS the kernel has been allowed so far
};

namespace {

const char *const kEntry = "dvo_amd_optimize_graphs_batch";

int grow(DeviceBuf &b, size_t bytes) { return grow(b, bytes, kGraphBufStep, "graph batch workspace"); }

int optimize_batch(dvo_amd_context *ctx, int n_graphs, dvo_amd_graph_batch_item *items, const dvo_amd_graph_options &opt) {
  // per graph: the unknowns and the contributor lists (CSR by lower block / by vertex slot, contributors in edge order)
  std::vector<graph_batch::Item> its(n_graphs);
  std::vector<int2> block_rc;
  std::vector<int> block_ptr, block_c, b_ptr, b_c, vertex_of_all;
  size_t n_vertices = 0, n_edges = 0;
  long long h_doubles = 0;
  int n_max = 0;
  for (int g = 0; g < n_graphs; ++g) {
    dvo_amd_graph_batch_item &it = items[g];
    const Unknowns U = free_unknowns(it.n_vertices, it.fixed, it.n_edges, it.edges);
    const Contributors C = contributor_lists(U, it.n_edges, it.edges, true);
    const int m = U.m;
    // h_off, n_vertices, n_edges, m, nblocks, then what lies before this graph: pose, edge, slot, block, bptr, gptr offsets
    its[g] = graph_batch::Item{h_doubles, it.n_vertices, it.n_edges, m, (int)C.block_rc.size(), (int)n_vertices, (int)n_edges,
                               (int)vertex_of_all.size(), (int)block_rc.size(), (int)block_ptr.size(), (int)b_ptr.size()};
    // the graph's pointers index the concatenated contributor arrays
    for (int p : C.block_ptr) block_ptr.push_back((int)block_c.size() + p);
    for (int p : C.b_ptr) b_ptr.push_back((int)b_c.size() + p);
    block_rc.insert(block_rc.end(), C.block_rc.begin(), C.block_rc.end());
    block_c.insert(block_c.end(), C.block_c.begin(), C.block_c.end());
    b_c.insert(b_c.end(), C.b_c.begin(), C.b_c.end());
    vertex_of_all.insert(vertex_of_all.end(), U.vertex_of.begin(), U.vertex_of.end());
    n_vertices += it.n_vertices;
    n_edges += it.n_edges;
    h_doubles += (long long)(6 * m) * (6 * m + 1) / 2;
    n_max = std::max(n_max, 6 * m);
    it.stats.n_free = m;
  }
  if (n_vertices > (size_t)(1 << 26) || n_edges > (size_t)(1 << 24)) {
    g_last_error = std::string(kEntry) + ": more than 2^26 vertices or 2^24 edges in one call";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  std::vector<double> poses(16 * std::max<size_t>(n_vertices, 1));
  std::vector<dvo_amd_graph_edge> edges(std::max<size_t>(n_edges, 1));
  for (int g = 0; g < n_graphs; ++g) {
    const dvo_amd_graph_batch_item &it = items[g];
    if (it.n_vertices) std::memcpy(poses.data() + 16 * (size_t)its[g].pose_off, it.poses, 16 * sizeof(double) * it.n_vertices);
    if (it.n_edges) std::memcpy(edges.data() + its[g].edge_off, it.edges, sizeof(dvo_amd_graph_edge) * it.n_edges);
  }

  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->graph_batch_ws) ctx->graph_batch_ws = new GraphBatchWorkspace();
  GraphBatchWorkspace &W = *ctx->graph_batch_ws;
  const hipStream_t st = ctx->stream;
  const int stride = std::max(1, std::min(opt.max_iterations, graph_batch::kMaxRecords));
  auto grow_up = [&](DeviceBuf &b, const void *src, size_t bytes) {
    return grow_upload(b, src, bytes, st, "graph batch workspace", "graph batch upload");
  };
  GRAPH_TRY(grow_up(W.items, its.data(), sizeof(graph_batch::Item) * its.size()));
  GRAPH_TRY(grow_up(W.edges, edges.data(), sizeof(dvo_amd_graph_edge) * n_edges));
  GRAPH_TRY(grow_up(W.poses, poses.data(), 16 * sizeof(double) * n_vertices));
  GRAPH_TRY(grow_up(W.block_rc, block_rc.data(), sizeof(int2) * block_rc.size()));
  GRAPH_TRY(grow_up(W.block_ptr, block_ptr.data(), sizeof(int) * block_ptr.size()));
  GRAPH_TRY(grow_up(W.block_c, block_c.data(), sizeof(int) * block_c.size()));
  GRAPH_TRY(grow_up(W.b_ptr, b_ptr.data(), sizeof(int) * b_ptr.size()));
  GRAPH_TRY(grow_up(W.b_c, b_c.data(), sizeof(int) * b_c.size()));
  GRAPH_TRY(grow_up(W.vertex_of, vertex_of_all.data(), sizeof(int) * vertex_of_all.size()));
  const size_t E = std::max<size_t>(n_edges, 1);
  GRAPH_TRY(grow(W.saved, 16 * sizeof(double) * std::max<size_t>(n_vertices, 1)));
  GRAPH_TRY(grow(W.rec, sizeof(double) * graph_batch::kRecord * E));
  GRAPH_TRY(grow(W.chi2, sizeof(double) * E));
  GRAPH_TRY(grow(W.rho1, sizeof(double) * E));
  GRAPH_TRY(grow(W.H, sizeof(double) * (size_t)std::max<long long>(h_doubles, 1)));
  GRAPH_TRY(grow(W.out, sizeof(graph_batch::Out) * n_graphs));
  GRAPH_TRY(grow(W.records, sizeof(dvo_amd_graph_iteration) * (size_t)stride * n_graphs));
  // blocks no edge touches stay zero
  if (h_doubles) HIP_TRY(hipMemsetAsync(W.H.p, 0, sizeof(double) * (size_t)h_doubles, st));
  HIP_TRY(hipMemsetAsync(W.records.p, 0, sizeof(dvo_amd_graph_iteration) * (size_t)stride * n_graphs, st));

  const size_t lds = sizeof(double) * std::max<size_t>(1, (size_t)n_max * (n_max + 1) / 2);
  if (lds > W.lds_allowed) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(graph_batch::k_optimize_batch),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    W.lds_allowed = lds;
  }
  // both in the order of their declarations
  const graph_batch::Buffers B{(const graph_batch::Item *)W.items.p, (const dvo_amd_graph_edge *)W.edges.p, (double *)W.poses.p,
                               (double *)W.saved.p, (double *)W.rec.p, (double *)W.chi2.p, (double *)W.rho1.p, (double *)W.H.p,
                               (const int2 *)W.block_rc.p, (const int *)W.block_ptr.p, (const int *)W.block_c.p,
                               (const int *)W.b_ptr.p, (const int *)W.b_c.p, (const int *)W.vertex_of.p,
                               (graph_batch::Out *)W.out.p, (dvo_amd_graph_iteration *)W.records.p};
  const graph_batch::Params P{opt.algorithm, opt.max_iterations, opt.max_trials, stride,
                              opt.robust_delta, opt.initial_lambda, opt.initial_delta};
  hipLaunchKernelGGL(graph_batch::k_optimize_batch, dim3(n_graphs), dim3(graph_batch::kThreads), lds, st, B, P);
  HIP_TRY(hipGetLastError());

  std::vector<graph_batch::Out> out(n_graphs);
  std::vector<double> chi2(E), rho1(E);
  HIP_TRY(hipMemcpyAsync(out.data(), W.out.p, sizeof(graph_batch::Out) * n_graphs, hipMemcpyDeviceToHost, st));
  if (n_vertices) HIP_TRY(hipMemcpyAsync(poses.data(), W.poses.p, 16 * sizeof(double) * n_vertices, hipMemcpyDeviceToHost, st));
  if (n_edges) {
    HIP_TRY(hipMemcpyAsync(chi2.data(), W.chi2.p, sizeof(double) * n_edges, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rho1.data(), W.rho1.p, sizeof(double) * n_edges, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  W.last_graphs = n_graphs;
  W.last_stride = stride;
  W.last_iterations.resize(n_graphs);
  for (int g = 0; g < n_graphs; ++g) {
    dvo_amd_graph_batch_item &it = items[g];
    const graph_batch::Item &I = its[g];
    // only the free active vertices change: the others stay the caller's bits
    for (int s = 0; s < I.m; ++s) {
      const int v = vertex_of_all[I.slot_off + s];
      std::memcpy(it.poses + 16 * (size_t)v, poses.data() + 16 * ((size_t)I.pose_off + v), 16 * sizeof(double));
    }
    if (it.edge_chi2 && it.n_edges) std::memcpy(it.edge_chi2, chi2.data() + I.edge_off, sizeof(double) * it.n_edges);
    if (it.edge_weight && it.n_edges) std::memcpy(it.edge_weight, rho1.data() + I.edge_off, sizeof(double) * it.n_edges);
    it.stats.iterations = out[g].iterations;
    it.stats.termination = out[g].termination;
    it.stats.cholesky_failures = out[g].cholesky_failures;
    it.stats.initial_objective = out[g].initial_objective;
    it.stats.final_objective = out[g].final_objective;
    it.stats.lambda = out[g].lambda;
    it.stats.delta = out[g].delta;
    W.last_iterations[g] = out[g].iterations;
  }
  return DVO_AMD_OK;
}

}  // namespace

void graph_batch_workspace_release(dvo_amd_context *ctx) {
  GraphBatchWorkspace *w = ctx->graph_batch_ws;
  if (!w) return;
  w->each_buf([](DeviceBuf &b) {
    if (b.p) (void)hipFree(b.p);
  });
  delete w;
  ctx->graph_batch_ws = nullptr;
}

}  // namespace host
}  // namespace dvo_amd

extern "C" {

int dvo_amd_optimize_graphs_batch(dvo_amd_context *ctx, int n_graphs, dvo_amd_graph_batch_item *items,
                                  const dvo_amd_graph_options *opt) {
  using namespace dvo_amd::host;
  // the options, then every item, before anything is touched
  int rc = graph_check_arguments(kEntry, 0, nullptr, 0, nullptr, opt);
  if (rc) return rc;
  if (opt->solver != DVO_AMD_GRAPH_SOLVER_DENSE) {
    g_last_error = std::string(kEntry) + ": only DVO_AMD_GRAPH_SOLVER_DENSE";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  if (n_graphs < 0 || (n_graphs > 0 && !items)) {
    g_last_error = std::string(kEntry) + ": null pointer or negative count";
    return DVO_AMD_ERR_INVALID_ARGUMENT;
  }
  for (int g = 0; g < n_graphs; ++g) {
    const std::string where = std::string(kEntry) + ": item " + std::to_string(g);
    rc = graph_check_arguments(where.c_str(), items[g].n_vertices, items[g].poses, items[g].n_edges, items[g].edges, opt);
    if (rc) return rc;
  }
  for (int g = 0; g < n_graphs; ++g) {
    rc = check_capacity(std::string(kEntry) + ": item " + std::to_string(g),
                        free_unknowns(items[g].n_vertices, items[g].fixed, items[g].n_edges, items[g].edges).m,
                        DVO_AMD_GRAPH_BATCH_MAX_FREE_VERTICES, "a graph of the batch");
    if (rc) return rc;
  }
  rc = have_device();
  if (rc) return rc;
  if (!ctx) return DVO_AMD_ERR_INVALID_ARGUMENT;
  rc = dvo_amd::host::queue_must_be_idle(ctx, kEntry);
  if (rc) return rc;
  for (int g = 0; g < n_graphs; ++g) std::memset(&items[g].stats, 0, sizeof(items[g].stats));
  if (n_graphs == 0) return DVO_AMD_OK;
  return optimize_batch(ctx, n_graphs, items, *opt);
}

int dvo_amd_debug_graph_batch_records(dvo_amd_context *ctx, int graph, int capacity, dvo_amd_graph_iteration *records,
                                      int *n_recorded) {
  using namespace dvo_amd::host;
  int rc = have_device();
  if (rc) return rc;
  if (!ctx || capacity < 0 || (capacity > 0 && !records)) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const GraphBatchWorkspace *W = ctx->graph_batch_ws;
  if (!W || graph < 0 || graph >= W->last_graphs) return DVO_AMD_ERR_INVALID_ARGUMENT;
  const int n = std::min(W->last_iterations[graph], W->last_stride);
  if (n_recorded) *n_recorded = n;
  const int take = std::min(n, capacity);
  if (take > 0) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(records, (const dvo_amd_graph_iteration *)W->records.p + (size_t)graph * W->last_stride,
                      sizeof(dvo_amd_graph_iteration) * take, hipMemcpyDeviceToHost));
  }
  return DVO_AMD_OK;
}

}  // extern "C"
