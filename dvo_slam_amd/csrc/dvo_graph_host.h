// Host-only pieces shared by the pose-graph entries (dvo_graph.cpp, dvo_graph_batch.cpp): which vertices are unknowns, the
// capacity refusal, and the contributor lists that k_assemble_H / k_assemble_b (and the batch kernel's copies) sum in edge order.
#pragma once
#include <map>

#include "dvo_internal.h"

namespace dvo_amd {
namespace host {

#define GRAPH_TRY(expr)       \
  do {                        \
    const int rc_ = (expr);   \
    if (rc_) return rc_;      \
  } while (0)

// a device buffer of a graph workspace (DeviceBuf, dvo_call.h) grows in 4 KiB steps; `what` names the workspace in
// dvo_amd_last_error()
constexpr size_t kGraphBufStep = 1 << 12;

// grow to at least one byte, then the asynchronous upload (none for bytes == 0); `copy_what` names the upload
inline int grow_upload(DeviceBuf &b, const void *src, size_t bytes, hipStream_t st, const char *what, const char *copy_what) {
  const int rc = grow(b, bytes ? bytes : 1, kGraphBufStep, what);
  if (rc || !bytes) return rc;
  const hipError_t e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st);
  return e == hipSuccess ? DVO_AMD_OK : fail_hip(("hipMemcpyAsync (" + std::string(copy_what) + ")").c_str(), e);
}

// A workspace names its buffers once, in a list macro LIST(X) = X(a) X(b) ...: the members, and each_buf(f) over all of them.
#define DEVICE_BUF_MEMBER(name) DeviceBuf name;
#define DEVICE_BUF_VISIT(name) f(name);
#define DEVICE_BUF_MEMBERS(LIST) \
  LIST(DEVICE_BUF_MEMBER)        \
  template <class F>             \
  void each_buf(F f) {           \
    LIST(DEVICE_BUF_VISIT)       \
  }

// the unknowns: a vertex is active if an edge touches it and free if it is not fixed; free active vertices get the slots
// 0 .. m - 1 in increasing vertex index (slot[v] = -1 for every other vertex)
struct Unknowns {
  std::vector<int> slot, vertex_of;
  int m = 0;
};

inline Unknowns free_unknowns(int n_vertices, const int *fixed, int n_edges, const dvo_amd_graph_edge *edges) {
  std::vector<char> active(n_vertices, 0);
  for (int k = 0; k < n_edges; ++k) active[edges[k].from] = active[edges[k].to] = 1;
  Unknowns U;
  U.slot.assign(n_vertices, -1);
  for (int v = 0; v < n_vertices; ++v)
    if (active[v] && !(fixed && fixed[v])) {
      U.slot[v] = (int)U.vertex_of.size();
      U.vertex_of.push_back(v);
    }
  U.m = (int)U.vertex_of.size();
  return U;
}

// `which`: "the dense solver", "the sparse solver", "a graph of the batch"
inline int check_capacity(const std::string &entry, int m, int cap, const char *which) {
  if (m <= cap) return DVO_AMD_OK;
  g_last_error = entry + ": " + std::to_string(m) + " free active vertices (" + which + " takes at most " + std::to_string(cap) + ")";
  return DVO_AMD_ERR_CAPACITY;
}

// CSR by target block of H (sorted by (row, col) slot; codes edge * 4 + kind: 0 Aff, 1 Att, 2 Aft, 3 Aft^T) and by vertex slot
// of b (codes edge * 2 + (0 from, 1 to)), contributors in edge order.  lower_only: the lower image of H alone -- Aft into block
// (f, t) when f > t, else its transpose into block (t, f); without it both mirror images are listed.
struct Contributors {
  std::vector<int2> block_rc;
  std::vector<int> block_ptr, block_c, b_ptr, b_c;
};

inline Contributors contributor_lists(const Unknowns &U, int n_edges, const dvo_amd_graph_edge *edges, bool lower_only) {
  const int m = U.m;
  std::map<long long, std::vector<int>> blocks;
  std::vector<std::vector<int>> bl(std::max(m, 1));
  for (int k = 0; k < n_edges; ++k) {
    const int f = U.slot[edges[k].from], t = U.slot[edges[k].to];
    if (f >= 0) blocks[(long long)f * m + f].push_back(4 * k + 0), bl[f].push_back(2 * k + 0);
    if (t >= 0) blocks[(long long)t * m + t].push_back(4 * k + 1), bl[t].push_back(2 * k + 1);
    if (f >= 0 && t >= 0) {
      if (!lower_only || f > t) blocks[(long long)f * m + t].push_back(4 * k + 2);
      if (!lower_only || f <= t) blocks[(long long)t * m + f].push_back(4 * k + 3);
    }
  }
  Contributors C;
  C.block_ptr.push_back(0);
  for (const auto &kv : blocks) {
    C.block_rc.push_back(make_int2((int)(kv.first / std::max(m, 1)), (int)(kv.first % std::max(m, 1))));
    C.block_c.insert(C.block_c.end(), kv.second.begin(), kv.second.end());
    C.block_ptr.push_back((int)C.block_c.size());
  }
  C.b_ptr.push_back(0);
  for (int s = 0; s < m; ++s) {
    C.b_c.insert(C.b_c.end(), bl[s].begin(), bl[s].end());
    C.b_ptr.push_back((int)C.b_c.size());
  }
  return C;
}

}  // namespace host
}  // namespace dvo_amd
