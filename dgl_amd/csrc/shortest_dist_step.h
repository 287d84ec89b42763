// The rule of shortest distances and paths (include/dgl_amd.h, "Shortest distances and paths"): the pieces that the
// kernels of csrc/shortest_dist.hip and dgla_shortest_dist_host both compile, so the two cannot drift.
//
// Input.  The in-edge CSR of a homogeneous graph with n nodes (indptr[n + 1], indices[nnz] = the source of every
// in-edge, data[nnz] = the edge-id map or NULL; int32 or int64 ids) and a list of S source ids.
//
// dist.  dist[s][v] is the number of edges on a shortest directed path from sources[s] to v: 0 for the source itself,
// -1 when v cannot be reached.  int64 whatever the id type.
//
// Predecessor edge.  For every reachable v != sources[s], among the in-edges (u -> v) with dist[s][u] == dist[s][v] - 1
// the one with the smallest edge id.  A self-loop never qualifies (dist[s][v] != dist[s][v] - 1); among parallel edges
// the smallest id wins.  The minimum is a commutative reduction: it depends neither on thread order nor on the order of
// the CSR's entries.
//
// path.  paths[s][v][0 .. d) holds the predecessor edges walked back from v, stored front to back, so that
// paths[s][v][d - 1] enters v; paths[s][v][d .. L) is -1.  L is the largest entry of dist (0 without a reachable pair).
//
// An entry of `indices` outside [0, n) is ignored and nothing is read or written through it.  Integers only.
#pragma once
#include <stdint.h>

#include "random_walk_step.h"   // DGLA_RW_HD

namespace dgla {

// One entry of the predecessor table: the predecessor edge of (s, v) and the node it leaves; {-1, -1} without one.
template <typename Idx>
struct alignas(2 * sizeof(Idx)) SdPred {
  Idx edge, node;
};

// The predecessor of v from the row [lo, hi) of the in-edge CSR; dist_s is row s of dist, d = dist_s[v].
template <typename Idx, typename IdxPtr, typename DistPtr>
DGLA_RW_HD SdPred<Idx> sd_predecessor(IdxPtr indices, IdxPtr data, DistPtr dist_s, int64_t n, int64_t lo, int64_t hi,
                                      int64_t d) {
  SdPred<Idx> best{Idx(-1), Idx(-1)};
  if (d <= 0) return best;  // the source itself, or unreachable
  for (int64_t q = lo; q < hi; ++q) {
    const int64_t u = static_cast<int64_t>(indices[q]);
    if (u < 0 || u >= n || dist_s[u] != d - 1) continue;
    const Idx e = data ? static_cast<Idx>(data[q]) : static_cast<Idx>(q);
    if (best.edge < 0 || e < best.edge) best.edge = e, best.node = static_cast<Idx>(u);
  }
  return best;
}

// The walk-back of (s, v): positions [k_lo, k_hi) of the path, k_hi <= the steps left at `cur`, written last first to
// out[k - k_lo]; returns the node the walk stands on afterwards.  pred_s is row s of the predecessor table.  A table
// entry without an edge (never met on a table built by sd_predecessor) ends the walk with -1s.
template <typename Idx, typename PredPtr>
DGLA_RW_HD int64_t sd_walk_back(PredPtr pred_s, int64_t n, int64_t cur, int64_t k_lo, int64_t k_hi, int64_t* out) {
  for (int64_t k = k_hi - 1; k >= k_lo; --k) {
    int64_t e = -1;
    if (cur >= 0 && cur < n) {
      const SdPred<Idx> p = pred_s[cur];
      e = static_cast<int64_t>(p.edge);
      cur = static_cast<int64_t>(p.node);
    }
    out[k - k_lo] = e;
  }
  return cur;
}

}  // namespace dgla
