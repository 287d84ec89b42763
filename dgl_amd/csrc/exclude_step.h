// The rules of edge exclusion and of graph compaction (include/dgl_amd.h, "Edge exclusion and compaction"): ONE
// definition, compiled for the device (csrc/exclude.hip) and for the host twins (dgla_exclude_set_host,
// dgla_frontier_exclude_host, dgla_compact_nodes_host), so the two cannot drift.
//
// The exclusion set X.  A list of n_x edge ids sorted ascending, duplicates allowed, in the graph's id width.
// member(X, n_x, e): a lower-bound bisection (the first position whose id is >= e) followed by an equality test.
//
// Building X.  Seed edge ids ids[n] and optionally a reverse map rev[num_edges].  Slot k of the unsorted list holds
// ids[k] for k < n and rev[ids[k - n]] for n <= k < 2n (without rev there are n slots).  An id outside [0, num_edges)
// is never used as an index: its slot(s) hold num_edges, which is no edge's id, and the out-of-range bit is raised; a
// rev entry outside [0, num_edges) does the same for its slot.  X is the slots sorted ascending.
//
// The frontier filter.  A frontier is a CSR over the seeds: indptr[nr + 1], src[nnz], eids[nnz].  Entry j is kept iff
// !member(X, n_x, eids[j]); row i of the result holds the kept entries of [indptr[i], indptr[i + 1]) in their order.
// Row bounds are clamped into [0, nnz], so a malformed indptr reads nothing outside the arrays.
//
// Compaction of one node type.  `preserve` (np ids, repeats allowed) and `ends` (ne ids: the end points of this type of
// every edge of every graph).  nodes = the ids of preserve in the order given, a repeated id at its first position only,
// then the ids of ends that are not in preserve, ascending, each once.  local[e] = the index of ends[e] in nodes.  An id
// outside [0, num_nodes) raises the out-of-range bit, is never used as an index and gets local -1.
//
// Integer arithmetic only: host and device agree bit for bit.  The pointer types are template parameters so that the
// kernels can hand in pointers that name the global address space.
#pragma once
#include <stdint.h>

#include "random_walk_step.h"   // DGLA_RW_HD

namespace dgla {

constexpr int32_t kExcludeOutOfRange = 1;  // flags: some id lies outside its range

// e is in the ascending list x[0 .. n_x)
template <typename XPtr>
DGLA_RW_HD bool exclude_member(XPtr x, int64_t n_x, int64_t e) {
  int64_t lo = 0, hi = n_x;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (static_cast<int64_t>(x[mid]) < e)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n_x && static_cast<int64_t>(x[lo]) == e;
}

// slot k of the unsorted exclusion list; *bad = the slot met an id outside [0, num_edges)
template <typename IdsPtr, typename RevPtr>
DGLA_RW_HD int64_t exclude_slot(IdsPtr ids, RevPtr rev, int64_t n, int64_t num_edges, int64_t k, bool* bad) {
  const int64_t e = static_cast<int64_t>(ids[k < n ? k : k - n]);
  *bad = e < 0 || e >= num_edges;
  if (*bad) return num_edges;
  if (k < n) return e;
  const int64_t r = static_cast<int64_t>(rev[e]);
  *bad = r < 0 || r >= num_edges;
  return *bad ? num_edges : r;
}

// [lo, hi) of frontier row i, clamped into [0, nnz]
template <typename IndptrPtr>
DGLA_RW_HD void exclude_row(IndptrPtr indptr, int64_t nnz, int64_t i, int64_t* lo, int64_t* hi) {
  int64_t a = static_cast<int64_t>(indptr[i]), b = static_cast<int64_t>(indptr[i + 1]);
  a = a < 0 ? 0 : (a > nnz ? nnz : a);
  b = b < a ? a : (b > nnz ? nnz : b);
  *lo = a;
  *hi = b;
}

// compaction: position i of the ascending end-point list opens a new node (first of its run, inside the range, not
// preserved: its map entry is still -1)
template <typename SPtr, typename MapPtr>
DGLA_RW_HD bool compact_head(SPtr sorted, MapPtr map, int64_t num_nodes, int64_t i) {
  const int64_t v = static_cast<int64_t>(sorted[i]);
  if (v < 0 || v >= num_nodes) return false;
  if (i > 0 && static_cast<int64_t>(sorted[i - 1]) == v) return false;
  return map[v] < 0;
}

}  // namespace dgla
