// The rule of a node-induced subgraph (include/dgl_amd.h, "Induced subgraphs"): ONE definition, compiled for the device
// (subgraph_count_kernel / subgraph_fill_kernel, csrc/subgraph.hip) and for the host (dgla_induced_subgraph_host), so
// the two cannot drift.
//
// Setting.  One relation as a CSR: indptr, indices, data (the edge-id map, or NULL for the identity).  For
// in-neighbourhoods this is the in-edge CSR: rows are destinations, indices are sources.  A list rows[nr] of selected
// row ids, and a dense col_map with one int32 per COLUMN node: -1 = not selected, otherwise the node's local id.  On a
// homogeneous graph rows and the column selection are the same list and col_map[rows[i]] == i.
//
// Rule.  For position i and row r = rows[i], visit every j in [indptr[r], indptr[r + 1]) in order, with u = indices[j]
// and l = col_map[u].  The entry is kept iff l >= 0, and then yields the triple
//     (local_row = i, local_col = l, eid = data ? data[j] : j).
// A row id outside [0, num_rows) keeps nothing and is never dereferenced; neither is a column id outside [0, num_cols)
// (col_map has num_cols entries).
//
// Order.  Rows of the result go by i, then by j.  out_indptr[i] = the number of kept entries of the positions before i,
// out_indptr[nr] = the total.  The eid order of the result is the same triples sorted by eid, ties by (i, j); edge ids
// are distinct, so that order is unique.
//
// The node map.  mark sets map[ids[i]] = i for ids in [0, map_len) and reports an id outside it (kSubgraphOutOfRange);
// a second pass reports map[ids[i]] != i, i.e. a duplicate id (kSubgraphDuplicate).  clear writes -1 back.
//
// Integer arithmetic only: host and device agree bit for bit.  The pointer types are template parameters so that the
// kernels can hand in pointers that name the global address space.
#pragma once
#include <stdint.h>

#include "random_walk_step.h"   // DGLA_RW_HD

namespace dgla {

constexpr int32_t kSubgraphOutOfRange = 1;  // flags: some node id lies outside [0, map_len)
constexpr int32_t kSubgraphDuplicate = 2;   // flags: some node id appears twice

// [lo, hi) of position i's row; a row id outside [0, num_rows) is an empty row and touches no memory
template <typename IndptrPtr, typename RowsPtr>
DGLA_RW_HD void subgraph_row(IndptrPtr indptr, RowsPtr rows, int64_t num_rows, int64_t i, int64_t* lo, int64_t* hi) {
  const int64_t r = static_cast<int64_t>(rows[i]);
  *lo = *hi = 0;
  if (r >= 0 && r < num_rows) {
    *lo = static_cast<int64_t>(indptr[r]);
    *hi = static_cast<int64_t>(indptr[r + 1]);
  }
}

// entry j: the local column id when the entry is kept, else -1
template <typename IdxPtr, typename MapPtr>
DGLA_RW_HD int32_t subgraph_entry(IdxPtr indices, MapPtr col_map, int64_t num_cols, int64_t j) {
  const int64_t u = static_cast<int64_t>(indices[j]);
  if (u < 0 || u >= num_cols) return -1;
  const int32_t l = col_map[u];
  return l >= 0 ? l : -1;
}

// the edge id of entry j
template <typename Idx, typename IdxPtr>
DGLA_RW_HD Idx subgraph_eid(IdxPtr data, int64_t j) {
  return data ? static_cast<Idx>(data[j]) : static_cast<Idx>(j);
}

// The sort key of the eid order: (eid, position in row order) in one word, `pb` bits for the position.
DGLA_RW_HD int64_t subgraph_key(int64_t eid, int64_t pos, int pb) { return (eid << pb) | pos; }

}  // namespace dgla
