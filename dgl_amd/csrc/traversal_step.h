// The rule of level-by-level graph traversal (include/dgl_amd.h, "Graph traversal"): ONE definition, compiled for the
// device (traverse_mark_kernel / traverse_select_kernel, csrc/traversal.hip) and for the host (dgla_traverse_host), so
// the two cannot drift.
//
// Input.  One CSR (indptr[n + 1], indices[nnz], data[nnz] = the edge-id map or NULL; int32 or int64 ids): the out-edge
// CSR for a forward traversal, the in-edge CSR for a reverse one.  For BFS a list of source ids.
//
// Expansion position.  Let the current frontier be f[0 .. m) and base[r] the exclusive scan of the row lengths of f[r].
// Entry j of row f[r] has the position x = off + base[r] + j, where off is the number of entries every earlier frontier
// expanded: positions keep growing across levels, so a key written in one level is never mistaken for one of another
// and nothing has to be cleared.  x is a 64-bit integer (a level can expand more than 2^32 entries).
//
// BFS.  key[v] = kTravUnseen for every node, then kTravSource for the sources.  Frontier 0 is the source list as given
// (duplicates are kept).  Mark: every entry (x -> v) lowers key[v] to min(key[v], x); a node seen in an earlier level
// holds a key below `off` and is left alone by the min.  Select: the entry is kept iff key[v] == x, i.e. it is the
// first entry of this level that points at a node no earlier level saw.  The next frontier is the kept targets in
// ascending x, the tree edge of v the edge id of that entry.  Self-loops and parallel edges need no special case.
//
// Topological.  count[v] = the degree of v in the opposite CSR (the in-degree for a forward traversal; parallel edges
// count once each), key[v] = kTravSource.  Frontier 0 is the nodes with count == 0, ascending.  Mark: every entry
// (x -> v) decrements count[v] and raises key[v] to max(key[v], x).  Select: the entry is kept iff count[v] == 0 and
// key[v] == x, i.e. it is the last decrement of v.  A node on a loop (a self-loop is one) never reaches 0.
//
// Why this is the order of a sequential queue.  A queue pops the rows of a frontier in order and scans each row in
// order, which is ascending x.  BFS appends v at the first entry that finds it unseen (the smallest x); the topological
// sort appends v at the entry that takes its count to 0 (the largest x of its in-edges).
//
// An entry whose v lies outside [0, n) is ignored and nothing is read or written through it; a frontier id outside
// [0, n) is an empty row (and, for a source, is reported).
//
// Integer arithmetic only.  min, max and the decrement commute, so the final key and count of a level do not depend on
// the order in which entries arrive: the kernels apply them with integer atomics, the host in a loop, and both read the
// same values in the select pass.  The update is a template parameter for that reason, and the pointer types are
// template parameters so that the kernels can hand in pointers that name the global address space.
#pragma once
#include <stdint.h>

#include "random_walk_step.h"   // DGLA_RW_HD

namespace dgla {

constexpr int64_t kTravUnseen = INT64_MAX;  // BFS key of a node no entry has reached
constexpr int64_t kTravSource = -1;         // BFS key of a source; the topological key before any entry

// [lo, hi) of frontier position i's row; an id outside [0, n) is an empty row and touches no memory
template <typename IndptrPtr, typename RowsPtr>
DGLA_RW_HD void trav_row(IndptrPtr indptr, RowsPtr frontier, int64_t n, int64_t i, int64_t* lo, int64_t* hi) {
  const int64_t u = static_cast<int64_t>(frontier[i]);
  *lo = *hi = 0;
  if (u < 0 || u >= n) return;
  *lo = static_cast<int64_t>(indptr[u]);
  *hi = static_cast<int64_t>(indptr[u + 1]);
  if (*hi < *lo) *hi = *lo;
}

// the target of entry q, or -1 when it lies outside [0, n)
template <typename IdxPtr>
DGLA_RW_HD int64_t trav_target(IdxPtr indices, int64_t n, int64_t q) {
  const int64_t v = static_cast<int64_t>(indices[q]);
  return v >= 0 && v < n ? v : -1;
}

// Mark, entry (x -> v) with v from trav_target.  `up` applies the commutative updates: up.lower(key + v, x),
// up.raise(key + v, x), up.decrement(count + v).  The BFS form reads key[v] first and skips the update when it cannot
// lower it; a value read while others lower it is only ever too large, which costs an update and changes nothing.
template <bool TOPO, typename KeyPtr, typename Update>
DGLA_RW_HD void trav_mark(KeyPtr key_read, int64_t* key, int64_t* count, int64_t v, int64_t x, Update up) {
  if (v < 0) return;
  if constexpr (TOPO) {
    up.decrement(count + v);
    up.raise(key + v, x);
  } else {
    if (key_read[v] > x) up.lower(key + v, x);
  }
}

// Select, entry (x -> v): is v a node of the next frontier, and this its entry?
template <bool TOPO, typename KeyPtr>
DGLA_RW_HD bool trav_keep(KeyPtr key, KeyPtr count, int64_t v, int64_t x) {
  if (v < 0 || key[v] != x) return false;
  if constexpr (TOPO) return count[v] == 0;
  return true;
}

// the edge id of entry q
template <typename Idx, typename IdxPtr>
DGLA_RW_HD Idx trav_eid(IdxPtr data, int64_t q) {
  return data ? static_cast<Idx>(data[q]) : static_cast<Idx>(q);
}

}  // namespace dgla
