// Graph traversal on the device: dgl.bfs_nodes_generator, bfs_edges_generator and topological_nodes_generator, the
// frontiers behind prop_nodes_bfs / prop_nodes_topo (TreeLSTM, junction-tree encoders, sweeps over a DAG).
//
// Reference: python/dgl/traversal.py copies the graph index to the CPU on every call and runs a sequential queue there
// (src/graph/traversal.cc); propagate.py copies every frontier back.  There is no GPU kernel.
//
// MI355X-first choices:
//  * The rule is the one of csrc/traversal_step.h, compiled here for the kernels and for dgla_traverse_host.  A level is
//    two passes over the frontier's rows.  Mark: every entry lowers (BFS) or raises (topological, which also decrements
//    the target's count) the target's key to its EXPANSION POSITION x, a 64-bit integer that keeps growing across levels.
//    Select: the entry whose x the key still holds owns the target.  min, max and the decrement commute, so the integer
//    atomics that apply them leave the same values whatever the arrival order, and no decision depends on it.
//  * The frontiers come out in the order of the reference's sequential queue (ascending x) WITHOUT a sort: select runs
//    count -> the library's scan (csrc/sort.hip.h) -> fill, and fill writes the survivors of row r at
//    (running offset) + offs[r] + popcount(lower lanes of the group's ballot bits), straight into the output array.
//    The next level reads its frontier from there.
//  * The hot path is a row stream, the idiom of csrc/labor.hip and csrc/subgraph.hip: a GROUP of G lanes strides one
//    frontier row with coalesced loads of `indices` through pointers that name the global address space; an entry costs
//    that load and ONE 8-byte gather of key[v] per pass (plus count[v] in the topological select).  G is 16 or 64 from
//    the CSR's mean degree (nnz / num_rows <= 32 -> 16); both widths write the same bits.
//  * The BFS mark reads key[v] before it updates: an entry that cannot lower the key (a node of an earlier level, or
//    one a smaller x already claimed) issues no atomic.  A stale read is only ever too large and costs one atomic.
//  * Working memory is O(n) (key, count) plus O(frontier) (row lengths and kept counts with their scans); nothing of
//    size nnz exists.  The edge form keeps the node frontiers in the workspace and writes the tree-edge ids to the
//    output at the same offsets.
//  * The host loop runs here.  A level is 6 launches (row lengths, scan, mark, count, scan, fill; the scans are 3
//    launches each above 32 768 rows) and ONE read-back of 24 bytes: the next frontier's size, the entries expanded
//    and the bad-source flag.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "sort.hip.h"
#include "traversal_step.h"

namespace dgla {
namespace {

constexpr int kTravBlock = 256;          // threads per workgroup: 256 / G rows
constexpr int64_t kTravShortMean = 32;   // mean degree up to which a row gets 16 lanes

int trav_group(const dgla_csr* c) {
  const int64_t rows = c->num_rows > 0 ? c->num_rows : 1;
  return c->nnz / rows <= kTravShortMean ? 16 : 64;
}

// the commutative updates of the mark pass, on the device: relaxed integer atomics at agent scope
struct DeviceUpdate {
  __device__ __forceinline__ void lower(int64_t* p, int64_t x) const {
    (void)__hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void raise(int64_t* p, int64_t x) const {
    (void)__hip_atomic_fetch_max(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void decrement(int64_t* p) const {
    (void)__hip_atomic_fetch_add(p, int64_t(-1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// ... and on the host
struct HostUpdate {
  void lower(int64_t* p, int64_t x) const {
    if (x < *p) *p = x;
  }
  void raise(int64_t* p, int64_t x) const {
    if (x > *p) *p = x;
  }
  void decrement(int64_t* p) const { --*p; }
};

// the bits of this lane's group in a wavefront ballot
template <int G>
__device__ __forceinline__ uint64_t group_bits(uint64_t ballot, int lane) {
  if constexpr (G == 64) {
    return ballot;
  } else {
    return (ballot >> (lane & ~(G - 1))) & ((uint64_t(1) << G) - 1);
  }
}

// state words of a call (device): what the host reads back once per level
enum : int { kStNext = 0, kStExpanded = 1, kStBad = 2, kStWords = 4 };

// ---- set-up -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTravBlock) void traverse_init_bfs_kernel(int64_t* __restrict__ key, int64_t n,
                                                                       int64_t* __restrict__ state) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock) + threadIdx.x;
  if (i < n) key[i] = kTravUnseen;
  if (i < kStWords) state[i] = 0;
}

// key[s] = kTravSource; a source outside [0, n) touches nothing and sets the bad flag (every writer stores 1)
template <typename Idx>
__global__ __launch_bounds__(kTravBlock) void traverse_sources_kernel(const Idx* __restrict__ sources, int64_t ns, int64_t n,
                                                                      int64_t* __restrict__ key, int64_t* __restrict__ state) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock) + threadIdx.x;
  if (i >= ns) return;
  const int64_t s = static_cast<int64_t>(sources[i]);
  if (s >= 0 && s < n)
    key[s] = kTravSource;
  else
    state[kStBad] = 1;
}

// topological: key = kTravSource, count = the degree in the opposite CSR, flag[i] = (count == 0), flag[n] = 0
template <typename Idx>
__global__ __launch_bounds__(kTravBlock) void traverse_init_topo_kernel(const Idx* __restrict__ opp_indptr, int64_t n,
                                                                        int64_t* __restrict__ key, int64_t* __restrict__ count,
                                                                        int64_t* __restrict__ flag, int64_t* __restrict__ state) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock) + threadIdx.x;
  if (i < kStWords) state[i] = 0;
  if (i == 0) flag[n] = 0;
  if (i >= n) return;
  const int64_t c = static_cast<int64_t>(opp_indptr[i + 1]) - static_cast<int64_t>(opp_indptr[i]);
  key[i] = kTravSource;
  count[i] = c;
  flag[i] = c == 0 ? 1 : 0;
}

// topological frontier 0: the nodes with count == 0, ascending, at their scanned rank
template <typename Idx>
__global__ __launch_bounds__(kTravBlock) void traverse_roots_kernel(const int64_t* __restrict__ count, const int64_t* __restrict__ rank,
                                                                    int64_t n, Idx* __restrict__ out, int64_t* __restrict__ state) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock) + threadIdx.x;
  if (i == 0) state[kStNext] = rank[n], state[kStExpanded] = 0;
  if (i >= n || count[i] != 0) return;
  const int64_t p = rank[i];
  if (p < n) out[p] = static_cast<Idx>(i);
}

// ---- a level ----------------------------------------------------------------------------------------
// len[i] = the row length of frontier position i, len[m] = 0 (closes the scan)
template <typename Idx>
__global__ __launch_bounds__(kTravBlock) void traverse_len_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ frontier,
                                                                  int64_t m, int64_t n, int64_t* __restrict__ len) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock) + threadIdx.x;
  if (i > m) return;
  int64_t lo = 0, hi = 0;
  if (i < m) trav_row((gptr<Idx>)indptr, frontier, n, i, &lo, &hi);
  len[i] = hi - lo;
}

template <typename Idx, int G, bool TOPO>
__global__ __launch_bounds__(kTravBlock) void traverse_mark_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                   const Idx* __restrict__ frontier, int64_t m, int64_t n,
                                                                   const int64_t* __restrict__ base, int64_t off,
                                                                   int64_t* key, int64_t* count) {
  const int lg = threadIdx.x & (G - 1);
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock / G) + threadIdx.x / G;
  if (i >= m) return;  // (whole groups leave)
  int64_t lo, hi;
  trav_row((gptr<Idx>)indptr, frontier, n, i, &lo, &hi);
  const int64_t x0 = off + base[i] - lo;
  for (int64_t q = lo + lg; q < hi; q += G)
    trav_mark<TOPO>((gptr<int64_t>)key, key, count, trav_target((gptr<Idx>)indices, n, q), x0 + q, DeviceUpdate{});
}

// The select pass.  FILL = false: cnt[i] = the kept entries of frontier position i (cnt[m] = 0 closes the scan).
// FILL = true: offs = the scanned counts; the kept entry of rank k in row i goes to position p = at + offs[i] + k of
// out_node (and of out_eid when EDGES); `cap` bounds every write.  One thread also leaves the level's read-back words.
template <typename Idx, int G, bool TOPO, bool FILL, bool EDGES>
__global__ __launch_bounds__(kTravBlock) void traverse_select_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                     const Idx* __restrict__ data, const Idx* __restrict__ frontier,
                                                                     int64_t m, int64_t n, const int64_t* __restrict__ base,
                                                                     int64_t off, const int64_t* __restrict__ key,
                                                                     const int64_t* __restrict__ count, int64_t* cnt,
                                                                     Idx* __restrict__ out_node, Idx* __restrict__ out_eid,
                                                                     int64_t at, int64_t cap, int64_t* __restrict__ state) {
  constexpr int R = 64 / G;
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTravBlock / G) + threadIdx.x / G;
  if constexpr (FILL) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[kStNext] = cnt[m], state[kStExpanded] = base[m];
  } else {
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[m] = 0;
  }
  if (i >= m) return;  // (whole groups leave)
  int64_t out_base = 0;
  if constexpr (FILL) {
    out_base = at + cnt[i];
    if (cnt[i + 1] - cnt[i] <= 0) return;  // nothing of this row survives
  }
  int64_t lo, hi;
  trav_row((gptr<Idx>)indptr, frontier, n, i, &lo, &hi);
  const int64_t x0 = off + base[i] - lo;
  int64_t run = 0;
  for (int64_t b = lo; b < hi; b += 64) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (b + r * G >= hi) break;  // (the same for every lane of the group)
      const int64_t q = b + r * G + lg;
      int64_t v = -1;
      if (q < hi) v = trav_target((gptr<Idx>)indices, n, q);
      const bool keep = trav_keep<TOPO>((gptr<int64_t>)key, (gptr<int64_t>)count, v, x0 + q);
      const uint64_t sub = group_bits<G>(__ballot(keep), lane);
      if constexpr (FILL) {
        if (keep) {
          const int64_t pos = out_base + run + __popcll(sub & ((uint64_t(1) << lg) - 1));
          if (pos < cap) {
            out_node[pos] = static_cast<Idx>(v);
            if constexpr (EDGES) out_eid[pos] = trav_eid<Idx>((gptr<Idx>)data, q);
          }
        }
      }
      run += __popcll(sub);
    }
  }
  if constexpr (!FILL) {
    if (lg == 0) cnt[i] = run;
  }
}

// ---- host side --------------------------------------------------------------------------------------
struct TravRows {  // the per-row arrays of a level: m + 1 entries each, and the scan's temporary
  size_t len, cnt, scan, bytes;
};

TravRows trav_rows(int64_t rows, Carver* c) {
  TravRows R{};
  const size_t at = c->bytes();
  R.len = c->take(sizeof(int64_t) * static_cast<size_t>(rows + 1));
  R.cnt = c->take(sizeof(int64_t) * static_cast<size_t>(rows + 1));
  R.scan = c->take(msd::scan_temp_bytes(rows + 1, sizeof(int64_t)));
  R.bytes = c->bytes() - at;
  return R;
}

struct TravLayout {  // offsets into the workspace of dgla_traverse
  size_t key, count, nodes, state, bytes;
  TravRows rows;
};

TravLayout trav_layout(int idtype_bits, int64_t n) {
  TravLayout L{};
  Carver c;
  L.key = c.take(sizeof(int64_t) * static_cast<size_t>(n));
  L.count = c.take(sizeof(int64_t) * static_cast<size_t>(n));
  L.nodes = c.take(static_cast<size_t>(idtype_bits / 8) * static_cast<size_t>(n));  // the node frontiers of the edge form
  L.state = c.take(sizeof(int64_t) * kStWords);
  L.rows = trav_rows(n, &c);  // a frontier after the first has at most n rows
  L.bytes = c.bytes();
  return L;
}

// everything dgla_traverse and dgla_traverse_host refuse before they read an array
int check_traverse(const char* who, int mode, const dgla_csr* csr, const dgla_csr* opposite, const void* sources,
                   int64_t num_sources, const void* ids, const int64_t* sections, const int64_t* num_ids,
                   const int64_t* num_sections) {
  if (mode != DGLA_TRAVERSE_BFS_NODES && mode != DGLA_TRAVERSE_BFS_EDGES && mode != DGLA_TRAVERSE_TOPO_NODES)
    return fail(who, "unknown mode " + std::to_string(mode));
  if (check_csr(who, csr, kCsrCols)) return -1;
  if (csr->num_rows != csr->num_cols)
    return fail(who, "invalid csr: traversal needs a square CSR, got " + std::to_string(csr->num_rows) + " x " +
                         std::to_string(csr->num_cols));
  if (!num_ids || !num_sections) return fail(who, "num_ids / num_sections are null");
  if (mode == DGLA_TRAVERSE_TOPO_NODES) {
    if (!opposite || !opposite->indptr)
      return fail(who, "the topological order needs the opposite CSR: its row lengths are the counts");
    if (opposite->idtype_bits != csr->idtype_bits) return fail(who, "csr and the opposite CSR differ in id type");
    if (opposite->num_rows != csr->num_rows || opposite->nnz != csr->nnz)
      return fail(who, "the count array does not match: the opposite CSR has " + std::to_string(opposite->num_rows) +
                           " rows and " + std::to_string(opposite->nnz) + " entries, the csr " +
                           std::to_string(csr->num_rows) + " and " + std::to_string(csr->nnz));
  } else {
    if (num_sources < 0) return fail(who, "negative number of sources");
    if (num_sources > 0 && !sources) return fail(who, "sources is null");
  }
  const int64_t cap = mode == DGLA_TRAVERSE_BFS_NODES ? csr->num_rows + num_sources : csr->num_rows;
  if (cap > 0 && (!ids || !sections)) return fail(who, "ids / sections are null");
  return 0;
}

int bad_source(const char* who, int64_t n) {
  return fail(who, "a source lies outside [0, " + std::to_string(n) + ")");
}

int loop_detected(const char* who, int64_t emitted, int64_t n) {
  return fail(who, "loop detected in the graph: only " + std::to_string(emitted) + " of " + std::to_string(n) +
                       " nodes have a topological order");
}

int count_mismatch(const char* who) {
  return fail(who, "the count array does not match the csr: more nodes were emitted than the graph has");
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename Idx>
int traverse_host(const char* who, int mode, const TypedCsr<Idx>& g, const dgla_csr* opposite, const Idx* sources, int64_t ns,
                  Idx* ids, int64_t* sections, int64_t* num_ids, int64_t* num_sections) {
  const int64_t n = g.num_rows;
  const Idx *indptr = g.indptr, *indices = g.indices, *data = g.data;
  const bool topo = mode == DGLA_TRAVERSE_TOPO_NODES, edges = mode == DGLA_TRAVERSE_BFS_EDGES;
  // refusals that need the arrays: nothing below reads through an id that failed here
  for (int64_t i = 0; i < n; ++i)
    if (indptr[i + 1] < indptr[i]) return fail(who, "invalid csr: indptr decreases at row " + std::to_string(i));
  if (static_cast<int64_t>(indptr[0]) != 0 || static_cast<int64_t>(indptr[n]) != g.nnz)
    return fail(who, "invalid csr: indptr does not span [0, nnz]");
  if (!topo)
    for (int64_t i = 0; i < ns; ++i)
      if (sources[i] < 0 || static_cast<int64_t>(sources[i]) >= n) return bad_source(who, n);

  std::vector<int64_t> key(static_cast<size_t>(n), topo ? kTravSource : kTravUnseen), count;
  std::vector<Idx> own;  // the node frontiers of the edge form
  Idx* nodes = ids;
  if (edges) own.resize(static_cast<size_t>(n)), nodes = own.data();
  const int64_t cap = mode == DGLA_TRAVERSE_BFS_NODES ? n + ns : n;
  const Idx* f = nullptr;
  int64_t m = 0, done = 0;  // done: entries of `nodes` used so far
  if (topo) {
    const Idx* op = static_cast<const Idx*>(opposite->indptr);
    count.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) count[i] = static_cast<int64_t>(op[i + 1]) - static_cast<int64_t>(op[i]);
    for (int64_t i = 0; i < n; ++i)
      if (count[i] == 0) nodes[m++] = static_cast<Idx>(i);
    f = nodes, done = m;
  } else {
    for (int64_t i = 0; i < ns; ++i) key[sources[i]] = kTravSource;
    if (mode == DGLA_TRAVERSE_BFS_NODES) {
      for (int64_t i = 0; i < ns; ++i) ids[i] = sources[i];
      done = ns;
    }
    f = sources, m = ns;
  }
  int64_t off = 0, nsec = 0, emitted = 0;
  if (m > 0 && !edges) sections[nsec++] = m;
  while (m > 0) {
    emitted += m;
    int64_t x = off;
    for (int64_t r = 0; r < m; ++r) {  // mark
      int64_t lo, hi;
      trav_row(indptr, f, n, r, &lo, &hi);
      for (int64_t q = lo; q < hi; ++q, ++x) {
        if (topo)
          trav_mark<true>(key.data(), key.data(), count.data(), trav_target(indices, n, q), x, HostUpdate{});
        else
          trav_mark<false>(key.data(), key.data(), count.data(), trav_target(indices, n, q), x, HostUpdate{});
      }
    }
    int64_t next = 0;
    x = off;
    for (int64_t r = 0; r < m; ++r) {  // select, in ascending x
      int64_t lo, hi;
      trav_row(indptr, f, n, r, &lo, &hi);
      for (int64_t q = lo; q < hi; ++q, ++x) {
        const int64_t v = trav_target(indices, n, q);
        const bool keep = topo ? trav_keep<true>(key.data(), count.data(), v, x)
                               : trav_keep<false>(key.data(), count.data(), v, x);
        if (!keep) continue;
        if (done + next >= cap) return count_mismatch(who);
        nodes[done + next] = static_cast<Idx>(v);
        if (edges) ids[done + next] = trav_eid<Idx>(data, q);
        ++next;
      }
    }
    off = x;
    f = nodes + done;
    done += next;
    m = next;
    if (m > 0) sections[nsec++] = m;
  }
  if (topo && emitted < n) return loop_detected(who, emitted, n);
  *num_ids = done;
  *num_sections = nsec;
  return 0;
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_traverse_workspace_bytes(int idtype_bits, int64_t num_nodes) {
  if (!idbits_ok(idtype_bits) || num_nodes <= 0) return 0;
  return trav_layout(idtype_bits, num_nodes).bytes;
}

int dgla_traverse(int mode, const dgla_csr* csr, const dgla_csr* opposite, const void* sources, int64_t num_sources,
                  void* ids, int64_t* sections, int64_t* num_ids, int64_t* num_sections, void* workspace,
                  size_t workspace_bytes, void* hip_stream) {
  const char* who = "traverse";
  if (check_traverse(who, mode, csr, opposite, sources, num_sources, ids, sections, num_ids, num_sections)) return -1;
  *num_ids = *num_sections = 0;
  const int64_t n = csr->num_rows;
  const bool topo = mode == DGLA_TRAVERSE_TOPO_NODES, edges = mode == DGLA_TRAVERSE_BFS_EDGES;
  const int64_t ns = topo ? 0 : num_sources;
  if (n == 0) return ns > 0 ? bad_source(who, n) : 0;  // (no node: every source is outside, and none is read)
  if (!topo && ns == 0) return 0;
  const TravLayout L = trav_layout(csr->idtype_bits, n);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, ids);
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  // a source list longer than n: the row arrays of frontier 0 do not fit the workspace and take scratch of their own
  Scratch wide(s);
  TravRows R0 = L.rows;
  char* rows0 = scratch.p;
  if (ns > n) {
    Carver c;
    R0 = trav_rows(ns, &c);
    if (wide.take(nullptr, 0, c.bytes())) return -1;
    rows0 = wide.p;
  }
  int64_t* key = reinterpret_cast<int64_t*>(scratch.p + L.key);
  int64_t* count = reinterpret_cast<int64_t*>(scratch.p + L.count);
  int64_t* state = reinterpret_cast<int64_t*>(scratch.p + L.state);
  const int64_t cap = mode == DGLA_TRAVERSE_BFS_NODES ? n + ns : n;
  int64_t nsec = 0, done = 0, emitted = 0;
  bool bad = false, over = false;
  const int rc = with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    const Idx *indptr = g.indptr, *indices = g.indices, *data = g.data;
    Idx* out = static_cast<Idx*>(ids);
    Idx* nodes = edges ? reinterpret_cast<Idx*>(scratch.p + L.nodes) : out;
    const dim3 block(kTravBlock);
    int64_t st[3] = {0, 0, 0};
    auto read_state = [&]() { return read_back(st, state, sizeof(st), s); };  // the one read-back of a level
    const Idx* f = nullptr;
    int64_t m = 0;
    if (topo) {
      int64_t* flag = reinterpret_cast<int64_t*>(scratch.p + L.rows.cnt);
      hipLaunchKernelGGL(traverse_init_topo_kernel<Idx>, dim3(grid1(n, kTravBlock)), block, 0, s,
                         static_cast<const Idx*>(opposite->indptr), n, key, count, flag, state);
      if (msd::exclusive_scan<int64_t, int64_t>(flag, flag, n + 1, scratch.p + L.rows.scan, s)) return -1;
      hipLaunchKernelGGL(traverse_roots_kernel<Idx>, dim3(grid1(n, kTravBlock)), block, 0, s, count, flag, n, nodes, state);
      if (read_state()) return -1;
      f = nodes, m = st[kStNext], done = m;
    } else {
      const Idx* src = static_cast<const Idx*>(sources);
      hipLaunchKernelGGL(traverse_init_bfs_kernel, dim3(grid1(n, kTravBlock)), block, 0, s, key, n, state);
      hipLaunchKernelGGL(traverse_sources_kernel<Idx>, dim3(grid1(ns, kTravBlock)), block, 0, s, src, ns, n, key, state);
      if (mode == DGLA_TRAVERSE_BFS_NODES) {
        DGLA_CHECK_HIP(hipMemcpyAsync(out, src, sizeof(Idx) * static_cast<size_t>(ns), hipMemcpyDeviceToDevice, s));
        done = ns;
      }
      f = src, m = ns;
    }
    if (m > 0 && !edges) sections[nsec++] = m;
    auto run = [&](auto g, auto is_topo, auto is_edges) -> int {
      constexpr int G = decltype(g)::value;
      constexpr bool TOPO = decltype(is_topo)::value, EDGES = decltype(is_edges)::value;
      int64_t off = 0;
      bool first = true;
      while (m > 0) {
        emitted += m;
        const TravRows& R = first ? R0 : L.rows;
        char* rp = first ? rows0 : scratch.p;
        int64_t* len = reinterpret_cast<int64_t*>(rp + R.len);
        int64_t* cnt = reinterpret_cast<int64_t*>(rp + R.cnt);
        const dim3 rows_grid(grid1(m, kTravBlock / G));
        hipLaunchKernelGGL(traverse_len_kernel<Idx>, dim3(grid1(m + 1, kTravBlock)), block, 0, s, indptr, f, m, n, len);
        if (msd::exclusive_scan<int64_t, int64_t>(len, len, m + 1, rp + R.scan, s)) return -1;
        hipLaunchKernelGGL((traverse_mark_kernel<Idx, G, TOPO>), rows_grid, block, 0, s, indptr, indices, f, m, n, len, off, key,
                           count);
        hipLaunchKernelGGL((traverse_select_kernel<Idx, G, TOPO, false, EDGES>), rows_grid, block, 0, s, indptr, indices, data,
                           f, m, n, len, off, key, count, cnt, static_cast<Idx*>(nullptr), static_cast<Idx*>(nullptr),
                           int64_t(0), int64_t(0), state);
        if (msd::exclusive_scan<int64_t, int64_t>(cnt, cnt, m + 1, rp + R.scan, s)) return -1;
        hipLaunchKernelGGL((traverse_select_kernel<Idx, G, TOPO, true, EDGES>), rows_grid, block, 0, s, indptr, indices, data, f,
                           m, n, len, off, key, count, cnt, nodes, out, done, cap, state);
        if (read_state()) return -1;
        if (st[kStBad]) {
          bad = true;
          return 0;
        }
        const int64_t next = st[kStNext];
        if (next < 0 || done + next > cap) {
          over = true;
          return 0;
        }
        off += st[kStExpanded];
        f = nodes + done;
        done += next;
        m = next;
        first = false;
        if (m > 0) sections[nsec++] = m;
      }
      return 0;
    };
    auto with_g = [&](auto is_topo, auto is_edges) -> int {
      if (trav_group(csr) == 16) return run(std::integral_constant<int, 16>{}, is_topo, is_edges);
      return run(std::integral_constant<int, 64>{}, is_topo, is_edges);
    };
    if (topo) return with_g(std::true_type{}, std::false_type{});
    if (edges) return with_g(std::false_type{}, std::true_type{});
    return with_g(std::false_type{}, std::false_type{});
  });
  if (rc) return -1;
  if (bad) return bad_source(who, n);
  if (over) return count_mismatch(who);
  if (topo && emitted < n) return loop_detected(who, emitted, n);
  *num_ids = done;
  *num_sections = nsec;
  return 0;
}

int dgla_traverse_host(int mode, const dgla_csr* csr, const dgla_csr* opposite, const void* sources, int64_t num_sources,
                       void* ids, int64_t* sections, int64_t* num_ids, int64_t* num_sections) {
  const char* who = "traverse_host";
  if (check_traverse(who, mode, csr, opposite, sources, num_sources, ids, sections, num_ids, num_sections)) return -1;
  *num_ids = *num_sections = 0;
  return with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    return traverse_host<Idx>(who, mode, TypedCsr<Idx>(csr), opposite, static_cast<const Idx*>(sources),
                              mode == DGLA_TRAVERSE_TOPO_NODES ? 0 : num_sources, static_cast<Idx*>(ids), sections, num_ids,
                              num_sections);
  });
}

}  // extern "C"
