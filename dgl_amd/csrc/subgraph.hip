// Node-induced subgraphs on the device: the step behind dgl.node_subgraph on a mini-batch of nodes, dgl.khop_in_subgraph /
// khop_out_subgraph and the ShaDow / SAINT samplers of dgl.dataloading.
//
// Reference: the reference cuts a node-induced subgraph on the CPU only (src/graph/unit_graph.cc VertexSubgraph over
// aten::CSRSliceMatrix, a hash map of the selected ids consulted per entry); a graph on the GPU is copied back first.
//
// MI355X-first choices:
//  * The work is O(sum of deg(selected rows)), not O(N + E): the selection travels as a list of rows plus a dense
//    int32 map over the column nodes (caller-owned scratch that is all -1 between calls, like dgla_to_block's), so an
//    entry costs one coalesced id load and ONE 4-byte gather, and nothing of graph size is filled or scanned.
//  * The rule is the one of csrc/subgraph_step.h, compiled here for the kernels and for dgla_induced_subgraph_host.
//  * The hot path is a row stream, the idiom of csrc/labor.hip: a GROUP of G lanes strides one row with coalesced loads,
//    the keep flags of a step come from one __ballot (64 bits), and a kept entry goes to (row start) + (kept so far) +
//    popcount(the group's lower lanes): row order is preserved without atomics and without a sort.
//  * G is 16 or 64, chosen per call from the relation's mean degree (nnz / num_rows <= 32 -> 16).  Both widths write the
//    same bits.
//  * count and fill both evaluate the rule (2 * sum deg ids and gathers).  A keep bitmask written by count would need a
//    workspace sized by the rows' degrees, which the host does not know before count has run.
//  * The eid order (what node_subgraph documents) is the row-order result permuted by the library's own stable sort
//    (csrc/sort.hip.h): fill writes (eid, position) packed into one 64-bit key, sort_keys orders the keys, and one
//    gather pass unpacks them.  The sort sees `total` keys, never the graph.
//  * No atomics anywhere; the offsets come from the library's scan.  The node map is marked with racing plain stores:
//    when an id appears twice one writer wins, and the loser is seen by the check pass.
#include "../../include/dgl_amd.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "sort.hip.h"
#include "subgraph_step.h"

namespace dgla {
namespace {

constexpr int kSubBlock = 256;          // threads per workgroup: 256 / G rows
constexpr int64_t kSubShortMean = 32;   // mean degree up to which a row gets 16 lanes

int subgraph_group(const dgla_csr* c) {
  const int64_t rows = c->num_rows > 0 ? c->num_rows : 1;
  return c->nnz / rows <= kSubShortMean ? 16 : 64;
}

// the bits of this lane's group in a wavefront ballot
template <int G>
__device__ __forceinline__ uint64_t group_bits(uint64_t ballot, int lane) {
  if constexpr (G == 64) {
    return ballot;
  } else {
    return (ballot >> (lane & ~(G - 1))) & ((uint64_t(1) << G) - 1);
  }
}

// ---- the node map -----------------------------------------------------------------------------------
// pass 0: map[ids[i]] = i, an id outside [0, map_len) sets kSubgraphOutOfRange.  pass 1: map[ids[i]] != i sets
// kSubgraphDuplicate.  pass 2: map[ids[i]] = -1.  Every writer of *flags in one launch stores (what it read) | (the
// launch's one bit), so the racing plain stores agree.
template <typename Idx, int PASS>
__global__ __launch_bounds__(kSubBlock) void node_map_kernel(const Idx* __restrict__ ids, int64_t n, int32_t* __restrict__ map,
                                                             int64_t map_len, int32_t* flags) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kSubBlock) + threadIdx.x;
  if (i >= n) return;
  const int64_t v = static_cast<int64_t>(ids[i]);
  const bool inside = v >= 0 && v < map_len;
  if constexpr (PASS == 0) {
    if (inside)
      map[v] = static_cast<int32_t>(i);
    else
      *flags = *flags | kSubgraphOutOfRange;
  } else if constexpr (PASS == 1) {
    if (inside && map[v] != static_cast<int32_t>(i)) *flags = *flags | kSubgraphDuplicate;
  } else {
    if (inside) map[v] = -1;
  }
}

// ---- the sweep --------------------------------------------------------------------------------------
// One sweep of row [lo, hi) by a group of G lanes (lg = lane in the group, lane = lane in the wavefront): 64 positions
// per outer step in 64 / G sub-steps.  Returns the kept count (the same in every lane of the group).  FILL: the kept
// entry of rank k goes to position p = out_base + k; `cap` bounds every write.  KEYS: out_eid receives the sort key
// (eid, p) instead of the edge id (the eid order).
template <typename Idx, int G, bool FILL, bool KEYS>
__device__ __forceinline__ int64_t subgraph_sweep(gptr<Idx> indices, gptr<Idx> data, gptr<int32_t> col_map, int64_t num_cols,
                                                  int64_t lo, int64_t hi, int lg, int lane, int64_t i,
                                                  Idx* __restrict__ out_row, Idx* __restrict__ out_col,
                                                  Idx* __restrict__ out_eid, int64_t* __restrict__ out_key, int pb,
                                                  int64_t out_base, int64_t cap) {
  constexpr int R = 64 / G;
  int64_t run = 0;
  for (int64_t base = lo; base < hi; base += 64) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (base + r * G >= hi) break;  // (the same for every lane of the group)
      const int64_t q = base + r * G + lg;
      int32_t l = -1;
      if (q < hi) l = subgraph_entry(indices, col_map, num_cols, q);
      const bool keep = l >= 0;
      const uint64_t sub = group_bits<G>(__ballot(keep), lane);
      if constexpr (FILL) {
        if (keep) {
          const int64_t pos = out_base + run + __popcll(sub & ((uint64_t(1) << lg) - 1));
          if (pos < cap) {
            out_row[pos] = static_cast<Idx>(i);
            out_col[pos] = static_cast<Idx>(l);
            const Idx e = subgraph_eid<Idx>(data, q);
            if constexpr (KEYS)
              out_key[pos] = subgraph_key(static_cast<int64_t>(e), pos, pb);
            else
              out_eid[pos] = e;
          }
        }
      }
      run += __popcll(sub);
    }
  }
  return run;
}

// cnt[i] = kept entries of position i (int64; cnt[nr] = 0 closes the scan)
template <typename Idx, int G>
__global__ __launch_bounds__(kSubBlock) void subgraph_count_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                   const Idx* __restrict__ rows, int64_t nr, int64_t num_rows,
                                                                   int64_t num_cols, const int32_t* __restrict__ col_map,
                                                                   int64_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t i = blockIdx.x * static_cast<int64_t>(kSubBlock / G) + threadIdx.x / G;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[nr] = 0;
  if (i >= nr) return;  // (whole groups leave)
  int64_t lo, hi;
  subgraph_row((gptr<Idx>)indptr, rows, num_rows, i, &lo, &hi);
  const int64_t kept = subgraph_sweep<Idx, G, false, false>((gptr<Idx>)indices, gptr<Idx>(), (gptr<int32_t>)col_map, num_cols,
                                                            lo, hi, lg, lane, i, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
  if (lg == 0) cnt[i] = kept;
}

// out_indptr = the scanned offsets in the id type
template <typename Idx>
__global__ __launch_bounds__(kSubBlock) void subgraph_indptr_kernel(const int64_t* __restrict__ offs, int64_t nr,
                                                                    Idx* __restrict__ out_indptr) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kSubBlock) + threadIdx.x;
  if (i <= nr) out_indptr[i] = static_cast<Idx>(offs ? offs[i] : 0);
}

template <typename Idx, int G, bool KEYS>
__global__ __launch_bounds__(kSubBlock) void subgraph_fill_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                  const Idx* __restrict__ data, const Idx* __restrict__ rows,
                                                                  int64_t nr, int64_t num_rows, int64_t num_cols,
                                                                  const int32_t* __restrict__ col_map,
                                                                  const Idx* __restrict__ out_indptr, Idx* __restrict__ out_row,
                                                                  Idx* __restrict__ out_col, Idx* __restrict__ out_eid,
                                                                  int64_t* __restrict__ out_key, int pb, int64_t cap) {
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t i = blockIdx.x * static_cast<int64_t>(kSubBlock / G) + threadIdx.x / G;
  if (i >= nr) return;
  const int64_t at = static_cast<int64_t>(out_indptr[i]);
  if (static_cast<int64_t>(out_indptr[i + 1]) - at <= 0) return;
  int64_t lo, hi;
  subgraph_row((gptr<Idx>)indptr, rows, num_rows, i, &lo, &hi);
  (void)subgraph_sweep<Idx, G, true, KEYS>((gptr<Idx>)indices, (gptr<Idx>)data, (gptr<int32_t>)col_map, num_cols, lo, hi, lg,
                                           lane, i, out_row, out_col, out_eid, out_key, pb, at, cap);
}

// the eid order: sorted key i names the row-order position it came from
template <typename Idx>
__global__ __launch_bounds__(kSubBlock) void subgraph_permute_kernel(const int64_t* __restrict__ sorted, int64_t total, int pb,
                                                                     const Idx* __restrict__ tmp_row,
                                                                     const Idx* __restrict__ tmp_col, Idx* __restrict__ out_row,
                                                                     Idx* __restrict__ out_col, Idx* __restrict__ out_eid) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kSubBlock) + threadIdx.x;
  if (i >= total) return;
  const int64_t k = sorted[i];
  const int64_t p = k & ((int64_t(1) << pb) - 1);
  if (p >= total) return;  // (cannot happen for keys fill wrote; keeps the gathers inside the buffers whatever it reads)
  out_row[i] = tmp_row[p];
  out_col[i] = tmp_col[p];
  out_eid[i] = static_cast<Idx>(k >> pb);
}

// ---- host side --------------------------------------------------------------------------------------
struct SubLayout {  // offsets into the workspace of dgla_induced_subgraph_count / _fill
  size_t offs, scan, tmp_row, tmp_col, keys, sorted, sort, bytes;
};

SubLayout subgraph_layout(int idtype_bits, int64_t nr, int64_t total) {
  SubLayout L{};
  Carver c;
  const size_t id = idtype_bits / 8;
  L.offs = c.take(sizeof(int64_t) * static_cast<size_t>(nr + 1));
  L.scan = c.take(msd::scan_temp_bytes(nr + 1, sizeof(int64_t)));
  if (total > 0) {  // the eid order
    L.tmp_row = c.take(id * static_cast<size_t>(total));
    L.tmp_col = c.take(id * static_cast<size_t>(total));
    L.keys = c.take(sizeof(int64_t) * static_cast<size_t>(total));
    L.sorted = c.take(sizeof(int64_t) * static_cast<size_t>(total));
    L.sort = c.take(msd::make_keys_plan(total, 0, sizeof(int64_t)).bytes);
  }
  L.bytes = c.bytes();
  return L;
}

int check_map(const char* who, int idtype_bits, const void* ids, int64_t n, const void* map, int64_t map_len) {
  if (!idbits_ok(idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (n < 0 || map_len < 0) return fail(who, "negative size");
  if (n >= (int64_t(1) << 31)) return fail(who, "n must be below 2^31 (local ids are int32), got " + std::to_string(n));
  if (n > 0 && !ids) return fail(who, "ids is null");
  if (n > 0 && map_len > 0 && !map) return fail(who, "map is null");
  return 0;
}

// everything the subgraph entry points refuse
int check_subgraph(const char* who, const dgla_csr* csr, const void* rows, int64_t nr, const void* out_indptr) {
  if (check_csr(who, csr, kCsrCols | kCsrEmptyIndptr)) return -1;
  if (nr < 0) return fail(who, "negative size");
  if (nr >= (int64_t(1) << 31)) return fail(who, "the number of rows must be below 2^31, got " + std::to_string(nr));
  if (nr > 0 && !rows) return fail(who, "rows is null");
  if (!out_indptr) return fail(who, "out_indptr is null");
  return 0;
}

// f(integral_constant<int, G>): the group width of a call
template <typename F>
decltype(auto) with_group(const dgla_csr* csr, F&& f) {
  if (subgraph_group(csr) == 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 64>{});
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename Idx>
void subgraph_host(const TypedCsr<Idx>& g, const Idx* rows, int64_t nr, const Idx* cols, int64_t nc, int eid_order,
                   Idx* out_indptr, Idx* out_row, Idx* out_col, Idx* out_eid, int64_t* total, int32_t* flags) {
  std::vector<int32_t> map(static_cast<size_t>(g.num_cols), -1);
  int32_t fl = 0;
  for (int64_t i = 0; i < nc; ++i) {
    const int64_t v = static_cast<int64_t>(cols[i]);
    if (v < 0 || v >= g.num_cols)
      fl |= kSubgraphOutOfRange;
    else if (map[v] >= 0)
      fl |= kSubgraphDuplicate;   // (the first writer keeps the slot; a flagged call has no defined result)
    else
      map[v] = static_cast<int32_t>(i);
  }
  for (int64_t i = 0; i < nr; ++i) {
    const int64_t r = static_cast<int64_t>(rows[i]);
    if (r < 0 || r >= g.num_rows) fl |= kSubgraphOutOfRange;
  }
  int64_t at = 0;
  for (int64_t i = 0; i < nr; ++i) {
    out_indptr[i] = static_cast<Idx>(at);
    int64_t lo, hi;
    subgraph_row(g.indptr, rows, g.num_rows, i, &lo, &hi);
    for (int64_t j = lo; j < hi; ++j) {
      const int32_t l = subgraph_entry(g.indices, map.data(), g.num_cols, j);
      if (l < 0) continue;
      if (out_row) {
        out_row[at] = static_cast<Idx>(i);
        out_col[at] = static_cast<Idx>(l);
        out_eid[at] = subgraph_eid<Idx>(g.data, j);
      }
      ++at;
    }
  }
  out_indptr[nr] = static_cast<Idx>(at);
  *total = at;
  *flags = fl;
  if (!out_row || !eid_order || at == 0) return;
  std::vector<int64_t> order(static_cast<size_t>(at));
  for (int64_t p = 0; p < at; ++p) order[p] = p;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return out_eid[a] < out_eid[b]; });
  std::vector<Idx> r(out_row, out_row + at), c(out_col, out_col + at), e(out_eid, out_eid + at);
  for (int64_t p = 0; p < at; ++p) out_row[p] = r[order[p]], out_col[p] = c[order[p]], out_eid[p] = e[order[p]];
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

int dgla_node_map_mark(int idtype_bits, const void* ids, int64_t n, int32_t* map, int64_t map_len, int32_t* flags,
                       void* hip_stream) {
  const char* who = "node_map_mark";
  if (check_map(who, idtype_bits, ids, n, map, map_len)) return -1;
  if (!flags) return fail(who, "flags is null");
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, flags);
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    hipLaunchKernelGGL((node_map_kernel<Idx, 0>), dim3(grid1(n, kSubBlock)), dim3(kSubBlock), 0, s,
                       static_cast<const Idx*>(ids), n, map, map_len, flags);
    hipLaunchKernelGGL((node_map_kernel<Idx, 1>), dim3(grid1(n, kSubBlock)), dim3(kSubBlock), 0, s,
                       static_cast<const Idx*>(ids), n, map, map_len, flags);
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_node_map_clear(int idtype_bits, const void* ids, int64_t n, int32_t* map, int64_t map_len, void* hip_stream) {
  if (check_map("node_map_clear", idtype_bits, ids, n, map, map_len)) return -1;
  if (n == 0 || map_len == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, map);
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    hipLaunchKernelGGL((node_map_kernel<Idx, 2>), dim3(grid1(n, kSubBlock)), dim3(kSubBlock), 0, s,
                       static_cast<const Idx*>(ids), n, map, map_len, static_cast<int32_t*>(nullptr));
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

size_t dgla_induced_subgraph_workspace_bytes(int idtype_bits, int64_t nr, int64_t total) {
  if (!idbits_ok(idtype_bits) || nr < 0 || nr >= (int64_t(1) << 31) || total < 0) return 0;
  return subgraph_layout(idtype_bits, nr, total).bytes;
}

int dgla_induced_subgraph_count(const dgla_csr* csr, const void* rows, int64_t nr, const int32_t* col_map, void* out_indptr,
                                void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "induced_subgraph_count";
  if (check_subgraph(who, csr, rows, nr, out_indptr)) return -1;
  if (!col_map) return fail(who, "col_map is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const bool sweep = nr > 0 && csr->nnz > 0 && csr->num_cols > 0;  // otherwise every row is empty: no graph memory is read
  SubLayout L{};
  if (sweep) {
    L = subgraph_layout(csr->idtype_bits, nr, 0);
    if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  }
  const DeviceGuard dev(s, out_indptr);
  char* ws = static_cast<char*>(workspace);
  int64_t* offs = sweep ? reinterpret_cast<int64_t*>(ws + L.offs) : nullptr;
  if (sweep) {
    with_idx(csr->idtype_bits, [&](auto tag) {
      using Idx = decltype(tag);
      const TypedCsr<Idx> g(csr);
      with_group(csr, [&](auto grp) {
        constexpr int G = decltype(grp)::value;
        hipLaunchKernelGGL((subgraph_count_kernel<Idx, G>), dim3(grid1(nr, kSubBlock / G)), dim3(kSubBlock), 0, s, g.indptr,
                           g.indices, static_cast<const Idx*>(rows), nr, g.num_rows, g.num_cols, col_map, offs);
      });
    });
    DGLA_CHECK_HIP(hipGetLastError());
    if (msd::exclusive_scan<int64_t, int64_t>(offs, offs, nr + 1, ws + L.scan, s)) return -1;
  }
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    hipLaunchKernelGGL(subgraph_indptr_kernel<Idx>, dim3(grid1(nr + 1, kSubBlock)), dim3(kSubBlock), 0, s, offs, nr,
                       static_cast<Idx*>(out_indptr));
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_induced_subgraph_fill(const dgla_csr* csr, const void* rows, int64_t nr, const int32_t* col_map,
                               const void* out_indptr, int64_t total, void* out_row, void* out_col, void* out_eid,
                               int eid_order, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "induced_subgraph_fill";
  if (check_subgraph(who, csr, rows, nr, out_indptr)) return -1;
  if (!col_map) return fail(who, "col_map is null");
  if (total < 0) return fail(who, "negative total");
  if (total > csr->nnz) return fail(who, "total exceeds the csr's nnz");
  if (nr == 0 || total == 0) return 0;  // nothing was counted
  if (!out_row || !out_col || !out_eid) return fail(who, "out_row / out_col / out_eid are null");
  const int pb = msd::bits_for(total), eb = msd::bits_for(csr->nnz);
  SubLayout L{};
  if (eid_order) {
    if (pb + eb > 63)
      return fail(who, "the eid order packs (edge id, position) into 63 bits; " + std::to_string(eb) + " + " +
                           std::to_string(pb) + " bits do not fit");
    L = subgraph_layout(csr->idtype_bits, nr, total);
    if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_row);
  char* ws = static_cast<char*>(workspace);
  int rc = 0;
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    const Idx *rws = static_cast<const Idx*>(rows), *optr = static_cast<const Idx*>(out_indptr);
    Idx *o_row = static_cast<Idx*>(out_row), *o_col = static_cast<Idx*>(out_col), *o_eid = static_cast<Idx*>(out_eid);
    with_group(csr, [&](auto grp) {
      constexpr int G = decltype(grp)::value;
      const dim3 grid(grid1(nr, kSubBlock / G)), block(kSubBlock);
      if (!eid_order) {
        hipLaunchKernelGGL((subgraph_fill_kernel<Idx, G, false>), grid, block, 0, s, g.indptr, g.indices, g.data, rws, nr,
                           g.num_rows, g.num_cols, col_map, optr, o_row, o_col, o_eid, static_cast<int64_t*>(nullptr), 0, total);
      } else {
        hipLaunchKernelGGL((subgraph_fill_kernel<Idx, G, true>), grid, block, 0, s, g.indptr, g.indices, g.data, rws, nr,
                           g.num_rows, g.num_cols, col_map, optr, reinterpret_cast<Idx*>(ws + L.tmp_row),
                           reinterpret_cast<Idx*>(ws + L.tmp_col), static_cast<Idx*>(nullptr), reinterpret_cast<int64_t*>(ws + L.keys), pb,
                           total);
      }
    });
    if (eid_order) {
      int64_t* sorted = reinterpret_cast<int64_t*>(ws + L.sorted);
      rc = msd::sort_keys<int64_t>(reinterpret_cast<const int64_t*>(ws + L.keys), sorted, total, eb + pb, ws + L.sort, s);
      if (rc) return;
      hipLaunchKernelGGL(subgraph_permute_kernel<Idx>, dim3(grid1(total, kSubBlock)), dim3(kSubBlock), 0, s, sorted, total, pb,
                         reinterpret_cast<const Idx*>(ws + L.tmp_row), reinterpret_cast<const Idx*>(ws + L.tmp_col), o_row,
                         o_col, o_eid);
    }
  });
  if (rc) return -1;
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_induced_subgraph_host(const dgla_csr* csr, const void* rows, int64_t nr, const void* cols, int64_t nc,
                               int eid_order, void* out_indptr, void* out_row, void* out_col, void* out_eid, int64_t* total,
                               int32_t* flags) {
  const char* who = "induced_subgraph_host";
  if (check_subgraph(who, csr, rows, nr, out_indptr)) return -1;
  if (nc < 0) return fail(who, "negative size");
  if (nc >= (int64_t(1) << 31)) return fail(who, "the number of columns must be below 2^31");
  if (nc > 0 && !cols) return fail(who, "cols is null");
  if (!total || !flags) return fail(who, "total / flags are null");
  if (out_row && (!out_col || !out_eid)) return fail(who, "out_col / out_eid are null");
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    subgraph_host<Idx>(TypedCsr<Idx>(csr), static_cast<const Idx*>(rows), nr, static_cast<const Idx*>(cols), nc, eid_order,
                       static_cast<Idx*>(out_indptr), static_cast<Idx*>(out_row), static_cast<Idx*>(out_col),
                       static_cast<Idx*>(out_eid), total, flags);
  });
  return 0;
}

}  // extern "C"
