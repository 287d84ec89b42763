// Edge exclusion and graph compaction on the device: what a link-prediction mini-batch needs on top of neighbour
// sampling.  The exclusion set (seed edges and their reverses, sorted), the filter that drops the set's edges from a
// sampled frontier, and the node compaction behind dgl.compact_graphs.
//
// Reference: python/dgl/sampling/utils.py EidExcluder (sample first, then drop; on the GPU a boolean mask built by
// torch-level isin), python/dgl/dataloading/base.py find_exclude_eids / EdgePredictionSampler, and
// src/graph/transform/cuda/cuda_compact_graph.cu (a device hash table filled with atomic inserts; its node order is
// whatever the insertion races leave).
//
// MI355X-first choices:
//  * X is tiny (2 x the batch) and stays in L2: membership is a bisection, ceil(log2 n_x) dependent loads per entry, no
//    hash table, no atomics, nothing sized by the graph and nothing to clean afterwards.
//  * The filter is a row stream, the idiom of csrc/subgraph.hip: a GROUP of G lanes (16 or 64, by mean row length) strides
//    a row with coalesced loads, the keep flags of a step come from one __ballot, and a kept entry goes to (row start) +
//    (kept so far) + popcount(the group's lower lanes).  Row order is preserved without atomics and without a sort.
//  * count writes ONE KEEP BYTE per entry into the workspace and fill reads it back: the frontier's nnz is known before
//    the call, so the bytes can be laid out up front, and the chain of dependent loads is walked once, not twice.
//  * One call: count -> the library's scan -> fill into caller-allocated outputs of nnz entries.  No read-back inside.
//  * Compaction keeps the first occurrence of a preserved id with one unsigned atomicMin per id on the node map (-1 is
//    the largest unsigned word, so the smallest position wins whatever the launch order); everything after that is the
//    library's sort and scan and plain stores.
#include "../../include/dgl_amd.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "sort.hip.h"
#include "exclude_step.h"   // (after the HIP runtime that host_util.h brings in)

namespace dgla {
namespace {

constexpr int kExBlock = 256;          // threads per workgroup: 256 / G rows
constexpr int64_t kExShortMean = 32;   // mean row length up to which a row gets 16 lanes

int exclude_group(int64_t nr, int64_t nnz) { return nnz / (nr > 0 ? nr : 1) <= kExShortMean ? 16 : 64; }

// the bits of this lane's group in a wavefront ballot
template <int G>
__device__ __forceinline__ uint64_t ex_group_bits(uint64_t ballot, int lane) {
  if constexpr (G == 64) {
    return ballot;
  } else {
    return (ballot >> (lane & ~(G - 1))) & ((uint64_t(1) << G) - 1);
  }
}

// ---- the exclusion set ------------------------------------------------------------------------------
// keys[k] = slot k of the unsorted list.  Every writer of *flags stores (what it read) | (the one bit), so the racing
// plain stores agree.
template <typename Idx>
__global__ __launch_bounds__(kExBlock) void exclude_slots_kernel(const Idx* __restrict__ ids, const Idx* __restrict__ rev, int64_t n,
                                                                 int64_t m, int64_t num_edges, Idx* __restrict__ keys,
                                                                 int32_t* flags) {
  const int64_t k = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if (k >= m) return;
  bool bad;
  keys[k] = static_cast<Idx>(exclude_slot((gptr<Idx>)ids, (gptr<Idx>)rev, n, num_edges, k, &bad));
  if (bad) *flags = *flags | kExcludeOutOfRange;
}

// ---- the filter -------------------------------------------------------------------------------------
// One group of G lanes per frontier row, 64 positions per outer step in 64 / G sub-steps.  !FILL: evaluates the rule,
// stores the keep byte of every entry and cnt[i] = the row's kept count.  FILL: reads the keep bytes; the kept entry of
// rank k of row i goes to offs[i] + k (`nnz` bounds every write).
template <typename Idx, int G, bool FILL>
__global__ __launch_bounds__(kExBlock) void exclude_sweep_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ src,
                                                                 const Idx* __restrict__ eids, int64_t nr, int64_t nnz,
                                                                 const Idx* __restrict__ x, int64_t n_x, uint8_t* keep,
                                                                 int64_t* cnt, Idx* __restrict__ out_src,
                                                                 Idx* __restrict__ out_eids) {
  constexpr int R = 64 / G;
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t i = blockIdx.x * static_cast<int64_t>(kExBlock / G) + threadIdx.x / G;
  if constexpr (!FILL) {
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[nr] = 0;   // closes the scan
  }
  if (i >= nr) return;  // (whole groups leave)
  int64_t lo, hi;
  exclude_row((gptr<Idx>)indptr, nnz, i, &lo, &hi);
  const int64_t at = FILL ? cnt[i] : 0;   // (fill: cnt holds the scanned offsets)
  int64_t run = 0;
  for (int64_t base = lo; base < hi; base += 64) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (base + r * G >= hi) break;  // (the same for every lane of the group)
      const int64_t q = base + r * G + lg;
      bool k = false;
      Idx e = 0;
      if (q < hi) {
        if constexpr (FILL) {
          k = keep[q] != 0;
        } else {
          e = eids[q];
          k = !exclude_member((gptr<Idx>)x, n_x, static_cast<int64_t>(e));
          keep[q] = k ? 1 : 0;
        }
      }
      const uint64_t sub = ex_group_bits<G>(__ballot(k), lane);
      if constexpr (FILL) {
        if (k) {
          const int64_t pos = at + run + __popcll(sub & ((uint64_t(1) << lg) - 1));
          if (pos < nnz) {
            out_src[pos] = src[q];
            out_eids[pos] = eids[q];
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

// out_indptr = the scanned offsets in the id type (offs == nullptr: all zero)
template <typename Idx>
__global__ __launch_bounds__(kExBlock) void exclude_indptr_kernel(const int64_t* __restrict__ offs, int64_t nr,
                                                                  Idx* __restrict__ out_indptr) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if (i <= nr) out_indptr[i] = static_cast<Idx>(offs ? offs[i] : 0);
}

// ---- compaction -------------------------------------------------------------------------------------
// PASS 0: map[preserve[i]] = min over the positions i of that id (unsigned min: -1 is the largest word).
// PASS 1: cnt[i] = 1 when position i is the first of its id.
template <typename Idx, int PASS>
__global__ __launch_bounds__(kExBlock) void compact_preserve_kernel(const Idx* __restrict__ preserve, int64_t np, int32_t* map,
                                                                    int64_t num_nodes, int64_t* __restrict__ cnt, int32_t* flags) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if constexpr (PASS == 1) {
    if (i == np) cnt[np] = 0;
  }
  if (i >= np) return;
  const int64_t v = static_cast<int64_t>(preserve[i]);
  const bool inside = v >= 0 && v < num_nodes;
  if constexpr (PASS == 0) {
    if (inside)
      atomicMin(reinterpret_cast<unsigned int*>(map + v), static_cast<unsigned int>(i));
    else
      *flags = *flags | kExcludeOutOfRange;
  } else {
    cnt[i] = inside && map[v] == static_cast<int32_t>(i) ? 1 : 0;
  }
}

// the first occurrences take their rank: nodes[rank] = id, map[id] = rank (one writer per id)
template <typename Idx>
__global__ __launch_bounds__(kExBlock) void compact_preserve_assign_kernel(const Idx* __restrict__ preserve, int64_t np,
                                                                           const int64_t* __restrict__ offs, int32_t* map,
                                                                           Idx* __restrict__ nodes) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if (i >= np) return;
  const int64_t r = offs[i];
  if (offs[i + 1] == r) return;
  nodes[r] = preserve[i];
  map[static_cast<int64_t>(preserve[i])] = static_cast<int32_t>(r);
}

// sort keys of the end points: the id, or num_nodes for an id outside the range
template <typename Idx>
__global__ __launch_bounds__(kExBlock) void compact_keys_kernel(const Idx* __restrict__ ends, int64_t ne, int64_t num_nodes,
                                                                Idx* __restrict__ keys, int32_t* flags) {
  const int64_t e = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if (e >= ne) return;
  const int64_t v = static_cast<int64_t>(ends[e]);
  const bool inside = v >= 0 && v < num_nodes;
  keys[e] = static_cast<Idx>(inside ? v : num_nodes);
  if (!inside) *flags = *flags | kExcludeOutOfRange;
}

template <typename Idx>
__global__ __launch_bounds__(kExBlock) void compact_heads_kernel(const Idx* __restrict__ sorted, int64_t ne, const int32_t* map,
                                                                 int64_t num_nodes, int64_t* __restrict__ cnt) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if (i == ne) cnt[ne] = 0;
  if (i >= ne) return;
  cnt[i] = compact_head((gptr<Idx>)sorted, (gptr<int32_t>)map, num_nodes, i) ? 1 : 0;
}

// the new nodes follow the preserved ones: rank = (preserved count) + (heads before i)
template <typename Idx>
__global__ __launch_bounds__(kExBlock) void compact_heads_assign_kernel(const Idx* __restrict__ sorted, int64_t ne,
                                                                        const int64_t* __restrict__ offs_e,
                                                                        const int64_t* __restrict__ kept_p, int64_t cap,
                                                                        int32_t* map, Idx* __restrict__ nodes,
                                                                        int64_t* __restrict__ num_out) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  const int64_t kp = kept_p ? *kept_p : 0;
  if (i == 0) *num_out = kp + (offs_e ? offs_e[ne] : 0);
  if (i >= ne) return;
  const int64_t r = offs_e[i];
  if (offs_e[i + 1] == r) return;
  const int64_t pos = kp + r;
  if (pos >= cap) return;  // (cannot happen: at most np + ne nodes)
  nodes[pos] = sorted[i];
  map[static_cast<int64_t>(sorted[i])] = static_cast<int32_t>(pos);
}

// PASS 0: local[e] = map[ends[e]].  PASS 1: map[ids[e]] = -1.
template <typename Idx, int PASS>
__global__ __launch_bounds__(kExBlock) void compact_lookup_kernel(const Idx* __restrict__ ids, int64_t n, int32_t* map,
                                                                  int64_t num_nodes, Idx* __restrict__ local) {
  const int64_t e = blockIdx.x * static_cast<int64_t>(kExBlock) + threadIdx.x;
  if (e >= n) return;
  const int64_t v = static_cast<int64_t>(ids[e]);
  const bool inside = v >= 0 && v < num_nodes;
  if constexpr (PASS == 0) {
    local[e] = static_cast<Idx>(inside ? map[v] : -1);
  } else {
    if (inside) map[v] = -1;
  }
}

// ---- host side --------------------------------------------------------------------------------------
int key_bits_for(int64_t top) {  // keys in [0, top]; 0 = every value bit of the id type
  return top >= (int64_t(1) << 62) ? 0 : msd::bits_for(top + 1);
}

struct SetLayout {  // workspace of dgla_exclude_set
  size_t keys, sort, bytes;
};
SetLayout set_layout(int idtype_bits, int64_t m) {
  SetLayout L{};
  Carver c;
  const size_t id = idtype_bits / 8;
  L.keys = c.take(id * static_cast<size_t>(m));
  L.sort = c.take(msd::make_keys_plan(m, 0, id).bytes);
  L.bytes = c.bytes();
  return L;
}

struct FilterLayout {  // workspace of dgla_frontier_exclude
  size_t keep, offs, scan, bytes;
};
FilterLayout filter_layout(int64_t nr, int64_t nnz) {
  FilterLayout L{};
  Carver c;
  L.keep = c.take(static_cast<size_t>(nnz));
  L.offs = c.take(sizeof(int64_t) * static_cast<size_t>(nr + 1));
  L.scan = c.take(msd::scan_temp_bytes(nr + 1, sizeof(int64_t)));
  L.bytes = c.bytes();
  return L;
}

struct CompactLayout {  // workspace of dgla_compact_nodes
  size_t offs_p, scan_p, keys, sorted, offs_e, scan_e, sort, bytes;
};
CompactLayout compact_layout(int idtype_bits, int64_t np, int64_t ne) {
  CompactLayout L{};
  Carver c;
  const size_t id = idtype_bits / 8;
  L.offs_p = c.take(sizeof(int64_t) * static_cast<size_t>(np + 1));
  L.scan_p = c.take(msd::scan_temp_bytes(np + 1, sizeof(int64_t)));
  L.keys = c.take(id * static_cast<size_t>(ne));
  L.sorted = c.take(id * static_cast<size_t>(ne));
  L.offs_e = c.take(sizeof(int64_t) * static_cast<size_t>(ne + 1));
  L.scan_e = c.take(msd::scan_temp_bytes(ne + 1, sizeof(int64_t)));
  L.sort = c.take(msd::make_keys_plan(ne, 0, id).bytes);
  L.bytes = c.bytes();
  return L;
}

bool sizes_ok(int idtype_bits, int64_t a, int64_t b) {
  return idbits_ok(idtype_bits) && a >= 0 && b >= 0 && a < (int64_t(1) << 31) && b < (int64_t(1) << 31);
}

int check_set(const char* who, int idtype_bits, const void* ids, int64_t n, int64_t num_edges, const void* out,
              const void* flags) {
  if (!idbits_ok(idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (n < 0 || num_edges < 0) return fail(who, "negative size");
  if (n >= (int64_t(1) << 30)) return fail(who, "n must be below 2^30, got " + std::to_string(n));
  if (idtype_bits == 32 && num_edges > INT32_MAX) return fail(who, "num_edges does not fit the id type");
  if (n > 0 && (!ids || !out)) return fail(who, "ids / out are null");
  if (!flags) return fail(who, "flags is null");
  return 0;
}

int check_filter(const char* who, int idtype_bits, const void* indptr, const void* src, const void* eids, int64_t nr,
                 int64_t nnz, const void* x, int64_t n_x, const void* out_indptr, const void* out_src, const void* out_eids) {
  if (!idbits_ok(idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (nr < 0 || nnz < 0 || n_x < 0) return fail(who, "negative size");
  if (nr >= (int64_t(1) << 31)) return fail(who, "the number of rows must be below 2^31, got " + std::to_string(nr));
  if (!indptr || !out_indptr) return fail(who, "indptr / out_indptr are null");
  if (nnz > 0 && (!src || !eids || !out_src || !out_eids)) return fail(who, "src / eids / out_src / out_eids are null");
  if (n_x > 0 && !x) return fail(who, "x is null");
  return 0;
}

int check_compact(const char* who, int idtype_bits, const void* preserve, int64_t np, const void* ends, int64_t ne,
                  int64_t num_nodes, const void* local, const void* nodes, const void* num_out, const void* flags) {
  if (!idbits_ok(idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (np < 0 || ne < 0 || num_nodes < 0) return fail(who, "negative size");
  if (np + ne >= (int64_t(1) << 31)) return fail(who, "preserve and ends together must stay below 2^31 ids (local ids are int32)");
  if (idtype_bits == 32 && num_nodes > INT32_MAX) return fail(who, "num_nodes does not fit the id type");
  if (np > 0 && !preserve) return fail(who, "preserve is null");
  if (ne > 0 && (!ends || !local)) return fail(who, "ends / local are null");
  if (np + ne > 0 && !nodes) return fail(who, "nodes is null");
  if (!num_out || !flags) return fail(who, "num_out / flags are null");
  return 0;
}

// ---- the rules run by the CPU -----------------------------------------------------------------------
template <typename Idx>
void exclude_set_host(const Idx* ids, const Idx* rev, int64_t n, int64_t num_edges, Idx* out, int32_t* flags) {
  const int64_t m = rev ? 2 * n : n;
  int32_t fl = 0;
  for (int64_t k = 0; k < m; ++k) {
    bool bad;
    out[k] = static_cast<Idx>(exclude_slot(ids, rev, n, num_edges, k, &bad));
    if (bad) fl |= kExcludeOutOfRange;
  }
  std::sort(out, out + m);
  *flags = fl;
}

template <typename Idx>
void frontier_exclude_host(const Idx* indptr, const Idx* src, const Idx* eids, int64_t nr, int64_t nnz, const Idx* x,
                           int64_t n_x, Idx* out_indptr, Idx* out_src, Idx* out_eids) {
  int64_t at = 0;
  for (int64_t i = 0; i < nr; ++i) {
    out_indptr[i] = static_cast<Idx>(at);
    int64_t lo, hi;
    exclude_row(indptr, nnz, i, &lo, &hi);
    for (int64_t j = lo; j < hi; ++j) {
      if (exclude_member(x, n_x, static_cast<int64_t>(eids[j]))) continue;
      if (at < nnz) out_src[at] = src[j], out_eids[at] = eids[j];
      ++at;
    }
  }
  out_indptr[nr] = static_cast<Idx>(at);
}

template <typename Idx>
void compact_nodes_host(const Idx* preserve, int64_t np, const Idx* ends, int64_t ne, int64_t num_nodes, Idx* local,
                        Idx* nodes, int64_t* num_out, int32_t* flags) {
  std::vector<int32_t> map(static_cast<size_t>(num_nodes), -1);
  int32_t fl = 0;
  int64_t k = 0;
  for (int64_t i = 0; i < np; ++i) {
    const int64_t v = static_cast<int64_t>(preserve[i]);
    if (v < 0 || v >= num_nodes) {
      fl |= kExcludeOutOfRange;
    } else if (map[v] < 0) {
      map[v] = static_cast<int32_t>(k);
      nodes[k++] = preserve[i];
    }
  }
  std::vector<Idx> sorted(static_cast<size_t>(ne));
  for (int64_t e = 0; e < ne; ++e) {
    const int64_t v = static_cast<int64_t>(ends[e]);
    const bool inside = v >= 0 && v < num_nodes;
    sorted[e] = static_cast<Idx>(inside ? v : num_nodes);
    if (!inside) fl |= kExcludeOutOfRange;
  }
  std::sort(sorted.begin(), sorted.end());
  std::vector<int64_t> heads;
  for (int64_t i = 0; i < ne; ++i)
    if (compact_head(sorted.data(), map.data(), num_nodes, i)) heads.push_back(i);
  for (int64_t i : heads) {
    map[static_cast<int64_t>(sorted[i])] = static_cast<int32_t>(k);
    nodes[k++] = sorted[i];
  }
  for (int64_t e = 0; e < ne; ++e) {
    const int64_t v = static_cast<int64_t>(ends[e]);
    local[e] = static_cast<Idx>(v >= 0 && v < num_nodes ? map[v] : -1);
  }
  *num_out = k;
  *flags = fl;
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_exclude_set_workspace_bytes(int idtype_bits, int64_t n, int with_reverse) {
  if (!idbits_ok(idtype_bits) || n < 0 || n >= (int64_t(1) << 30)) return 0;
  return set_layout(idtype_bits, with_reverse ? 2 * n : n).bytes;
}

int dgla_exclude_set(int idtype_bits, const void* ids, int64_t n, const void* rev, int64_t num_edges, void* out,
                     int32_t* flags, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "exclude_set";
  if (check_set(who, idtype_bits, ids, n, num_edges, out, flags)) return -1;
  if (n == 0) return 0;
  const int64_t m = rev ? 2 * n : n;
  const SetLayout L = set_layout(idtype_bits, m);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  Scratch ws(s);
  if (ws.take(workspace, workspace_bytes, L.bytes)) return -1;
  int rc = 0;
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    Idx* keys = reinterpret_cast<Idx*>(ws.p + L.keys);
    hipLaunchKernelGGL(exclude_slots_kernel<Idx>, dim3(grid1(m, kExBlock)), dim3(kExBlock), 0, s, static_cast<const Idx*>(ids),
                       static_cast<const Idx*>(rev), n, m, num_edges, keys, flags);
    rc = msd::sort_keys<Idx>(keys, static_cast<Idx*>(out), m, key_bits_for(num_edges), ws.p + L.sort, s);
  });
  if (rc) return -1;
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_exclude_set_host(int idtype_bits, const void* ids, int64_t n, const void* rev, int64_t num_edges, void* out,
                          int32_t* flags) {
  if (check_set("exclude_set_host", idtype_bits, ids, n, num_edges, out, flags)) return -1;
  *flags = 0;
  if (n == 0) return 0;
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    exclude_set_host<Idx>(static_cast<const Idx*>(ids), static_cast<const Idx*>(rev), n, num_edges, static_cast<Idx*>(out), flags);
  });
  return 0;
}

size_t dgla_frontier_exclude_workspace_bytes(int idtype_bits, int64_t num_rows, int64_t nnz) {
  if (!idbits_ok(idtype_bits) || num_rows < 0 || num_rows >= (int64_t(1) << 31) || nnz < 0) return 0;
  return filter_layout(num_rows, nnz).bytes;
}

int dgla_frontier_exclude(int idtype_bits, const void* indptr, const void* src, const void* eids, int64_t num_rows,
                          int64_t nnz, const void* x, int64_t n_x, void* out_indptr, void* out_src, void* out_eids,
                          void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "frontier_exclude";
  if (check_filter(who, idtype_bits, indptr, src, eids, num_rows, nnz, x, n_x, out_indptr, out_src, out_eids)) return -1;
  const bool sweep = num_rows > 0 && nnz > 0;
  const FilterLayout L = filter_layout(num_rows, nnz);
  if (sweep && optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_indptr);
  Scratch ws(s);
  if (sweep && ws.take(workspace, workspace_bytes, L.bytes)) return -1;
  int rc = 0;
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    int64_t* offs = sweep ? reinterpret_cast<int64_t*>(ws.p + L.offs) : nullptr;
    if (sweep) {
      uint8_t* keep = reinterpret_cast<uint8_t*>(ws.p + L.keep);
      auto run = [&](auto g) {
        constexpr int G = decltype(g)::value;
        const dim3 grid(grid1(num_rows, kExBlock / G)), block(kExBlock);
        hipLaunchKernelGGL((exclude_sweep_kernel<Idx, G, false>), grid, block, 0, s, static_cast<const Idx*>(indptr),
                           static_cast<const Idx*>(src), static_cast<const Idx*>(eids), num_rows, nnz, static_cast<const Idx*>(x),
                           n_x, keep, offs, static_cast<Idx*>(nullptr), static_cast<Idx*>(nullptr));
        rc = msd::exclusive_scan<int64_t, int64_t>(offs, offs, num_rows + 1, ws.p + L.scan, s);
        if (rc) return;
        hipLaunchKernelGGL((exclude_sweep_kernel<Idx, G, true>), grid, block, 0, s, static_cast<const Idx*>(indptr),
                           static_cast<const Idx*>(src), static_cast<const Idx*>(eids), num_rows, nnz, static_cast<const Idx*>(x),
                           n_x, keep, offs, static_cast<Idx*>(out_src), static_cast<Idx*>(out_eids));
      };
      if (exclude_group(num_rows, nnz) == 16)
        run(std::integral_constant<int, 16>{});
      else
        run(std::integral_constant<int, 64>{});
    }
    if (rc) return;
    hipLaunchKernelGGL(exclude_indptr_kernel<Idx>, dim3(grid1(num_rows + 1, kExBlock)), dim3(kExBlock), 0, s, offs, num_rows,
                       static_cast<Idx*>(out_indptr));
  });
  if (rc) return -1;
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_frontier_exclude_host(int idtype_bits, const void* indptr, const void* src, const void* eids, int64_t num_rows,
                               int64_t nnz, const void* x, int64_t n_x, void* out_indptr, void* out_src, void* out_eids) {
  if (check_filter("frontier_exclude_host", idtype_bits, indptr, src, eids, num_rows, nnz, x, n_x, out_indptr, out_src,
                   out_eids))
    return -1;
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    frontier_exclude_host<Idx>(static_cast<const Idx*>(indptr), static_cast<const Idx*>(src), static_cast<const Idx*>(eids),
                               num_rows, nnz, static_cast<const Idx*>(x), n_x, static_cast<Idx*>(out_indptr),
                               static_cast<Idx*>(out_src), static_cast<Idx*>(out_eids));
  });
  return 0;
}

size_t dgla_compact_nodes_workspace_bytes(int idtype_bits, int64_t n_preserve, int64_t n_ends) {
  if (!sizes_ok(idtype_bits, n_preserve, n_ends) || n_preserve + n_ends >= (int64_t(1) << 31)) return 0;
  return compact_layout(idtype_bits, n_preserve, n_ends).bytes;
}

int dgla_compact_nodes(int idtype_bits, const void* preserve, int64_t n_preserve, const void* ends, int64_t n_ends,
                       int32_t* node_map, int64_t num_nodes, void* local, void* nodes, int64_t* num_out, int32_t* flags,
                       void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "compact_nodes";
  if (check_compact(who, idtype_bits, preserve, n_preserve, ends, n_ends, num_nodes, local, nodes, num_out, flags)) return -1;
  if (num_nodes > 0 && !node_map) return fail(who, "node_map is null");
  const int64_t np = n_preserve, ne = n_ends;
  const CompactLayout L = compact_layout(idtype_bits, np, ne);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, num_out);
  Scratch ws(s);
  if (ws.take(workspace, workspace_bytes, L.bytes)) return -1;
  int rc = 0;
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const Idx *pre = static_cast<const Idx*>(preserve), *end = static_cast<const Idx*>(ends);
    Idx *nod = static_cast<Idx*>(nodes), *keys = reinterpret_cast<Idx*>(ws.p + L.keys),
        *sorted = reinterpret_cast<Idx*>(ws.p + L.sorted);
    int64_t *offs_p = reinterpret_cast<int64_t*>(ws.p + L.offs_p), *offs_e = reinterpret_cast<int64_t*>(ws.p + L.offs_e);
    const dim3 block(kExBlock);
    if (np > 0) {
      const dim3 gp(grid1(np + 1, kExBlock));
      hipLaunchKernelGGL((compact_preserve_kernel<Idx, 0>), gp, block, 0, s, pre, np, node_map, num_nodes, offs_p, flags);
      hipLaunchKernelGGL((compact_preserve_kernel<Idx, 1>), gp, block, 0, s, pre, np, node_map, num_nodes, offs_p, flags);
      rc = msd::exclusive_scan<int64_t, int64_t>(offs_p, offs_p, np + 1, ws.p + L.scan_p, s);
      if (rc) return;
      hipLaunchKernelGGL(compact_preserve_assign_kernel<Idx>, gp, block, 0, s, pre, np, offs_p, node_map, nod);
    }
    if (ne > 0) {
      const dim3 ge(grid1(ne + 1, kExBlock));
      hipLaunchKernelGGL(compact_keys_kernel<Idx>, ge, block, 0, s, end, ne, num_nodes, keys, flags);
      rc = msd::sort_keys<Idx>(keys, sorted, ne, key_bits_for(num_nodes), ws.p + L.sort, s);
      if (rc) return;
      hipLaunchKernelGGL(compact_heads_kernel<Idx>, ge, block, 0, s, sorted, ne, node_map, num_nodes, offs_e);
      rc = msd::exclusive_scan<int64_t, int64_t>(offs_e, offs_e, ne + 1, ws.p + L.scan_e, s);
      if (rc) return;
    }
    // (also the launch that writes *num_out when there are no end points)
    hipLaunchKernelGGL(compact_heads_assign_kernel<Idx>, dim3(grid1(ne, kExBlock)), block, 0, s, sorted, ne,
                       ne > 0 ? offs_e : nullptr, np > 0 ? offs_p + np : nullptr, np + ne, node_map, nod, num_out);
    if (ne > 0) {
      hipLaunchKernelGGL((compact_lookup_kernel<Idx, 0>), dim3(grid1(ne, kExBlock)), block, 0, s, end, ne, node_map, num_nodes,
                         static_cast<Idx*>(local));
      hipLaunchKernelGGL((compact_lookup_kernel<Idx, 1>), dim3(grid1(ne, kExBlock)), block, 0, s, end, ne, node_map, num_nodes,
                         static_cast<Idx*>(nullptr));
    }
    if (np > 0)
      hipLaunchKernelGGL((compact_lookup_kernel<Idx, 1>), dim3(grid1(np, kExBlock)), block, 0, s, pre, np, node_map, num_nodes,
                         static_cast<Idx*>(nullptr));
  });
  if (rc) return -1;
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_compact_nodes_host(int idtype_bits, const void* preserve, int64_t n_preserve, const void* ends, int64_t n_ends,
                            int64_t num_nodes, void* local, void* nodes, int64_t* num_out, int32_t* flags) {
  if (check_compact("compact_nodes_host", idtype_bits, preserve, n_preserve, ends, n_ends, num_nodes, local, nodes, num_out,
                    flags))
    return -1;
  with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    compact_nodes_host<Idx>(static_cast<const Idx*>(preserve), n_preserve, static_cast<const Idx*>(ends), n_ends, num_nodes,
                            static_cast<Idx*>(local), static_cast<Idx*>(nodes), num_out, flags);
  });
  return 0;
}

}  // extern "C"
