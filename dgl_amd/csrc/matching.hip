// Graph coarsening on the device: dgl.geometry.neighbor_matching, the edge-coarsening step of Graclus pooling and of
// multilevel (Metis) partitioning.
//
// Reference: NeighborMatching<kDGLCUDA> (src/geometry/cuda/edge_coarsening_impl.cu): a colour / propose / respond loop
// with one thread per node, colours and an E-sized array of random weights written to memory and read again, `result`
// read while the same kernel writes it (the output depends on thread timing), and a flag read back by the host in every
// round; a CSR that is not symmetric never ends.
//
// MI355X-first choices:
//  * The rule is the one of csrc/matching_step.h, compiled here for the kernels and for dgla_neighbor_matching_host.
//    Colours and tie-breaking hashes are counter-based functions of (seed, ids, round) computed in registers: no
//    colour array, no random-weight array.  Propose reads label and writes prop, respond reads prop and writes label,
//    so no phase reads what it writes (the one exception is argued in the step header) and the labels are a pure
//    function of (CSR, weights, seed, max_rounds), whatever the launch geometry and the thread timing.
//  * A workgroup owns 256 consecutive nodes.  Each lane tests ONE node (a coalesced read of label; in respond also
//    prop and the colour), and a ballot and popcount per wavefront compact the rows that have to stream into an LDS
//    list: an inactive row costs that one lane and touches neither indptr nor indices.  (One group per node, active
//    or not, made a round in which nothing is active cost 0.26 ms on 2.4 M nodes; compaction inside the workgroup
//    needs no global scan and no further launch: DESIGN.md 3.17.)  A GROUP of G lanes (G = 16 or 64 from the mean
//    degree, as csrc/labor.hip) then takes the listed rows in turn and streams each with coalesced loads of
//    `indices`; every entry costs ONE gather (label[v] in propose, prop[v] in respond) through pointers that name
//    the global address space.  The weight and its edge id are read only for the entries that are candidates (active
//    RED neighbours of a BLUE row; proposers of a RED row).  The group's best key (w', h, v) is found by an xor
//    butterfly.  A RED row leaves propose at its first active neighbour.
//  * No atomics; every store is a plain vector store.  label[u] and prop[u] have one writer per phase, except
//    label[v] of a matched BLUE v, whose one writer is the RED row that picked it.
//  * Termination: every workgroup with an active row in round t stores t + 1 into one device word (the same value
//    from every writer of a launch, launches in stream order).  The host queues `batch_rounds` rounds, reads that
//    word back and stops when it is below the rounds queued.  A round after the last node matched finds every row inactive, so the batch size
//    never changes a result, and the word is the number of rounds used.
//  * Relabelling: flag label[i] == i, the library's exclusive scan (csrc/sort.hip.h), new[i] = scan[label[i]].  Nothing
//    is read back.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "matching_step.h"
#include "sort.hip.h"

namespace dgla {
namespace {

constexpr int kMatchBlock = 256;         // threads per workgroup, and the nodes it owns
constexpr int64_t kMatchShortMean = 32;  // mean degree up to which a row gets 16 lanes
constexpr int64_t kMatchBatch = 8;       // rounds per read-back when the caller names none

int match_group(const dgla_csr* c) {
  const int64_t rows = c->num_rows > 0 ? c->num_rows : 1;
  return c->nnz / rows <= kMatchShortMean ? 16 : 64;
}

// the best key of the group, the same bits in every lane
template <int G>
__device__ __forceinline__ MatchKey group_best(MatchKey k) {
#pragma unroll
  for (int s = G / 2; s >= 1; s >>= 1) {
    MatchKey o;
    o.w = __shfl_xor(k.w, s, G);
    o.h = static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(k.h), s, G));
    o.v = static_cast<int64_t>(__shfl_xor(static_cast<long long>(k.v), s, G));
    if (match_better(o, k)) k = o;
  }
  return k;
}

template <int G>
__device__ __forceinline__ bool group_any(bool p, int lane) {
  const uint64_t b = __ballot(p);
  if constexpr (G == 64) {
    return b != 0;
  } else {
    return ((b >> (lane & ~(G - 1))) & ((uint64_t(1) << G) - 1)) != 0;
  }
}

template <typename Idx>
__global__ __launch_bounds__(kMatchBlock) void matching_init_kernel(Idx* __restrict__ label, Idx* __restrict__ prop, int64_t n,
                                                                    int64_t* __restrict__ used) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kMatchBlock) + threadIdx.x;
  if (i < n) label[i] = Idx(-1), prop[i] = static_cast<Idx>(kMatchNone);
  if (i == 0) *used = 0;
}

// The rows of this workgroup's 256 consecutive nodes that `take` selects, compacted in node order into list[] (the
// offset inside the workgroup): a ballot and a popcount per wavefront, the four counts exchanged through LDS.  Returns
// their number.  An unselected row costs its one lane here and nothing else: no group is spent on it.
__device__ __forceinline__ int block_compact(bool take, int* list, int* wcnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t bal = __ballot(take);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kMatchBlock / 64; ++w) {
    if (w < wave) base += wcnt[w];
    total += wcnt[w];
  }
  if (take) list[base + __popcll(bal & ((uint64_t(1) << lane) - 1))] = threadIdx.x;
  __syncthreads();
  return total;
}

// ---- propose ----------------------------------------------------------------------------------------
template <typename Idx, typename W, bool WEIGHTED, int G>
__global__ __launch_bounds__(kMatchBlock) void matching_propose_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                       const Idx* __restrict__ data, const W* __restrict__ weight,
                                                                       const Idx* __restrict__ label, Idx* __restrict__ prop,
                                                                       int64_t n, uint64_t seed, int64_t t,
                                                                       int64_t* __restrict__ used) {
  __shared__ int list[kMatchBlock];
  __shared__ int wcnt[kMatchBlock / 64];
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t row0 = blockIdx.x * static_cast<int64_t>(kMatchBlock);
  gptr<Idx> lab = (gptr<Idx>)label;
  gptr<Idx> ptr = (gptr<Idx>)indptr;
  const int64_t mine = row0 + threadIdx.x;
  const int total = block_compact(mine < n && lab[mine] < 0, list, wcnt);  // inactive rows: no row traffic
  if (total == 0) return;
  if (threadIdx.x == 0) *used = t + 1;  // (every writer of this launch stores the same value)
  for (int k = threadIdx.x / G; k < total; k += kMatchBlock / G) {  // a group of G lanes per active row
    const int64_t u = row0 + list[k];
    const int64_t lo = static_cast<int64_t>(ptr[u]), hi = static_cast<int64_t>(ptr[u + 1]);
    const bool blue = match_is_blue(seed, u, t);
    bool any = false;
    MatchKey best = match_no_key();
    for (int64_t base = lo; base < hi; base += G) {
      const int64_t q = base + lg;
      if (q < hi) {
        MatchKey key;
        const int st = match_propose_entry<WEIGHTED>((gptr<Idx>)indices, (gptr<Idx>)data, (gptr<W>)weight, lab, n, seed, t, u,
                                                     blue, q, &key);
        any = any || st >= 1;
        if (st == 2 && match_better(key, best)) best = key;
      }
      if (!blue && group_any<G>(any, lane)) break;  // a RED row only asks whether an active neighbour exists
    }
    any = group_any<G>(any, lane);
    if (blue) best = group_best<G>(best);
    if (lg == 0) prop[u] = static_cast<Idx>(match_proposal(any, blue, best));
  }
}

// ---- respond ----------------------------------------------------------------------------------------
template <typename Idx, typename W, bool WEIGHTED, int G>
__global__ __launch_bounds__(kMatchBlock) void matching_respond_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                       const Idx* __restrict__ data, const W* __restrict__ weight,
                                                                       const Idx* __restrict__ prop, Idx* label, int64_t n,
                                                                       uint64_t seed, int64_t t) {
  __shared__ int list[kMatchBlock];
  __shared__ int wcnt[kMatchBlock / 64];
  const int lg = threadIdx.x & (G - 1);
  const int64_t row0 = blockIdx.x * static_cast<int64_t>(kMatchBlock);
  gptr<Idx> pr = (gptr<Idx>)prop;
  gptr<Idx> ptr = (gptr<Idx>)indptr;
  const int64_t mine = row0 + threadIdx.x;
  // (label[mine] of a BLUE node may be written by the RED row that picks it while it is read here: a BLUE node whose
  // prop is not kMatchSingle does nothing either way)
  bool red = false;
  if (mine < n && label[mine] < 0) {
    if (static_cast<int64_t>(pr[mine]) == kMatchSingle) label[mine] = static_cast<Idx>(mine);
    else red = !match_is_blue(seed, mine, t);
  }
  const int total = block_compact(red, list, wcnt);  // only the active RED rows with an active neighbour stream
  for (int k = threadIdx.x / G; k < total; k += kMatchBlock / G) {
    const int64_t u = row0 + list[k];
    const int64_t lo = static_cast<int64_t>(ptr[u]), hi = static_cast<int64_t>(ptr[u + 1]);
    MatchKey best = match_no_key();
    for (int64_t q = lo + lg; q < hi; q += G) {
      MatchKey key;
      if (match_respond_entry<WEIGHTED>((gptr<Idx>)indices, (gptr<Idx>)data, (gptr<W>)weight, pr, n, seed, u, q, &key) &&
          match_better(key, best))
        best = key;
    }
    best = group_best<G>(best);
    if (lg == 0 && best.v >= 0) {  // best.v passed the range test of match_respond_entry
      const Idx m = static_cast<Idx>(u < best.v ? u : best.v);
      label[u] = m;
      label[best.v] = m;
    }
  }
}

// *used = max_rounds + 1 when a node is still active after the last round
template <typename Idx>
__global__ __launch_bounds__(kMatchBlock) void matching_left_kernel(const Idx* __restrict__ label, int64_t n, int64_t over,
                                                                    int64_t* __restrict__ used) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kMatchBlock) + threadIdx.x;
  if (i < n && label[i] < 0) *used = over;
}

// ---- relabel ----------------------------------------------------------------------------------------
template <typename Idx>
__global__ __launch_bounds__(kMatchBlock) void matching_flag_kernel(const Idx* __restrict__ label, int64_t n, Idx* __restrict__ flag) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kMatchBlock) + threadIdx.x;
  if (i < n) flag[i] = label[i] == static_cast<Idx>(i) ? Idx(1) : Idx(0);
}

template <typename Idx>
__global__ __launch_bounds__(kMatchBlock) void matching_relabel_kernel(const Idx* __restrict__ label, const Idx* __restrict__ rank,
                                                                       int64_t n, Idx* __restrict__ out) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kMatchBlock) + threadIdx.x;
  if (i >= n) return;
  const int64_t l = static_cast<int64_t>(label[i]);
  out[i] = l >= 0 && l < n ? ((gptr<Idx>)rank)[l] : Idx(-1);
}

// ---- host side --------------------------------------------------------------------------------------
struct MatchLayout {  // one workspace for dgla_neighbor_matching (prop, used) and dgla_neighbor_matching_relabel (ids, scan)
  size_t ids, used, scan, bytes;
};

MatchLayout match_layout(int idbits, int64_t n) {
  MatchLayout L{};
  Carver c;
  L.ids = c.take(static_cast<size_t>(idbits / 8) * static_cast<size_t>(n));  // prop of the loop, the flags / ranks of relabel
  L.used = c.take(sizeof(int64_t));
  L.scan = c.take(msd::scan_temp_bytes(n, static_cast<size_t>(idbits / 8)));
  L.bytes = c.bytes();
  return L;
}

// everything dgla_neighbor_matching and dgla_neighbor_matching_host refuse
int check_matching(const char* who, const dgla_csr* csr, const void* weight, int weight_dtype, int64_t max_rounds,
                   const void* label, const int64_t* rounds) {
  if (check_csr(who, csr)) return -1;
  if (weight && (weight_dtype == kF16 || weight_dtype == kBF16))
    return fail(who, "float16 / bfloat16 weights are not supported; use float32 or float64");
  if (weight && weight_dtype != kF32 && weight_dtype != kF64) return fail(who, "unknown weight dtype " + std::to_string(weight_dtype));
  if (max_rounds < 1) return fail(who, "max_rounds must be at least 1, got " + std::to_string(max_rounds));
  if (csr->num_rows > 0 && !label) return fail(who, "label is null");
  if (!rounds) return fail(who, "rounds is null");
  return 0;
}

int check_relabel(const char* who, const void* label, int idbits, int64_t n, const void* out) {
  if (!idbits_ok(idbits)) return fail(who, "idtype must be int32 or int64");
  if (n < 0) return fail(who, "negative size");
  if (n > 0 && (!label || !out)) return fail(who, "label / out are null");
  return 0;
}

int cap_reached(const char* who, int64_t max_rounds) {
  return fail(who, "nodes are still unmatched after max_rounds = " + std::to_string(max_rounds) +
                       " rounds; the graph is probably not bi-directed (a CSR that is not symmetric can cycle for ever)");
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
// returns the rounds used, or -1 when nodes are left at the cap
template <typename Idx, typename W, bool WEIGHTED>
int64_t matching_host(const TypedCsr<Idx>& g, const W* weight, uint64_t seed, int64_t max_rounds, Idx* label) {
  const int64_t n = g.num_rows;
  const Idx *indptr = g.indptr, *indices = g.indices, *data = g.data;
  std::vector<Idx> prop(n, static_cast<Idx>(kMatchNone));
  for (int64_t i = 0; i < n; ++i) label[i] = Idx(-1);
  for (int64_t t = 0;; ++t) {
    bool active = false;
    for (int64_t u = 0; u < n && !active; ++u) active = label[u] < 0;
    if (!active) return t;
    if (t == max_rounds) return -1;
    for (int64_t u = 0; u < n; ++u) {  // propose
      if (label[u] >= 0) continue;
      const bool blue = match_is_blue(seed, u, t);
      bool any = false;
      MatchKey best = match_no_key();
      for (int64_t q = indptr[u]; q < indptr[u + 1]; ++q) {
        MatchKey k;
        const int st = match_propose_entry<WEIGHTED>(indices, data, weight, label, n, seed, t, u, blue, q, &k);
        any = any || st >= 1;
        if (st == 2 && match_better(k, best)) best = k;
      }
      prop[u] = static_cast<Idx>(match_proposal(any, blue, best));
    }
    for (int64_t u = 0; u < n; ++u) {  // respond
      if (label[u] >= 0) continue;
      if (prop[u] == static_cast<Idx>(kMatchSingle)) {
        label[u] = static_cast<Idx>(u);
        continue;
      }
      if (match_is_blue(seed, u, t)) continue;
      MatchKey best = match_no_key();
      for (int64_t q = indptr[u]; q < indptr[u + 1]; ++q) {
        MatchKey k;
        if (match_respond_entry<WEIGHTED>(indices, data, weight, prop.data(), n, seed, u, q, &k) && match_better(k, best))
          best = k;
      }
      if (best.v >= 0) label[u] = label[best.v] = static_cast<Idx>(u < best.v ? u : best.v);
    }
  }
}

template <typename Idx>
void relabel_host(const Idx* label, int64_t n, Idx* out) {
  std::vector<Idx> rank(n);
  Idx run = 0;
  for (int64_t i = 0; i < n; ++i) rank[i] = run, run += label[i] == static_cast<Idx>(i) ? 1 : 0;
  for (int64_t i = 0; i < n; ++i) out[i] = label[i] >= 0 && label[i] < n ? rank[label[i]] : Idx(-1);
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_neighbor_matching_workspace_bytes(int idtype_bits, int64_t num_nodes) {
  if (!idbits_ok(idtype_bits) || num_nodes <= 0) return 0;
  return match_layout(idtype_bits, num_nodes).bytes;
}

int dgla_neighbor_matching(const dgla_csr* csr, const void* weight, int weight_dtype, uint64_t seed, int64_t max_rounds,
                           int64_t batch_rounds, void* label, int64_t* rounds, void* workspace, size_t workspace_bytes,
                           void* hip_stream) {
  const char* who = "neighbor_matching";
  if (check_matching(who, csr, weight, weight_dtype, max_rounds, label, rounds)) return -1;
  *rounds = 0;
  const int64_t n = csr->num_rows;
  if (n == 0) return 0;
  const MatchLayout L = match_layout(csr->idtype_bits, n);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, label);
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  int64_t* used = reinterpret_cast<int64_t*>(scratch.p + L.used);
  const int64_t batch = batch_rounds >= 1 ? batch_rounds : kMatchBatch;
  int64_t done = 0;
  const int rc = with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    Idx* lab = static_cast<Idx*>(label);
    Idx* prop = reinterpret_cast<Idx*>(scratch.p + L.ids);
    hipLaunchKernelGGL(matching_init_kernel<Idx>, dim3(grid1(n, kMatchBlock)), dim3(kMatchBlock), 0, s, lab, prop, n, used);
    return with_weight(weight, weight_dtype, [&](auto wtag, auto weighted) -> int {
      using W = decltype(wtag);
      constexpr bool WEIGHTED = decltype(weighted)::value;
      auto run = [&](auto grp) -> int {
        constexpr int G = decltype(grp)::value;
        const dim3 grid(grid1(n, kMatchBlock)), block(kMatchBlock);
        const TypedCsr<Idx> g(csr);
        const Idx *indptr = g.indptr, *indices = g.indices, *data = g.data;
        const W* wt = static_cast<const W*>(weight);
        int64_t queued = 0;
        while (queued < max_rounds) {
          const int64_t end = queued + batch < max_rounds ? queued + batch : max_rounds;
          for (int64_t t = queued; t < end; ++t) {
            hipLaunchKernelGGL((matching_propose_kernel<Idx, W, WEIGHTED, G>), grid, block, 0, s, indptr, indices, data, wt, lab,
                               prop, n, seed, t, used);
            hipLaunchKernelGGL((matching_respond_kernel<Idx, W, WEIGHTED, G>), grid, block, 0, s, indptr, indices, data, wt, prop,
                               lab, n, seed, t);
          }
          queued = end;
          if (queued == max_rounds)  // the cap: are nodes left?
            hipLaunchKernelGGL(matching_left_kernel<Idx>, dim3(grid1(n, kMatchBlock)), dim3(kMatchBlock), 0, s, lab, n,
                               max_rounds + 1, used);
          if (read_back(&done, used, sizeof(int64_t), s)) return -1;  // the one read-back of a batch
          if (done < queued) break;  // the last queued round found no active node
        }
        return 0;
      };
      if (match_group(csr) == 16) return run(std::integral_constant<int, 16>{});
      return run(std::integral_constant<int, 64>{});
    });
  });
  if (rc) return -1;
  if (done > max_rounds) return cap_reached(who, max_rounds);
  *rounds = done;
  return 0;
}

int dgla_neighbor_matching_relabel(const void* label, int idtype_bits, int64_t num_nodes, void* out, void* workspace,
                                   size_t workspace_bytes, void* hip_stream) {
  const char* who = "neighbor_matching_relabel";
  if (check_relabel(who, label, idtype_bits, num_nodes, out)) return -1;
  const int64_t n = num_nodes;
  if (n == 0) return 0;
  const MatchLayout L = match_layout(idtype_bits, n);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  return with_idx(idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    const Idx* lab = static_cast<const Idx*>(label);
    Idx* rank = reinterpret_cast<Idx*>(scratch.p + L.ids);
    const dim3 grid(grid1(n, kMatchBlock)), block(kMatchBlock);
    hipLaunchKernelGGL(matching_flag_kernel<Idx>, grid, block, 0, s, lab, n, rank);
    if (msd::exclusive_scan<Idx, Idx>(rank, rank, n, scratch.p + L.scan, s)) return -1;
    hipLaunchKernelGGL(matching_relabel_kernel<Idx>, grid, block, 0, s, lab, rank, n, static_cast<Idx*>(out));
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

int dgla_neighbor_matching_host(const dgla_csr* csr, const void* weight, int weight_dtype, uint64_t seed, int64_t max_rounds,
                                void* label, int64_t* rounds, void* relabel) {
  if (check_matching("neighbor_matching_host", csr, weight, weight_dtype, max_rounds, label, rounds)) return -1;
  *rounds = 0;
  const int64_t used = with_idx(csr->idtype_bits, [&](auto tag) -> int64_t {
    using Idx = decltype(tag);
    return with_weight(weight, weight_dtype, [&](auto wtag, auto weighted) -> int64_t {
      using W = decltype(wtag);
      return matching_host<Idx, W, decltype(weighted)::value>(TypedCsr<Idx>(csr), static_cast<const W*>(weight), seed,
                                                              max_rounds, static_cast<Idx*>(label));
    });
  });
  if (used < 0) return cap_reached("neighbor_matching_host", max_rounds);
  *rounds = used;
  if (relabel) {
    with_idx(csr->idtype_bits, [&](auto tag) {
      using Idx = decltype(tag);
      relabel_host<Idx>(static_cast<const Idx*>(label), csr->num_rows, static_cast<Idx*>(relabel));
    });
  }
  return 0;
}

}  // extern "C"
