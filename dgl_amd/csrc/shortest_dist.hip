// Shortest distances and paths on the device: dgl.shortest_dist, what the SpatialEncoder / PathEncoder of a graph
// transformer consume (the hop distance of every pair of nodes and one shortest path per pair).
//
// Reference: python/dgl/transforms/functional.py shortest_dist copies the graph to the host, runs scipy's shortest_path
// / dijkstra there, rebuilds every path in a Python double loop over the pairs and asks edge_ids for the edges.  There is
// no GPU kernel.
//
// MI355X-first choices (the rule: csrc/shortest_dist_step.h):
//  * Bit-parallel multi-source BFS.  64 sources share one 64-bit word per node, so one OR per in-edge advances 64
//    searches; S sources are W = ceil(S / 64) independent words.  ONE workgroup of 256 threads owns a word and runs its
//    search from the first level to the last: words never interact, so there is no grid-wide synchronisation and no
//    host round trip per level.
//  * The three mask arrays of a search (frontier, next, seen: n words each) live in LDS up to kSdLdsNodes nodes
//    (3 x 8 x 6400 = 153 600 of gfx950's 163 840 bytes; a word has at most n / 64 <= 100 workgroups then, fewer than the
//    device has CUs, so one workgroup per CU costs nothing).  Above it, or when the device grants less LDS, they live
//    in the workgroup's own slice of the workspace.
//  * A level is a PULL over the in-edge CSR: new[v] = OR of frontier[u] over the in-neighbours, minus seen[v].  One lane
//    takes one row of up to kSdLongRow entries; a longer row is streamed by the whole wavefront with a wave-wide OR, so
//    a hub does not serialise a lane.  A node whose seen word holds every valid source bit skips its row.
//  * dist is written while the wave holds 64 consecutive v: the wave ORs its lanes' new masks, walks the set bits of
//    the union, and for each bit the lanes that own it store the level to dist[64 w + b][v], runs of consecutive
//    addresses along v.  At the end the bits seen[v] lacks get -1.  Every element of dist is written exactly once and no
//    fill pass precedes the kernel.
//  * The level loop ends when no lane found a new bit (one workgroup-wide OR, __syncthreads_or) and after at most n - 1
//    levels whatever the input holds.  Every barrier sits in workgroup-uniform control flow.
//  * Predecessor edges: one lane per (s, v), lanes along v; the lane scans the in-row of v, gathers dist[s][u] inside one
//    row of dist and keeps the smallest qualifying edge id with its u, one 2-id table entry per pair.
//  * Paths: each lane walks its (s, v) back through the table into an LDS tile [lane][k]; paths[s][v .. v + 64)[0 .. L)
//    is one contiguous span, which the wave writes as one coalesced stream, the -1 padding included.  Paths longer than
//    kSdChunk steps go through the tile in chunks, last chunk first (the walk starts at v).
#include "../../include/dgl_amd.h"

#include <algorithm>
#include <string>
#include <vector>

#include "host_util.h"
#include "shortest_dist_step.h"

namespace dgla {
namespace {

constexpr int kSdBlock = 256;        // threads per workgroup, 4 wavefronts
constexpr int kSdLdsNodes = 6400;    // nodes up to which the masks of a search live in LDS
constexpr int kSdLongRow = 64;       // a row with more entries is streamed by the wavefront
constexpr int kSdChunk = 16;         // path steps per pass through the LDS tile
constexpr int kSdTileRow = kSdChunk + 1;  // (an odd row length in 8-byte words: the lanes' rows start in different banks)

__device__ __forceinline__ uint64_t wave_or(uint64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(x), o));
  return x;
}

// a value every lane holds, moved to scalar registers
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The wave holds 64 consecutive v; lane's `bits` names the sources whose dist[.][v] becomes `value` (0 for a lane
// past n).  Called by whole wavefronts.
__device__ __forceinline__ void sd_store_bits(int64_t* __restrict__ dist, int64_t n, int64_t s0, int64_t v, uint64_t bits,
                                              int64_t value) {
  uint64_t uni = uniform64(wave_or(bits));
  while (uni) {
    const int b = __builtin_ctzll(uni);
    uni &= uni - 1;
    if ((bits >> b) & 1) dist[(s0 + b) * n + v] = value;
  }
}

// frontier[u] of entry q, 0 for an entry outside [0, n)
template <typename Idx>
__device__ __forceinline__ uint64_t sd_pull(gptr<Idx> indices, const uint64_t* frontier, int64_t n, int64_t q) {
  const int64_t u = static_cast<int64_t>(indices[q]);
  return u >= 0 && u < n ? frontier[u] : 0;
}

// The search of word blockIdx.x.  m = its three mask arrays, `stride` words apart: LDS or a slice of the workspace.
template <typename Idx>
__device__ __forceinline__ void sd_bfs(uint64_t* m, int64_t stride, const Idx* __restrict__ indptr_, const Idx* __restrict__ indices_,
                                       const Idx* __restrict__ sources, int64_t num_sources, int64_t n, int64_t nnz,
                                       int64_t* __restrict__ dist, unsigned long long* __restrict__ state) {
  const gptr<Idx> indptr = (gptr<Idx>)indptr_, indices = (gptr<Idx>)indices_;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s0 = static_cast<int64_t>(blockIdx.x) * 64;
  const int nbits = static_cast<int>(num_sources - s0 < 64 ? num_sources - s0 : 64);
  const uint64_t valid = nbits == 64 ? ~uint64_t(0) : (uint64_t(1) << nbits) - 1;
  const int64_t chunks = (n + 63) / 64;
  int64_t f = 0, x = stride;  // the offsets of frontier and next; they swap after a level
  uint64_t* const seen = m + 2 * stride;

  // level 0: the sources' bits
  for (int64_t v = tid; v < n; v += kSdBlock) m[f + v] = 0;
  __syncthreads();
  if (tid < nbits) {
    const int64_t src = sources ? static_cast<int64_t>(sources[s0 + tid]) : s0 + tid;
    if (src >= 0 && src < n) atomicOr(reinterpret_cast<unsigned long long*>(m + f + src), 1ull << tid);
  }
  __syncthreads();
  for (int64_t c = wave; c < chunks; c += kSdBlock / 64) {
    const int64_t v = c * 64 + lane;
    const uint64_t mine = v < n ? m[f + v] : 0;
    if (v < n) seen[v] = mine;
    sd_store_bits(dist, n, s0, v, mine, 0);
  }
  __syncthreads();

  int64_t last = 0;  // the last level that found a node
  for (int64_t level = 1; level < n; ++level) {
    const uint64_t* frontier = m + f;
    int found = 0;
    for (int64_t c = wave; c < chunks; c += kSdBlock / 64) {
      const int64_t v = c * 64 + lane;
      uint64_t sv = valid, acc = 0;
      int64_t lo = 0, hi = 0;
      if (v < n) {
        sv = seen[v];
        if (sv != valid) {  // (a node every source of the word has reached skips its row)
          lo = static_cast<int64_t>(indptr[v]);
          hi = static_cast<int64_t>(indptr[v + 1]);
          lo = lo < 0 ? 0 : lo;
          hi = hi > nnz ? nnz : hi;
          hi = hi < lo ? lo : hi;
        }
      }
      const bool is_long = hi - lo > kSdLongRow;
      if (!is_long)
        for (int64_t q = lo; q < hi; ++q) acc |= sd_pull<Idx>(indices, frontier, n, q);
      uint64_t longs = __ballot(is_long);
      while (longs) {  // (the same for every lane)
        const int j = __builtin_ctzll(longs);
        longs &= longs - 1;
        const int64_t jlo = __shfl(static_cast<long long>(lo), j), jhi = __shfl(static_cast<long long>(hi), j);
        uint64_t a = 0;
        for (int64_t q = jlo + lane; q < jhi; q += 64) a |= sd_pull<Idx>(indices, frontier, n, q);
        a = wave_or(a);
        if (lane == j) acc = a;
      }
      const uint64_t nw = acc & ~sv;
      if (v < n) {
        m[x + v] = nw;
        if (nw) seen[v] = sv | nw;
      }
      sd_store_bits(dist, n, s0, v, nw, level);
      found |= nw != 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (the masks may be global memory)
    const int more = __syncthreads_or(found);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (!more) break;
    last = level;
    const int64_t t = f;
    f = x, x = t;
  }

  for (int64_t c = wave; c < chunks; c += kSdBlock / 64) {
    const int64_t v = c * 64 + lane;
    sd_store_bits(dist, n, s0, v, v < n ? valid & ~seen[v] : 0, -1);
  }
  if (tid == 0 && state) atomicMax(state, static_cast<unsigned long long>(last));
}

template <typename Idx, bool LDS>
__global__ __launch_bounds__(kSdBlock) void sd_bfs_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                          const Idx* __restrict__ sources, int64_t num_sources, int64_t n,
                                                          int64_t nnz, int64_t* __restrict__ dist, uint64_t* masks,
                                                          int64_t stride, unsigned long long* __restrict__ state) {
  if constexpr (LDS) {
    __shared__ uint64_t lds[3 * kSdLdsNodes];
    sd_bfs<Idx>(lds, kSdLdsNodes, indptr, indices, sources, num_sources, n, nnz, dist, state);
  } else {
    sd_bfs<Idx>(masks + static_cast<int64_t>(blockIdx.x) * 3 * stride, stride, indptr, indices, sources, num_sources, n, nnz,
                dist, state);
  }
}

// pred[s][v]: one lane per pair, lanes along v; block b is piece b % vblocks of source b / vblocks
template <typename Idx>
__global__ __launch_bounds__(kSdBlock) void sd_pred_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                           const Idx* __restrict__ data, int64_t n, int64_t nnz,
                                                           const int64_t* __restrict__ dist, SdPred<Idx>* __restrict__ pred,
                                                           int64_t vblocks) {
  const int64_t s = blockIdx.x / vblocks;
  const int64_t v = (blockIdx.x % vblocks) * kSdBlock + threadIdx.x;
  if (v >= n) return;
  const int64_t* dist_s = dist + s * n;
  const int64_t d = dist_s[v];
  int64_t lo = 0, hi = 0;
  if (d > 0) {
    lo = static_cast<int64_t>(indptr[v]);
    hi = static_cast<int64_t>(indptr[v + 1]);
    lo = lo < 0 ? 0 : lo;
    hi = hi > nnz ? nnz : hi;
  }
  pred[s * n + v] = sd_predecessor<Idx>((gptr<Idx>)indices, (gptr<Idx>)data, (gptr<int64_t>)dist_s, n, lo, hi, d);
}

// paths[s][v][0 .. L): a wave takes 64 consecutive v of one source
template <typename Idx>
__global__ __launch_bounds__(kSdBlock) void sd_paths_kernel(const SdPred<Idx>* __restrict__ pred, const int64_t* __restrict__ dist,
                                                            int64_t n, int64_t L, int64_t* __restrict__ paths, int64_t vblocks) {
  __shared__ int64_t tile[kSdBlock / 64][64][kSdTileRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = blockIdx.x / vblocks;
  const int64_t v0 = (blockIdx.x % vblocks) * kSdBlock + wave * 64, v = v0 + lane;
  if (v0 >= n) return;  // (whole wavefronts leave; the kernel has no barrier)
  const SdPred<Idx>* pred_s = pred + s * n;
  int64_t d = v < n ? dist[s * n + v] : 0;
  d = d < 0 ? 0 : (d > L ? L : d);
  const unsigned rows = static_cast<unsigned>(n - v0 < 64 ? n - v0 : 64);
  int64_t* out = paths + (s * n + v0) * L;
  int64_t* row = tile[wave][lane];
  int64_t cur = v;
  for (int64_t k0 = (L - 1) / kSdChunk * kSdChunk; k0 >= 0; k0 -= kSdChunk) {
    const unsigned cw = static_cast<unsigned>(L - k0 < kSdChunk ? L - k0 : kSdChunk);
    const int64_t end = d < k0 + cw ? d : k0 + cw;  // the lane's path covers [k0, end) of this chunk
    for (int64_t k = end > k0 ? end : k0; k < k0 + cw; ++k) row[k - k0] = -1;
    if (end > k0) cur = sd_walk_back<Idx>(pred_s, n, cur, k0, end, row);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (unsigned i = lane; i < rows * cw; i += 64) {  // cw == L: one contiguous stream
      const unsigned r = i / cw, k = i - r * cw;
      out[r * L + k0 + k] = tile[wave][r][k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// ---- host side --------------------------------------------------------------------------------------
struct SdLayout {  // offsets into the workspace of dgla_shortest_dist
  size_t masks, pred, state, bytes;
  int64_t stride;  // 64-bit words between the mask arrays of a search
};

SdLayout sd_layout(int idtype_bits, int64_t n, int64_t num_sources) {
  SdLayout L{};
  Carver c;
  const size_t words = static_cast<size_t>((num_sources + 63) / 64);
  const size_t one = align256(sizeof(uint64_t) * static_cast<size_t>(n));
  L.stride = static_cast<int64_t>(one / sizeof(uint64_t));
  L.masks = c.take(words * 3 * one);
  L.pred = c.take(static_cast<size_t>(idtype_bits / 8) * 2 * static_cast<size_t>(num_sources) * static_cast<size_t>(n));
  L.state = c.take(sizeof(uint64_t));
  L.bytes = c.bytes();
  return L;
}

int bad_source(const char* who, int64_t n) { return fail(who, "a source lies outside [0, " + std::to_string(n) + ")"); }

// everything dgla_shortest_dist and dgla_shortest_dist_host refuse before they read an array
int check_shortest_dist(const char* who, const dgla_csr* csr, const void* sources, int64_t num_sources, const int64_t* dist,
                        const int64_t* paths, const int64_t* max_len) {
  if (check_csr(who, csr, kCsrCols)) return -1;
  if (csr->num_rows != csr->num_cols)
    return fail(who, "invalid csr: shortest distances need a square CSR, got " + std::to_string(csr->num_rows) + " x " +
                         std::to_string(csr->num_cols));
  if (num_sources < 0) return fail(who, "negative number of sources");
  if (!sources && num_sources != csr->num_rows)
    return fail(who, "sources is null, which stands for every node, but num_sources is " + std::to_string(num_sources) +
                         " and the graph has " + std::to_string(csr->num_rows) + " nodes");
  if (sources && num_sources > 0 && csr->num_rows == 0) return bad_source(who, 0);
  if (num_sources > 0 && !dist) return fail(who, "dist is null");
  if (paths && !max_len) return fail(who, "max_len is null: paths are written at the length an earlier call reported");
  if (paths && (*max_len < 0 || *max_len > (csr->num_rows > 0 ? csr->num_rows - 1 : 0)))
    return fail(who, "max_len " + std::to_string(*max_len) + " is no path length of a graph with " +
                         std::to_string(csr->num_rows) + " nodes");
  return 0;
}

template <typename Idx>
bool sources_ok(const Idx* sources, int64_t num_sources, int64_t n) {
  for (int64_t i = 0; i < num_sources; ++i)
    if (sources[i] < 0 || static_cast<int64_t>(sources[i]) >= n) return false;
  return true;
}

// does the LDS form's static allocation fit what the device grants a workgroup?
template <typename Idx>
bool sd_lds_fits() {
  hipFuncAttributes at;
  int dev = 0, granted = 0;
  if (hipFuncGetAttributes(&at, reinterpret_cast<const void*>(sd_bfs_kernel<Idx, true>)) != hipSuccess ||
      hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&granted, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.sharedSizeBytes <= static_cast<size_t>(granted);
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename Idx>
int shortest_dist_host(const char* who, const TypedCsr<Idx>& g, const Idx* sources, int64_t num_sources, int64_t* dist,
                       int64_t* paths, int64_t* max_len) {
  const int64_t n = g.num_rows;
  for (int64_t i = 0; i < n; ++i)
    if (g.indptr[i + 1] < g.indptr[i]) return fail(who, "invalid csr: indptr decreases at row " + std::to_string(i));
  if (static_cast<int64_t>(g.indptr[0]) != 0 || static_cast<int64_t>(g.indptr[n]) != g.nnz)
    return fail(who, "invalid csr: indptr does not span [0, nnz]");
  if (sources && !sources_ok(sources, num_sources, n)) return bad_source(who, n);
  // the queue walks OUT-edges: the transpose of the in-edge CSR, entries outside [0, n) left out
  std::vector<int64_t> optr(static_cast<size_t>(n) + 1, 0), onbr;
  for (int64_t q = 0; q < g.nnz; ++q)
    if (g.indices[q] >= 0 && static_cast<int64_t>(g.indices[q]) < n) ++optr[g.indices[q] + 1];
  for (int64_t i = 0; i < n; ++i) optr[i + 1] += optr[i];
  onbr.resize(static_cast<size_t>(optr[n]));
  std::vector<int64_t> at(optr.begin(), optr.end() - 1), queue(static_cast<size_t>(n));
  for (int64_t v = 0; v < n; ++v)
    for (int64_t q = g.indptr[v]; q < g.indptr[v + 1]; ++q)
      if (g.indices[q] >= 0 && static_cast<int64_t>(g.indices[q]) < n) onbr[at[g.indices[q]]++] = v;
  int64_t longest = 0;
  for (int64_t s = 0; s < num_sources; ++s) {
    int64_t* d = dist + s * n;
    std::fill(d, d + n, int64_t(-1));
    const int64_t src = sources ? static_cast<int64_t>(sources[s]) : s;
    int64_t head = 0, tail = 0;
    d[src] = 0, queue[tail++] = src;
    while (head < tail) {
      const int64_t u = queue[head++];
      longest = std::max(longest, d[u]);
      for (int64_t q = optr[u]; q < optr[u + 1]; ++q)
        if (d[onbr[q]] < 0) d[onbr[q]] = d[u] + 1, queue[tail++] = onbr[q];
    }
  }
  if (!paths) {
    if (max_len) *max_len = longest;
    return 0;
  }
  if (*max_len != longest)
    return fail(who, "max_len is " + std::to_string(*max_len) + ", the longest shortest path has " + std::to_string(longest) +
                         " edges");
  std::vector<SdPred<Idx>> pred(static_cast<size_t>(n));
  for (int64_t s = 0; s < num_sources; ++s) {
    const int64_t* d = dist + s * n;
    for (int64_t v = 0; v < n; ++v)
      pred[v] = sd_predecessor<Idx>(g.indices, g.data, d, n, g.indptr[v], g.indptr[v + 1], d[v]);
    for (int64_t v = 0; v < n; ++v) {
      int64_t* p = paths + (s * n + v) * longest;
      const int64_t len = d[v] < 0 ? 0 : d[v];
      std::fill(p + len, p + longest, int64_t(-1));
      (void)sd_walk_back<Idx>(pred.data(), n, v, 0, len, p);
    }
  }
  return 0;
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_shortest_dist_workspace_bytes(int idtype_bits, int64_t num_nodes, int64_t num_sources) {
  if (!idbits_ok(idtype_bits) || num_nodes <= 0 || num_sources <= 0) return 0;
  return sd_layout(idtype_bits, num_nodes, num_sources).bytes;
}

int dgla_shortest_dist(const dgla_csr* csr, const void* sources, int64_t num_sources, int64_t* dist, int64_t* paths,
                       int64_t* max_len, void* workspace, size_t workspace_bytes, int64_t max_lds_nodes, void* hip_stream) {
  const char* who = "shortest_dist";
  if (check_shortest_dist(who, csr, sources, num_sources, dist, paths, max_len)) return -1;
  const int64_t n = csr->num_rows;
  if (!paths && max_len) *max_len = 0;
  if (n == 0 || num_sources == 0) return 0;
  const int64_t vblocks = (n + kSdBlock - 1) / kSdBlock;
  if (num_sources > INT32_MAX / vblocks)
    return fail(who, std::to_string(num_sources) + " sources x " + std::to_string(n) + " nodes are more pairs than one launch takes");
  const SdLayout L = sd_layout(csr->idtype_bits, n, num_sources);
  if (paths ? need_workspace(who, workspace, workspace_bytes, L.bytes) : optional_workspace(who, workspace, workspace_bytes, L.bytes))
    return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, dist);
  return with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    const Idx* src = static_cast<const Idx*>(sources);
    const dim3 block(kSdBlock), pairs(static_cast<unsigned>(num_sources * vblocks));
    if (paths) {  // the second call: the table of the first one is in the workspace
      if (*max_len == 0) return 0;
      const SdPred<Idx>* pred = reinterpret_cast<const SdPred<Idx>*>(static_cast<char*>(workspace) + L.pred);
      hipLaunchKernelGGL(sd_paths_kernel<Idx>, pairs, block, 0, s, pred, dist, n, *max_len, paths, vblocks);
      DGLA_CHECK_HIP(hipGetLastError());
      return 0;
    }
    if (src) {  // refused before any launch: the list is read back and checked here
      std::vector<Idx> host(static_cast<size_t>(num_sources));
      if (read_back(host.data(), src, sizeof(Idx) * host.size(), s)) return -1;
      if (!sources_ok(host.data(), num_sources, n)) return bad_source(who, n);
    }
    Scratch scratch(s);
    if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
    unsigned long long* state = max_len ? reinterpret_cast<unsigned long long*>(scratch.p + L.state) : nullptr;
    if (state) DGLA_CHECK_HIP(hipMemsetAsync(state, 0, sizeof(*state), s));
    const int64_t lds_nodes = max_lds_nodes > 0 && max_lds_nodes < kSdLdsNodes ? max_lds_nodes : kSdLdsNodes;
    const dim3 words(static_cast<unsigned>((num_sources + 63) / 64));
    if (n <= lds_nodes && sd_lds_fits<Idx>())
      hipLaunchKernelGGL((sd_bfs_kernel<Idx, true>), words, block, 0, s, g.indptr, g.indices, src, num_sources, n, g.nnz, dist,
                         static_cast<uint64_t*>(nullptr), int64_t(0), state);
    else
      hipLaunchKernelGGL((sd_bfs_kernel<Idx, false>), words, block, 0, s, g.indptr, g.indices, src, num_sources, n, g.nnz, dist,
                         reinterpret_cast<uint64_t*>(scratch.p + L.masks), L.stride, state);
    if (!max_len) {
      DGLA_CHECK_HIP(hipGetLastError());
      return 0;
    }
    if (workspace)  // (a table in scratch of this call's own would be lost with it)
      hipLaunchKernelGGL(sd_pred_kernel<Idx>, pairs, block, 0, s, g.indptr, g.indices, g.data, n, g.nnz, dist,
                         reinterpret_cast<SdPred<Idx>*>(scratch.p + L.pred), vblocks);
    unsigned long long longest = 0;
    if (read_back(&longest, state, sizeof(longest), s)) return -1;  // the one read-back: 8 bytes
    *max_len = static_cast<int64_t>(longest < static_cast<unsigned long long>(n) ? longest : n - 1);
    return 0;
  });
}

int dgla_shortest_dist_host(const dgla_csr* csr, const void* sources, int64_t num_sources, int64_t* dist, int64_t* paths,
                            int64_t* max_len) {
  const char* who = "shortest_dist_host";
  if (check_shortest_dist(who, csr, sources, num_sources, dist, paths, max_len)) return -1;
  if (!paths && max_len) *max_len = 0;
  if (csr->num_rows == 0 || num_sources == 0) return 0;
  return with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    return shortest_dist_host<Idx>(who, TypedCsr<Idx>(csr), static_cast<const Idx*>(sources), num_sources, dist, paths, max_len);
  });
}

}  // extern "C"
