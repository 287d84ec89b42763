// Negative sampling on the device: global uniform (u, v) pairs that are not edges, and the edge lookup behind it
// (dgl.sampling.global_uniform_negative_sampling, DGLGraph.has_edges_between).
//
// Reference: CSRGlobalUniformNegativeSampling<kDGLCUDA> (src/array/cuda/negative_sampling.cu): a Philox kernel draws
// num_trials pairs per slot and tests them by a linear / binary search of the row; cub DeviceSelect::If drops the empty
// slots; without replacement two cub radix sorts order the pairs by (row, col), DeviceSelect::Unique drops duplicates
// and the FIRST num_samples of the sorted pairs are returned — the lexicographically smallest, a sample biased toward
// small source ids.
//
// MI355X-first choices:
//  * The rule is the one of csrc/negative_sample_step.h, compiled here for the kernels and for
//    dgla_negative_sample_host: counter-based draws keyed by (seed, slot, trial), the edge test a bisection of the
//    relation's membership list (dgla_csr_sorted_columns, the list the node2vec step reads).  The result is a pure
//    function of its arguments, whatever the launch geometry.
//  * Work and memory per call are O(n_slots): nothing is sized by the node or edge count of the graph.
//  * Draw: one lane per slot writes the pair and an accept flag; the workgroup's accept count comes from the library's
//    block scan (csrc/sort.hip.h).  Compaction: a device scan of the per-block counts, then every workgroup re-derives its
//    in-block offsets with the same block scan — slot order is kept, so with replacement the result is the first
//    accepted slots.
//  * Duplicates (without replacement) are found WITHOUT sorting by node ids: ONE stable dgla_coo_to_csr over the slots
//    (int32), the row a hash bucket mix(u, v) mod B with B = the power of two >= n_slots (at most 2^30), the column the
//    accept flag (one bit) and the carried position the slot.  One lane per sorted position walks back inside its bucket
//    run to the first earlier accepted slot with the same pair and clears its own keep flag when there is one; the sort
//    is stable, so "earlier in the run" is "earlier slot".  The same count / scan / compact then runs over the keep
//    flags, in slot order.  The hash decides cost only, never the result.
//  * The accepted count never leaves the device.  The sort runs over all n_slots slots (a host-known number) and not
//    over the accepted ones: an empty slot goes to bucket mix(i) mod B, is carried with flag 0 and is stepped over by
//    the walk, so no kernel needs a launch size read from device memory and no bucket collects the empties.
//  * exclude_self_loops and replace are template parameters of the draw kernel, not flags tested in the trial loop.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>
#include <unordered_set>
#include <utility>

#include "host_util.h"
#include "negative_sample_step.h"
#include "sort.hip.h"

namespace dgla {
namespace {

constexpr int kNegBlock = 256;         // every launch here: grid1(n) blocks of kNegBlock threads
constexpr int kNegMaxBucketBits = 30;  // B + 1 int32 row starts must stay addressable with int32 ids
static_assert(kNegBlock == 256, "grid1 counts blocks of 256");

int bucket_bits(int64_t n) {
  const int b = msd::bits_for(n);
  return b > kNegMaxBucketBits ? kNegMaxBucketBits : b;
}

// ---- draw -------------------------------------------------------------------------------------
// Slot i: pu[i], pv[i] = the pair or -1, flag[i] = accepted.  REPLACE: cnt[block] = accepted slots of the workgroup
// (cnt[gridDim.x] = 0 closes the scan).  !REPLACE: row[i] = the slot's bucket in the duplicate search.
template <typename Idx, bool EXCL, bool REPLACE>
__global__ __launch_bounds__(kNegBlock) void neg_draw_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ member,
                                                             int64_t R, int64_t C, int T, uint64_t seed, int64_t n,
                                                             Idx* __restrict__ pu, Idx* __restrict__ pv,
                                                             int32_t* __restrict__ flag, int32_t* __restrict__ cnt,
                                                             int32_t* __restrict__ row, uint32_t bucket_mask) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kNegBlock) + threadIdx.x;
  int64_t u = -1, v = -1;
  bool ok = false;
  if (i < n) {
    ok = neg_draw<EXCL>((gptr<Idx>)indptr, (gptr<Idx>)member, R, C, T, seed, i, &u, &v);
    pu[i] = ok ? static_cast<Idx>(u) : Idx(-1);
    pv[i] = ok ? static_cast<Idx>(v) : Idx(-1);
    flag[i] = ok ? 1 : 0;
    if (!REPLACE)
      row[i] = static_cast<int32_t>((ok ? neg_pair_hash(u, v) : rw_mix64(static_cast<uint64_t>(i))) & bucket_mask);
  }
  if (REPLACE) {
    __shared__ int wsum[kNegBlock / 64];
    int total;
    (void)msd::block_exclusive_scan<kNegBlock>(ok ? 1 : 0, &total, wsum);
    if (threadIdx.x == 0) {
      cnt[blockIdx.x] = total;
      if (blockIdx.x == 0) cnt[gridDim.x] = 0;
    }
  }
}

// cnt[block] = flags set among the workgroup's slots (after the duplicate search)
__global__ __launch_bounds__(kNegBlock) void neg_count_kernel(const int32_t* __restrict__ flag, int64_t n,
                                                              int32_t* __restrict__ cnt) {
  __shared__ int wsum[kNegBlock / 64];
  const int64_t i = blockIdx.x * static_cast<int64_t>(kNegBlock) + threadIdx.x;
  int total;
  (void)msd::block_exclusive_scan<kNegBlock>(i < n ? flag[i] : 0, &total, wsum);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = total;
    if (blockIdx.x == 0) cnt[gridDim.x] = 0;
  }
}

// ---- duplicates ---------------------------------------------------------------------------------
// One lane per sorted position p: the slot there loses its keep flag when an earlier position of its bucket run holds
// an accepted slot with the same pair.  s_flag / s_slot: the accept flags and the slots in sorted order; bstart: the
// bucket starts.  A lane writes the flag of its own slot only and reads nothing another lane writes.
// Order inside a run: the sort orders by ROW only and is stable (the column travels with the element, it is no key:
// coo2csr.hip, "edges keep their COO order inside a row"; dgla_csr_sorted_columns needs a second sort for the same
// reason).  So a run lists its slots in ascending slot order, empty ones (flag 0) BETWEEN accepted ones, and the walk
// has to step over them: stopping at the first flag-0 entry would miss earlier slots with the same pair.  The walk is
// short all the same: B >= n_slots buckets hold about one DISTINCT pair and one empty slot each, so a repeat meets its
// pair a step or two back and a first occurrence sits near the start of its run.
template <typename Idx>
__global__ __launch_bounds__(kNegBlock) void neg_dedup_kernel(const int32_t* __restrict__ bstart, const int32_t* __restrict__ row,
                                                              const int32_t* __restrict__ s_flag,
                                                              const int32_t* __restrict__ s_slot, const Idx* __restrict__ pu,
                                                              const Idx* __restrict__ pv, int64_t n, int32_t* __restrict__ flag) {
  const int64_t p = blockIdx.x * static_cast<int64_t>(kNegBlock) + threadIdx.x;
  if (p >= n || !s_flag[p]) return;
  const int32_t slot = s_slot[p];
  const int64_t start = bstart[row[slot]];
  const Idx u = pu[slot], v = pv[slot];
  for (int64_t q = p - 1; q >= start; --q) {
    if (!s_flag[q]) continue;
    const int32_t other = s_slot[q];
    if (pu[other] == u && pv[other] == v) {
      flag[slot] = 0;
      break;
    }
  }
}

// ---- compaction, padding and the count ------------------------------------------------------------
// base = the exclusive scan of cnt over nb + 1 entries, so base[nb] is the number of flagged slots.  Flagged slot i
// goes to position base[block] + (flagged slots before it in the workgroup) when that is < num_samples; the entries
// from min(base[nb], num_samples) on are -1.  The two sets of positions are disjoint, so no write is ordered.
template <typename Idx>
__global__ __launch_bounds__(kNegBlock) void neg_compact_kernel(const Idx* __restrict__ pu, const Idx* __restrict__ pv,
                                                                const int32_t* __restrict__ flag,
                                                                const int32_t* __restrict__ base, int64_t n, int64_t nb,
                                                                int64_t num_samples, Idx* __restrict__ out_src,
                                                                Idx* __restrict__ out_dst, int64_t* __restrict__ out_count) {
  __shared__ int wsum[kNegBlock / 64];
  const int64_t i = blockIdx.x * static_cast<int64_t>(kNegBlock) + threadIdx.x;
  const int f = i < n ? flag[i] : 0;
  int total;
  const int off = msd::block_exclusive_scan<kNegBlock>(f, &total, wsum);
  const int64_t all = base[nb];
  if (f) {
    const int64_t pos = static_cast<int64_t>(base[blockIdx.x]) + off;   // (f set: i < n, so blockIdx.x < nb)
    if (pos < num_samples) out_src[pos] = pu[i], out_dst[pos] = pv[i];
  }
  if (i < num_samples && i >= all) out_src[i] = Idx(-1), out_dst[i] = Idx(-1);
  if (i == 0) *out_count = all < num_samples ? all : num_samples;
}

// nothing can be drawn (no slots, no rows or no columns): -1 everywhere, count 0
template <typename Idx>
__global__ __launch_bounds__(kNegBlock) void neg_fill_kernel(int64_t num_samples, Idx* __restrict__ out_src,
                                                             Idx* __restrict__ out_dst, int64_t* __restrict__ out_count) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kNegBlock) + threadIdx.x;
  if (i < num_samples) out_src[i] = Idx(-1), out_dst[i] = Idx(-1);
  if (i == 0) *out_count = 0;
}

// ---- the edge lookup --------------------------------------------------------------------------------
template <typename Idx>
__global__ __launch_bounds__(kNegBlock) void has_edges_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ member,
                                                              int64_t R, int64_t C, const Idx* __restrict__ u,
                                                              const Idx* __restrict__ v, int64_t n, uint8_t* __restrict__ out) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kNegBlock) + threadIdx.x;
  if (i >= n) return;
  out[i] = neg_has_edge((gptr<Idx>)indptr, (gptr<Idx>)member, R, C, static_cast<int64_t>(u[i]), static_cast<int64_t>(v[i])) ? 1 : 0;
}

// ---- host side --------------------------------------------------------------------------------------
struct NegLayout {  // offsets into the workspace of dgla_negative_sample
  size_t pu, pv, flag, cnt, base, scan, row, s_flag, s_slot, bstart, sort, sort_bytes, bytes;
  int64_t nb;
  int kb;
};

NegLayout neg_layout(int idtype_bits, int64_t n) {
  NegLayout L{};
  const size_t ids = (idtype_bits == 32 ? 4 : 8) * static_cast<size_t>(n), words = sizeof(int32_t) * static_cast<size_t>(n);
  L.nb = (n + kNegBlock - 1) / kNegBlock;
  L.kb = bucket_bits(n);
  const int64_t B = int64_t(1) << L.kb;
  Carver c;
  L.pu = c.take(ids);
  L.pv = c.take(ids);
  L.flag = c.take(words);
  L.cnt = c.take(sizeof(int32_t) * static_cast<size_t>(L.nb + 1));
  L.base = c.take(sizeof(int32_t) * static_cast<size_t>(L.nb + 1));
  L.scan = c.take(msd::scan_temp_bytes(L.nb + 1, sizeof(int32_t)));
  // the duplicate search (sized whatever `replace` is: the size query does not know it)
  L.row = c.take(words);
  L.s_flag = c.take(words);
  L.s_slot = c.take(words);
  L.bstart = c.take(sizeof(int32_t) * static_cast<size_t>(B + 1));
  L.sort_bytes = align256(dgla_coo_to_csr_workspace_bytes(32, B, n));
  L.sort = c.take(L.sort_bytes);
  L.bytes = c.bytes();
  return L;
}

// the column ids are read from `member` (the csr with sorted columns), never from csr->indices
constexpr unsigned kNegCsr = kCsrCols | kCsrEmptyIndptr | kCsrAnyIndices;

int check_has_edges(const char* who, const dgla_csr* csr, const void* member, const void* u, const void* v, int64_t n,
                    const void* out) {
  if (check_csr(who, csr, kNegCsr)) return -1;
  if (n < 0) return fail(who, "negative size");
  if (csr->nnz > 0 && !member) return fail(who, "member is null");
  if (n > 0 && (!u || !v || !out)) return fail(who, "u / v / out are null");
  return 0;
}

// everything both sampling entry points refuse
int check_neg(const char* who, const dgla_csr* csr, const void* member, int64_t n_slots, int64_t num_samples, int num_trials,
              const void* out_src, const void* out_dst, const void* out_count) {
  if (check_csr(who, csr, kNegCsr)) return -1;
  if (n_slots < 0 || num_samples < 0) return fail(who, "negative number of slots / samples");
  if (n_slots >= (int64_t(1) << 31) || num_samples >= (int64_t(1) << 31))
    return fail(who, "n_slots and num_samples must be below 2^31, got " + std::to_string(n_slots) + " and " +
                         std::to_string(num_samples));
  if (num_trials < 1 || num_trials > kNegMaxTrials)
    return fail(who, "num_trials must be in 1 .. " + std::to_string(kNegMaxTrials) + ", got " + std::to_string(num_trials));
  if (csr->nnz > 0 && !member) return fail(who, "member is null");
  if (num_samples > 0 && (!out_src || !out_dst)) return fail(who, "out_src / out_dst are null");
  if (!out_count) return fail(who, "out_count is null");
  return 0;
}

template <typename Idx>
int run_neg(const TypedCsr<Idx>& c, const void* member, int64_t n, int64_t num_samples, int T, bool excl, bool replace,
            uint64_t seed, void* out_src, void* out_dst, int64_t* out_count, char* ws, const NegLayout& L, hipStream_t s) {
  Idx *pu = reinterpret_cast<Idx*>(ws + L.pu), *pv = reinterpret_cast<Idx*>(ws + L.pv);
  int32_t *flag = reinterpret_cast<int32_t*>(ws + L.flag), *cnt = reinterpret_cast<int32_t*>(ws + L.cnt),
          *base = reinterpret_cast<int32_t*>(ws + L.base), *row = reinterpret_cast<int32_t*>(ws + L.row),
          *s_flag = reinterpret_cast<int32_t*>(ws + L.s_flag), *s_slot = reinterpret_cast<int32_t*>(ws + L.s_slot),
          *bstart = reinterpret_cast<int32_t*>(ws + L.bstart);
  const uint32_t mask = (1u << L.kb) - 1u;
#define DGLA_NEG_DRAW(E, P)                                                                                             \
  hipLaunchKernelGGL((neg_draw_kernel<Idx, E, P>), dim3(grid1(n)), dim3(kNegBlock), 0, s,                               \
                     c.indptr, static_cast<const Idx*>(member), c.num_rows, c.num_cols, T, seed, n, pu, pv, flag, cnt, \
                     row, mask)
  if (excl) {
    if (replace) DGLA_NEG_DRAW(true, true); else DGLA_NEG_DRAW(true, false);
  } else {
    if (replace) DGLA_NEG_DRAW(false, true); else DGLA_NEG_DRAW(false, false);
  }
#undef DGLA_NEG_DRAW
  DGLA_CHECK_HIP(hipGetLastError());
  if (!replace) {
    // stable by bucket: column = the accept flag (one bit), carried position = the slot
    if (dgla_coo_to_csr_bounded(32, int64_t(1) << L.kb, 2, n, row, flag, nullptr, bstart, s_flag, s_slot, ws + L.sort,
                                L.sort_bytes, s))
      return -1;
    hipLaunchKernelGGL(neg_dedup_kernel<Idx>, dim3(grid1(n)), dim3(kNegBlock), 0, s, bstart, row, s_flag, s_slot, pu, pv, n,
                       flag);
    hipLaunchKernelGGL(neg_count_kernel, dim3(grid1(n)), dim3(kNegBlock), 0, s, flag, n, cnt);
    DGLA_CHECK_HIP(hipGetLastError());
  }
  if (msd::exclusive_scan<int32_t, int32_t>(cnt, base, L.nb + 1, ws + L.scan, s)) return -1;
  hipLaunchKernelGGL(neg_compact_kernel<Idx>, dim3(grid1(n > num_samples ? n : num_samples)), dim3(kNegBlock), 0, s, pu, pv,
                     flag, base, n, L.nb, num_samples, static_cast<Idx*>(out_src), static_cast<Idx*>(out_dst), out_count);
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

struct PairHash {
  size_t operator()(const std::pair<int64_t, int64_t>& p) const { return static_cast<size_t>(neg_pair_hash(p.first, p.second)); }
};

// the whole rule, slot by slot
template <typename Idx, bool EXCL>
void neg_host(const TypedCsr<Idx>& c, const void* member, int64_t n, int64_t num_samples, int T, bool replace, uint64_t seed,
              void* out_src, void* out_dst, int64_t* out_count) {
  const Idx* mem = static_cast<const Idx*>(member);
  Idx *os = static_cast<Idx*>(out_src), *od = static_cast<Idx*>(out_dst);
  std::unordered_set<std::pair<int64_t, int64_t>, PairHash> seen;
  int64_t count = 0;
  for (int64_t i = 0; i < n && count < num_samples; ++i) {
    int64_t u, v;
    if (!neg_draw<EXCL>(c.indptr, mem, c.num_rows, c.num_cols, T, seed, i, &u, &v)) continue;
    if (!replace && !seen.insert({u, v}).second) continue;
    os[count] = static_cast<Idx>(u), od[count] = static_cast<Idx>(v);
    ++count;
  }
  for (int64_t k = count; k < num_samples; ++k) os[k] = Idx(-1), od[k] = Idx(-1);
  *out_count = count;
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_negative_sample_workspace_bytes(int idtype_bits, int64_t n_slots) {
  if (!idbits_ok(idtype_bits) || n_slots <= 0 || n_slots >= (int64_t(1) << 31)) return 0;
  return neg_layout(idtype_bits, n_slots).bytes;
}

int dgla_negative_sample(const dgla_csr* csr, const void* member, int64_t n_slots, int64_t num_samples, int num_trials,
                         int exclude_self_loops, int replace, uint64_t seed, void* out_src, void* out_dst,
                         int64_t* out_count, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "negative_sample";
  if (check_neg(who, csr, member, n_slots, num_samples, num_trials, out_src, out_dst, out_count)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const bool drawable = n_slots > 0 && csr->num_rows > 0 && csr->num_cols > 0;
  NegLayout L{};
  if (drawable) {
    L = neg_layout(csr->idtype_bits, n_slots);
    if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  }
  const DeviceGuard dev(s, out_count);
  if (!drawable) {
    with_idx(csr->idtype_bits, [&](auto tag) {
      using Idx = decltype(tag);
      hipLaunchKernelGGL(neg_fill_kernel<Idx>, dim3(grid1(num_samples)), dim3(kNegBlock), 0, s, num_samples,
                         static_cast<Idx*>(out_src), static_cast<Idx*>(out_dst), out_count);
    });
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  }
  char* ws = static_cast<char*>(workspace);
  return with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    return run_neg<Idx>(TypedCsr<Idx>(csr), member, n_slots, num_samples, num_trials, exclude_self_loops != 0, replace != 0,
                        seed, out_src, out_dst, out_count, ws, L, s);
  });
}

int dgla_negative_sample_host(const dgla_csr* csr, const void* member, int64_t n_slots, int64_t num_samples, int num_trials,
                              int exclude_self_loops, int replace, uint64_t seed, void* out_src, void* out_dst,
                              int64_t* out_count) {
  if (check_neg("negative_sample_host", csr, member, n_slots, num_samples, num_trials, out_src, out_dst, out_count)) return -1;
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    auto run = [&](auto excl) {
      neg_host<Idx, decltype(excl)::value>(TypedCsr<Idx>(csr), member, n_slots, num_samples, num_trials, replace != 0, seed, out_src,
                                           out_dst, out_count);
    };
    if (exclude_self_loops) run(std::true_type{}); else run(std::false_type{});
  });
  return 0;
}

int dgla_csr_has_edges(const dgla_csr* csr, const void* member, const void* u, const void* v, int64_t n, uint8_t* out,
                       void* hip_stream) {
  if (check_has_edges("csr_has_edges", csr, member, u, v, n, out)) return -1;
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    hipLaunchKernelGGL(has_edges_kernel<Idx>, dim3(grid1(n)), dim3(kNegBlock), 0, s, TypedCsr<Idx>(csr).indptr,
                       static_cast<const Idx*>(member), csr->num_rows, csr->num_cols, static_cast<const Idx*>(u),
                       static_cast<const Idx*>(v), n, out);
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_csr_has_edges_host(const dgla_csr* csr, const void* member, const void* u, const void* v, int64_t n, uint8_t* out) {
  if (check_has_edges("csr_has_edges_host", csr, member, u, v, n, out)) return -1;
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    const Idx *mem = static_cast<const Idx*>(member), *us = static_cast<const Idx*>(u), *vs = static_cast<const Idx*>(v);
    for (int64_t i = 0; i < n; ++i)
      out[i] = neg_has_edge(g.indptr, mem, csr->num_rows, csr->num_cols, static_cast<int64_t>(us[i]), static_cast<int64_t>(vs[i]));
  });
  return 0;
}

}  // extern "C"
