// Top-k neighbour selection on the device: dgl.sampling.select_topk, the k in- or out-edges of every seed with the
// largest (or smallest) weight.
//
// Reference: python/dgl/sampling/neighbor.py select_topk asserts a CPU graph and sorts every row with std::sort
// (src/array/cpu/rowwise_topk.cc).  There is no GPU kernel.
//
// MI355X-first choices:
//  * The rule is the one of csrc/topk_step.h, compiled here for the kernels and for dgla_select_topk_host: an integer
//    key per edge, a strict total order (key, edge id), the first min(k, deg) entries of a row in rank order.
//  * ONE pass over a row.  A lane GROUP owns a row and streams it: coalesced loads of the edge ids, four independent
//    weight gathers per lane in flight, every entry read from HBM once (weighted_pick_kernel of csrc/sampling.hip
//    re-reads the row once per pick).
//  * Wavefront-cooperative buffered insertion.  The group holds 2 * CAP entries in LDS as three arrays (key, edge id,
//    position in the row): the KEPT half, in rank order, and a candidate BUFFER.  An entry that is before the group's
//    threshold (the kept entry of rank picks - 1) is compacted into the buffer with one __ballot and a popcount.  When
//    another round of the group might not fit, the whole group MERGES: a bitonic sort of the buffer, which leaves it in
//    reverse rank order, then one bitonic merge step against the kept half and the remaining steps over the better
//    half only.  The threshold tightens at every merge.  The last merge leaves the kept half in rank order and
//    consecutive lanes store it; the neighbour id is gathered for the picks only.  A row of deg <= picks never fills
//    the buffer before its end and is sorted once.
//  * Size classes by the largest pick count of the call (k, or the flag words of the count pass) and the CSR's mean
//    degree: 16 lanes and CAP = 32 (four rows per 64-thread workgroup), 64 lanes and CAP = 128, a 256-thread workgroup
//    and CAP = 1024.  The small classes run one wavefront per workgroup, so a barrier costs nothing and every loop can
//    be uniform over the workgroup with a per-group predicate.
//  * No atomics, no per-lane lists, no inline assembly.  The order is strict, so the result does not depend on the
//    class, the buffer's fill or the launch geometry.
#include "../../include/dgl_amd.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "sort.hip.h"
#include "topk_step.h"

namespace dgla {
namespace {

constexpr int kTopkCountBlock = 256;
constexpr int kTopkUnroll = 4;           // independent weight gathers per lane
constexpr int64_t kTopkShortMean = 32;   // mean degree up to which a row gets 16 lanes
constexpr int kTopkCapA = 32, kTopkCapB = 128, kTopkCapC = kTopkMaxPicks;

// flag words of a call (device)
enum : int { kFlBadSeed = 0, kFlOver = 1, kFlOverPicks = 2, kFlAboveA = 3, kFlAboveB = 4, kFlWords = 8 };

// picks[i] of every seed (picks[n] = 0 closes the scan) and the flag words; every writer of a flag stores the same 1
template <typename Idx>
__global__ __launch_bounds__(kTopkCountBlock) void topk_count_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ seeds,
                                                                     int64_t n, int64_t num_rows, int64_t nnz, int64_t k,
                                                                     int64_t* __restrict__ picks, int64_t* __restrict__ flags) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kTopkCountBlock) + threadIdx.x;
  if (i > n) return;
  int64_t p = 0;
  if (i < n) {
    int64_t lo, hi;
    bool bad;
    topk_row((gptr<Idx>)indptr, seeds, num_rows, nnz, i, &lo, &hi, &bad);
    p = topk_picks(hi - lo, k);
    if (bad) flags[kFlBadSeed] = 1;
    if (p > kTopkCapA) flags[kFlAboveA] = 1;
    if (p > kTopkCapB) flags[kFlAboveB] = 1;
    if (p > kTopkMaxPicks) flags[kFlOver] = 1, flags[kFlOverPicks] = p;
  }
  picks[i] = p;
}

// the bits of this lane's group in a wavefront ballot
template <int G>
__device__ __forceinline__ uint64_t topk_group_bits(uint64_t ballot, int lane) {
  if constexpr (G >= 64) {
    return ballot;
  } else {
    return (ballot >> (lane & ~(G - 1))) & ((uint64_t(1) << G) - 1);
  }
}

// One compare-exchange of the network: afterwards the entry at a is before the entry at b.
template <typename K, typename U>
__device__ __forceinline__ void topk_order(K* key, U* eid, uint32_t* pos, int a, int b) {
  const K ka = key[a], kb = key[b];
  const U ea = eid[a], eb = eid[b];
  const uint32_t pa = pos[a], pb = pos[b];
  if (topk_before(kb, eb, pb, ka, ea, pa)) {
    key[a] = kb, eid[a] = eb, pos[a] = pb;
    key[b] = ka, eid[b] = ea, pos[b] = pa;
  }
}

// The selection kernel.  NT threads per workgroup, groups of G lanes, NT / G rows per workgroup, CAP kept entries and
// CAP buffered ones per row.  Every loop and every barrier is uniform over the workgroup; `live` and `need` are the
// per-group predicates.
template <typename Idx, int DT, int NT, int G, int CAP>
__global__ __launch_bounds__(NT) void topk_select_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                         const Idx* __restrict__ data, const void* __restrict__ weight,
                                                         const Idx* __restrict__ seeds, int64_t n, int64_t num_rows, int64_t nnz,
                                                         int64_t k, int ascending, const Idx* __restrict__ out_indptr,
                                                         Idx* __restrict__ out_nbr, Idx* __restrict__ out_eids) {
  using K = typename TopkTypes<DT>::key;
  using Word = typename TopkTypes<DT>::word;
  using U = typename std::make_unsigned<Idx>::type;
  constexpr int R = NT / G, N2 = 2 * CAP, WAVES = NT / 64;
  static_assert(G <= CAP && (G >= 64 ? G == NT : true), "a round of the group must fit the buffer");
  __shared__ K s_key[R * N2];
  __shared__ U s_eid[R * N2];
  __shared__ uint32_t s_pos[R * N2];
  __shared__ int64_t s_deg[R];
  __shared__ int s_wcnt[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, lg = tid & (G - 1), grp = tid / G;
  K* key = s_key + grp * N2;
  U* eid = s_eid + grp * N2;
  uint32_t* pos = s_pos + grp * N2;
  const gptr<Word> w = (gptr<Word>)static_cast<const Word*>(weight);
  const bool asc = ascending != 0;

  const int64_t i = blockIdx.x * static_cast<int64_t>(R) + grp;
  int64_t lo = 0, hi = 0;
  int picks = 0;
  if (i < n) {
    bool bad;
    topk_row((gptr<Idx>)indptr, seeds, num_rows, nnz, i, &lo, &hi, &bad);
    const int64_t p = topk_picks(hi - lo, k);
    picks = p > CAP ? 0 : static_cast<int>(p);   // (the host refused such a row before this launch)
  }
  const bool live = picks > 0;
  if (!live) hi = lo;
  if (lg == 0) s_deg[grp] = hi - lo;
  for (int j = lg; j < CAP; j += G) key[j] = 0, eid[j] = ~U(0), pos[j] = kTopkPad;
  __syncthreads();
  int64_t maxdeg = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) maxdeg = s_deg[r] > maxdeg ? s_deg[r] : maxdeg;
  if (maxdeg == 0) return;  // (the whole workgroup leaves)

  K tk = 0;          // the threshold: the kept entry of rank picks - 1, padding until that many entries were merged
  U te = ~U(0);
  uint32_t tp = kTopkPad;
  int cnt = 0;       // entries in the buffer (the same in every lane of the group)

  // merges the buffers of the groups with `need` into their kept halves (uniform over the workgroup)
  auto merge = [&](bool need) {
    if (need)
      for (int j = cnt + lg; j < CAP; j += G) key[CAP + j] = 0, eid[CAP + j] = ~U(0), pos[CAP + j] = kTopkPad;
    __syncthreads();
    // the buffer, as the upper half of a bitonic sort of 2 * CAP entries: it ends in REVERSE rank order
    for (int kk = 2; kk <= CAP; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        if (need)
          for (int t = lg; t < CAP / 2; t += G) {
            const int a = 2 * t - (t & (j - 1)), b = a | j;
            if ((a & kk) == 0 && kk < CAP)
              topk_order(key + CAP, eid + CAP, pos + CAP, a, b);
            else
              topk_order(key + CAP, eid + CAP, pos + CAP, b, a);
          }
        __syncthreads();
      }
    }
    // kept (rank order) followed by the buffer (reverse) is bitonic: one step leaves the best CAP in the lower half
    if (need)
      for (int t = lg; t < CAP; t += G) topk_order(key, eid, pos, t, t + CAP);
    __syncthreads();
    for (int j = CAP >> 1; j > 0; j >>= 1) {
      if (need)
        for (int t = lg; t < CAP / 2; t += G) {
          const int a = 2 * t - (t & (j - 1));
          topk_order(key, eid, pos, a, a | j);
        }
      __syncthreads();
    }
    if (need) {
      tk = key[picks - 1], te = eid[picks - 1], tp = pos[picks - 1];
      cnt = 0;
    }
  };

  for (int64_t b = 0; b < maxdeg; b += G * kTopkUnroll) {
    K ck[kTopkUnroll];
    U ce[kTopkUnroll];
    bool cv[kTopkUnroll];
#pragma unroll
    for (int u = 0; u < kTopkUnroll; ++u) {
      const int64_t q = lo + b + u * G + lg;
      cv[u] = q < hi;
      ck[u] = 0, ce[u] = 0;
      if (cv[u]) {
        const int64_t e = topk_eid((gptr<Idx>)data, q);
        ce[u] = static_cast<U>(e);
        ck[u] = topk_edge_key<DT>(w, nnz, e, asc);
      }
    }
#pragma unroll
    for (int u = 0; u < kTopkUnroll; ++u) {
      if (b + u * G >= maxdeg) break;  // (the same for every lane of the workgroup)
      const bool need = cnt > CAP - G;
      if (__syncthreads_or(need ? 1 : 0)) merge(need);
      const uint32_t p = static_cast<uint32_t>(b + u * G + lg);
      const bool pass = cv[u] && topk_before(ck[u], ce[u], p, tk, te, tp);
      const uint64_t ballot = __ballot(pass);
      int off, total;
      if constexpr (G <= 64) {
        const uint64_t bits = topk_group_bits<G>(ballot, lane);
        off = __popcll(bits & ((uint64_t(1) << lg) - 1));
        total = __popcll(bits);
      } else {
        if (lane == 0) s_wcnt[tid >> 6] = __popcll(ballot);
        __syncthreads();
        off = __popcll(ballot & ((uint64_t(1) << lane) - 1));
        total = 0;
#pragma unroll
        for (int x = 0; x < WAVES; ++x) {
          if (x < (tid >> 6)) off += s_wcnt[x];
          total += s_wcnt[x];
        }
        __syncthreads();
      }
      if (pass) {
        const int at = CAP + cnt + off;   // < 2 * CAP: cnt <= CAP - G and off < G
        key[at] = ck[u], eid[at] = ce[u], pos[at] = p;
      }
      cnt += total;
    }
  }
  {
    const bool need = cnt > 0;
    if (__syncthreads_or(need ? 1 : 0)) merge(need);
  }
  if (!live) return;
  const int64_t base = static_cast<int64_t>(out_indptr[i]);
  for (int r = lg; r < picks; r += G) {
    const uint32_t p = pos[r];
    if (p == kTopkPad) continue;  // (cannot happen: a row has at least `picks` entries)
    out_eids[base + r] = static_cast<Idx>(eid[r]);
    out_nbr[base + r] = indices[lo + p];
  }
}

// ---- host side --------------------------------------------------------------------------------------
struct TopkLayout {  // offsets into the workspace of dgla_select_topk
  size_t picks, scan, flags, bytes;
};

TopkLayout topk_layout(int64_t n) {
  TopkLayout L{};
  Carver c;
  L.picks = c.take(sizeof(int64_t) * static_cast<size_t>(n + 1));
  L.scan = c.take(msd::scan_temp_bytes(n + 1, sizeof(int64_t)));
  L.flags = c.take(sizeof(int64_t) * kFlWords);
  L.bytes = c.bytes();
  return L;
}

bool topk_dtype_ok(int dt) { return dt >= kTopkF32 && dt <= kTopkI64; }

// everything dgla_select_topk and dgla_select_topk_host refuse before they read an array
int check_topk(const char* who, const dgla_csr* csr, const void* weight, int weight_dtype, const void* seeds,
               int64_t num_seeds, int64_t k, const void* out_indptr) {
  if (check_csr(who, csr)) return -1;
  if (!weight && csr->nnz > 0) return fail(who, "weight is null");
  if (!topk_dtype_ok(weight_dtype))
    return fail(who, "unsupported weight dtype " + std::to_string(weight_dtype) +
                         " (fp32, fp64, fp16, bf16, int32 and int64 are accepted)");
  if (num_seeds < 0) return fail(who, "negative number of seeds");
  if (num_seeds > 0 && !seeds) return fail(who, "seeds is null");
  if (k < -1) return fail(who, "k must be -1 (all), 0 or positive, got " + std::to_string(k));
  if (!out_indptr) return fail(who, "out_indptr is null");
  return 0;
}

int topk_over(const char* who, int64_t picks) {
  return fail(who, "a row yields " + std::to_string(picks) + " picks, which exceeds the limit of " +
                       std::to_string(kTopkMaxPicks) + " picks per row (select_topk_max_picks)");
}

int topk_bad_seed(const char* who, int64_t num_rows) {
  return fail(who, "a seed lies outside [0, " + std::to_string(num_rows) + ")");
}

// f(std::integral_constant<int, DT>{}) for the weight type of a call, checked by the caller
template <typename F>
int with_topk_dtype(int dt, F&& f) {
  switch (dt) {
    case kTopkF32: return f(std::integral_constant<int, kTopkF32>{});
    case kTopkF64: return f(std::integral_constant<int, kTopkF64>{});
    case kTopkF16: return f(std::integral_constant<int, kTopkF16>{});
    case kTopkBF16: return f(std::integral_constant<int, kTopkBF16>{});
    case kTopkI32: return f(std::integral_constant<int, kTopkI32>{});
    default: return f(std::integral_constant<int, kTopkI64>{});
  }
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename Idx, int DT>
int select_topk_host(const char* who, const TypedCsr<Idx>& g, const void* weight, const Idx* seeds, int64_t n, int64_t k,
                     bool asc, Idx* out_indptr, Idx* out_nbr, Idx* out_eids) {
  using K = typename TopkTypes<DT>::key;
  using Word = typename TopkTypes<DT>::word;
  using U = typename std::make_unsigned<Idx>::type;
  const Word* w = static_cast<const Word*>(weight);
  // refusals that need the arrays, before anything is written
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo, hi;
    bool bad;
    topk_row(g.indptr, seeds, g.num_rows, g.nnz, i, &lo, &hi, &bad);
    if (bad) return topk_bad_seed(who, g.num_rows);
    const int64_t p = topk_picks(hi - lo, k);
    if (p > kTopkMaxPicks) return topk_over(who, p);
  }
  struct Entry {
    K key;
    U eid;
    uint32_t pos;
  };
  std::vector<Entry> row;
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo, hi;
    bool bad;
    topk_row(g.indptr, seeds, g.num_rows, g.nnz, i, &lo, &hi, &bad);
    const int64_t p = topk_picks(hi - lo, k);
    out_indptr[i] = static_cast<Idx>(at);
    if (p == 0 || !out_nbr) {
      at += p;
      continue;
    }
    row.resize(static_cast<size_t>(hi - lo));
    for (int64_t q = lo; q < hi; ++q) {
      const int64_t e = topk_eid(g.data, q);
      row[q - lo] = Entry{topk_edge_key<DT>(w, g.nnz, e, asc), static_cast<U>(e), static_cast<uint32_t>(q - lo)};
    }
    std::partial_sort(row.begin(), row.begin() + p, row.end(), [](const Entry& a, const Entry& b) {
      return topk_before(a.key, a.eid, a.pos, b.key, b.eid, b.pos);
    });
    for (int64_t r = 0; r < p; ++r) {
      out_eids[at + r] = static_cast<Idx>(row[r].eid);
      out_nbr[at + r] = g.indices[lo + row[r].pos];
    }
    at += p;
  }
  out_indptr[n] = static_cast<Idx>(at);
  return 0;
}

template <typename Idx, int DT, int NT, int G, int CAP>
void launch_select(const dgla_csr* csr, const void* weight, const void* seeds, int64_t n, int64_t k, int asc, void* out_indptr,
                   void* out_nbr, void* out_eids, hipStream_t s) {
  const TypedCsr<Idx> g(csr);
  hipLaunchKernelGGL((topk_select_kernel<Idx, DT, NT, G, CAP>), dim3(grid1(n, NT / G)), dim3(NT), 0, s, g.indptr, g.indices,
                     g.data, weight, static_cast<const Idx*>(seeds), n, g.num_rows, g.nnz, k, asc,
                     static_cast<const Idx*>(out_indptr), static_cast<Idx*>(out_nbr), static_cast<Idx*>(out_eids));
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

int dgla_select_topk_max_picks(void) { return kTopkMaxPicks; }

size_t dgla_select_topk_workspace_bytes(int idtype_bits, int64_t num_seeds) {
  if (!idbits_ok(idtype_bits) || num_seeds <= 0) return 0;
  return topk_layout(num_seeds).bytes;
}

int dgla_select_topk(const dgla_csr* csr, const void* weight, int weight_dtype, const void* seeds, int64_t num_seeds,
                     int64_t k, int ascending, void* out_indptr, void* out_nbr, void* out_eids, void* workspace,
                     size_t workspace_bytes, void* hip_stream) {
  const char* who = "select_topk";
  if (check_topk(who, csr, weight, weight_dtype, seeds, num_seeds, k, out_indptr)) return -1;
  if (out_nbr && !out_eids) return fail(who, "out_eids is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_indptr);
  const int64_t n = num_seeds;
  const size_t id = static_cast<size_t>(csr->idtype_bits / 8);
  if (n == 0) {
    DGLA_CHECK_HIP(hipMemsetAsync(out_indptr, 0, id, s));
    return 0;
  }
  const TopkLayout L = topk_layout(n);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  int64_t* picks = reinterpret_cast<int64_t*>(scratch.p + L.picks);
  int64_t* flags = reinterpret_cast<int64_t*>(scratch.p + L.flags);
  DGLA_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int64_t) * kFlWords, s));
  const int rc = with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    hipLaunchKernelGGL(topk_count_kernel<Idx>, dim3(grid1(n + 1, kTopkCountBlock)), dim3(kTopkCountBlock), 0, s,
                       TypedCsr<Idx>(csr).indptr, static_cast<const Idx*>(seeds), n, csr->num_rows, csr->nnz, k, picks, flags);
    return msd::exclusive_scan<int64_t, Idx>(picks, static_cast<Idx*>(out_indptr), n + 1, scratch.p + L.scan, s);
  });
  if (rc) return -1;
  // The largest pick count decides the size class.  0 <= k <= 1024 bounds it without a read-back (and a seed outside
  // the graph is then an empty row); otherwise the flag words come back before any selection launch.
  int64_t bound = k;
  if (k < 0 || k > kTopkMaxPicks) {
    int64_t fl[kFlWords];
    if (read_back(fl, flags, sizeof(fl), s)) return -1;
    if (fl[kFlBadSeed]) return topk_bad_seed(who, csr->num_rows);
    if (fl[kFlOver]) return topk_over(who, fl[kFlOverPicks]);
    bound = fl[kFlAboveB] ? kTopkCapC : (fl[kFlAboveA] ? kTopkCapB : kTopkCapA);
  }
  if (!out_nbr || bound == 0) {
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const int64_t rows = csr->num_rows > 0 ? csr->num_rows : 1;
  const bool short_rows = csr->nnz / rows <= kTopkShortMean;
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    return with_topk_dtype(weight_dtype, [&](auto dt) -> int {
      constexpr int DT = decltype(dt)::value;
      if (bound <= kTopkCapA && short_rows)
        launch_select<Idx, DT, 64, 16, kTopkCapA>(csr, weight, seeds, n, k, ascending, out_indptr, out_nbr, out_eids, s);
      else if (bound <= kTopkCapB)
        launch_select<Idx, DT, 64, 64, kTopkCapB>(csr, weight, seeds, n, k, ascending, out_indptr, out_nbr, out_eids, s);
      else
        launch_select<Idx, DT, 256, 256, kTopkCapC>(csr, weight, seeds, n, k, ascending, out_indptr, out_nbr, out_eids, s);
      return 0;
    });
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_select_topk_host(const dgla_csr* csr, const void* weight, int weight_dtype, const void* seeds, int64_t num_seeds,
                          int64_t k, int ascending, void* out_indptr, void* out_nbr, void* out_eids) {
  const char* who = "select_topk_host";
  if (check_topk(who, csr, weight, weight_dtype, seeds, num_seeds, k, out_indptr)) return -1;
  if (out_nbr && !out_eids) return fail(who, "out_eids is null");
  return with_idx(csr->idtype_bits, [&](auto tag) -> int {
    using Idx = decltype(tag);
    return with_topk_dtype(weight_dtype, [&](auto dt) -> int {
      constexpr int DT = decltype(dt)::value;
      return select_topk_host<Idx, DT>(who, TypedCsr<Idx>(csr), weight, static_cast<const Idx*>(seeds), num_seeds, k, ascending != 0,
                                       static_cast<Idx*>(out_indptr), static_cast<Idx*>(out_nbr), static_cast<Idx*>(out_eids));
    });
  });
}

}  // extern "C"
