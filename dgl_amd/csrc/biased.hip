// Tag sort and tag-biased neighbour sampling on the device: dgl.sort_csr_by_tag / sort_csc_by_tag and
// dgl.sampling.sample_neighbors_biased.
//
// Reference: CSRSortByTag (src/array/cpu/csr_sort.cc) and CSRRowWiseSamplingBiased (src/array/cpu/rowwise_sampling.cc)
// exist for the CPU only; python/dgl/sampling/neighbor.py documents "Must be on CPU".
//
// MI355X-first choices:
//  * The rules are those of csrc/biased_step.h, compiled here for the kernels and for the two host twins.
//  * Sort: a UNIT owns a row, 16 lanes (mean degree <= 32), a wavefront, or a 256-lane workgroup for rows of 2048
//    entries and more (the lane-group pass reports such rows in a flag word that the call reads back anyway, and the
//    workgroup pass runs only then).  Two sweeps over the row in chunks of the unit's width: a histogram, and a stable
//    scatter.  Tags are peeled off a chunk with a first-active-lane broadcast; one ballot and one popcount per distinct
//    tag give the count (sweep 1) and every lane's rank among the equal tags below it (sweep 2).  ONE lane per distinct
//    tag touches a counter: no atomics.  The 256-lane unit lets its four wavefronts at the counters in turn.
//  * Counters: T + 1 <= 256 per unit live in LDS; beyond that they live in the row's own tag_pos slice, which the unit
//    alone owns.  The cursor of tag t is slot t + 1: it starts at the tag's offset and ends at the next tag's, so what
//    the scatter leaves behind IS the reference's tag_pos.  No scratch and no workspace proportional to N * T.
//  * Picks: a count kernel (one thread per seed, T offsets), the device scan, and a pick kernel in which a lane group
//    owns a seed (16 lanes when T <= 16, else a wavefront) and NEVER walks the row: it keeps start, length, bias and the
//    taken count of every tag in LDS, one tag per lane and chunk, draws a tag with the Hillis-Steele lane scan of the
//    rule and a ballot, and gathers `indices` / `data` for the picks only.  Without replacement the earlier picks of the
//    row are staged in the seed's own output slice and Floyd's step tests them a group width at a time: no rejection
//    loop.  Cost per seed O(T / W * picks + picks^2 / W), independent of the degree.
//  * fanout >= 0 reads nothing back and allocates nothing when a workspace is given: the call can be captured.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "sort.hip.h"
#include "biased_step.h"

namespace dgla {
namespace {

constexpr int kSortLdsTags = 255;        // T + 1 <= 256 counters per unit live in LDS
constexpr int64_t kSortShortMean = 32;   // mean degree up to which a row gets 16 lanes
constexpr int64_t kSortHubDeg = 2048;    // rows at least this long go to the workgroup pass
constexpr int kBiasedCountBlock = 256;
constexpr int kBiasedCapSmall = 64;      // tags per group of the small pick kernels

// flag words of a call (device); every writer of a word stores the same 1
enum : int { kFwBadTag = 0, kFwBadEid = 1, kFwHub = 2, kFwBadSeed = 3, kFwWords = 4 };

__global__ void biased_clear_kernel(int* words, int n) {
  if (static_cast<int>(threadIdx.x) < n) words[threadIdx.x] = 0;
}

// the bits of this lane's group in a wavefront ballot
template <int G>
__device__ __forceinline__ uint64_t group_bits(uint64_t ballot, int lane) {
  if constexpr (G >= 64) {
    return ballot;
  } else {
    return (ballot >> (lane & ~(G - 1))) & ((uint64_t(1) << G) - 1);
  }
}

// what one lane of a unit wrote is seen by the others: a wavefront needs no instruction but an ordering, a workgroup a
// barrier
template <int G>
__device__ __forceinline__ void unit_sync() {
  if constexpr (G > 64) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

// Peels the distinct tags off one chunk of a group of G <= 64 lanes.  f(tag, same, leader_lane, mine) runs once per
// distinct tag in all lanes of the group: `same` = the group's lanes that hold the tag, `mine` = this lane is one.
template <int G, typename F>
__device__ __forceinline__ void peel(bool active, int64_t t, int lane, F&& f) {
  const int gbase = G >= 64 ? 0 : (lane & ~(G - 1));
  while (true) {
    const uint64_t bits = group_bits<G>(__ballot(active), lane);
    if (!bits) break;
    const int leader = gbase + __ffsll(static_cast<unsigned long long>(bits)) - 1;
    const int64_t lt = __shfl(t, leader, 64);
    const bool mine = active && t == lt;
    const uint64_t same = group_bits<G>(__ballot(mine), lane);
    f(lt, same, leader, mine);
    active = active && !mine;
  }
}

// The sort kernel.  NT threads per workgroup, units of G lanes, NT / G rows per workgroup.
template <typename Idx, typename Tag, int NT, int G, bool LDSC>
__global__ __launch_bounds__(NT) void tag_sort_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                      const Idx* __restrict__ data, const Tag* __restrict__ tag,
                                                      int64_t num_rows, int64_t nnz, int64_t T, Idx* __restrict__ out_indices,
                                                      Idx* __restrict__ out_data, Idx* tag_pos, int* __restrict__ flags) {
  constexpr int R = NT / G, S = G < 64 ? G : 64, PG = G < 64 ? G : 64, WAVES = NT / 64;
  __shared__ Idx s_cnt[LDSC ? R * (kSortLdsTags + 1) : 1];
  const int tid = threadIdx.x, lane = tid & 63, lg = tid & (G - 1), grp = tid / G, wave = tid >> 6;
  const int64_t row = blockIdx.x * static_cast<int64_t>(R) + grp;
  if (row >= num_rows) return;
  int64_t lo = static_cast<int64_t>(indptr[row]), hi = static_cast<int64_t>(indptr[row + 1]);
  lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
  hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
  const int64_t deg = hi - lo;
  const bool hub = deg >= kSortHubDeg;
  if constexpr (G < 256) {
    if (hub) {  // (left to the workgroup pass)
      if (lg == 0) flags[kFwHub] = 1;
      return;
    }
  } else {
    if (!hub) return;  // (the whole workgroup leaves)
  }
  Idx* c;
  if constexpr (LDSC) {
    c = s_cnt + grp * (kSortLdsTags + 1);
  } else {
    c = tag_pos + row * (T + 1);
  }
  for (int64_t j = lg; j <= T; j += G) c[j] = 0;
  unit_sync<G>();

  int fl = 0;
  // one chunk's entry of this lane
  auto load = [&](int64_t b, int64_t* e, int64_t* t) -> bool {
    const int64_t q = lo + b + lg;
    if (q >= hi) return false;
    *e = topk_eid((gptr<Idx>)data, q);
    *t = biased_tag((gptr<Tag>)tag, nnz, T, *e, &fl);
    return *t >= 0;
  };
  // runs body(w) for the wavefronts of the unit in turn, so that a counter has one writer at a time
  auto in_turn = [&](auto&& body) {
    if constexpr (G > 64) {
      for (int w = 0; w < WAVES; ++w) {
        if (wave == w) body();
        __syncthreads();
      }
    } else {
      body();
    }
  };

  // sweep 1: the histogram, the count of tag t in slot t + 1
  for (int64_t b = 0; b < deg; b += G) {
    int64_t e = 0, t = -1;
    const bool valid = load(b, &e, &t);
    in_turn([&] {
      peel<PG>(valid, t, lane, [&](int64_t lt, uint64_t same, int leader, bool mine) {
        if (lane == leader) c[lt + 1] += static_cast<Idx>(__popcll(same));
      });
    });
  }
  unit_sync<G>();
  // slot t + 1 becomes the offset of tag t (an exclusive prefix over slots 1 .. T), slot 0 stays 0
  if (G <= 64 || wave == 0) {
    const int ls = tid & (S - 1);
    Idx carry = 0;
    for (int64_t j0 = 1; j0 <= T; j0 += S) {
      const int64_t j = j0 + ls;
      const Idx own = j <= T ? c[j] : Idx(0);
      Idx inc = own;
#pragma unroll
      for (int d = 1; d < S; d <<= 1) {
        const Idx y = __shfl_up(inc, d, S);
        if (ls >= d) inc += y;
      }
      if (j <= T) c[j] = carry + inc - own;
      carry += __shfl(inc, S - 1, S);
    }
  }
  unit_sync<G>();
  // sweep 2: the stable scatter; the cursor of tag t is slot t + 1
  for (int64_t b = 0; b < deg; b += G) {
    int64_t e = 0, t = -1;
    const bool valid = load(b, &e, &t);
    const Idx nbr = valid ? indices[lo + b + lg] : Idx(0);
    int64_t rank = 0;
    in_turn([&] {
      peel<PG>(valid, t, lane, [&](int64_t lt, uint64_t same, int leader, bool mine) {
        Idx cur = 0;
        if (lane == leader) cur = c[lt + 1];
        cur = __shfl(cur, leader, 64);
        const int below = __popcll(same & ((uint64_t(1) << (lane & (PG - 1))) - 1));
        if (mine) rank = static_cast<int64_t>(cur) + below;
        if (lane == leader) c[lt + 1] = cur + static_cast<Idx>(__popcll(same));
      });
    });
    if (valid && rank < deg) {
      out_indices[lo + rank] = nbr;
      out_data[lo + rank] = static_cast<Idx>(e);
    }
  }
  if (fl & kBiasedBadTag) flags[kFwBadTag] = 1;
  if (fl & kBiasedBadEid) flags[kFwBadEid] = 1;
  if constexpr (LDSC) {
    unit_sync<G>();
    Idx* dst = tag_pos + row * (T + 1);
    for (int64_t j = lg; j <= T; j += G) dst[j] = c[j];
  }
}

// picks[i] of every seed (picks[n] = 0 closes the scan)
template <typename Idx, typename B>
__global__ __launch_bounds__(kBiasedCountBlock) void biased_count_kernel(const Idx* __restrict__ indptr,
                                                                         const Idx* __restrict__ tag_offset,
                                                                         const B* __restrict__ bias, const Idx* __restrict__ seeds,
                                                                         int64_t n, int64_t num_rows, int64_t nnz, int64_t T,
                                                                         int64_t fanout, int replace, int64_t* __restrict__ picks,
                                                                         int* __restrict__ flags) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kBiasedCountBlock) + threadIdx.x;
  if (i > n) return;
  int64_t p = 0;
  if (i < n) {
    int64_t lo, hi;
    bool bad;
    topk_row((gptr<Idx>)indptr, seeds, num_rows, nnz, i, &lo, &hi, &bad);
    if (bad) {
      flags[kFwBadSeed] = 1;
    } else {
      const int64_t u = static_cast<int64_t>(seeds[i]);
      p = biased_picks(biased_positive((gptr<Idx>)(tag_offset + u * (T + 1)), (gptr<B>)bias, T, hi - lo), fanout, replace != 0);
    }
  }
  picks[i] = p;
}

// The pick kernel.  64 threads per workgroup, groups of W lanes, 64 / W seeds per workgroup, at most TCAP tags.
template <typename Idx, typename B, int W, int TCAP>
__global__ __launch_bounds__(64) void biased_pick_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                         const Idx* __restrict__ data, const Idx* __restrict__ tag_offset,
                                                         const B* __restrict__ bias, const Idx* __restrict__ seeds, int64_t n,
                                                         int64_t num_rows, int64_t nnz, int64_t T, int64_t fanout, int replace,
                                                         uint64_t rng_seed, const Idx* __restrict__ out_indptr, Idx* out_nbr,
                                                         Idx* out_eids) {
  constexpr int R = 64 / W;
  __shared__ int64_t s_start[R * TCAP];
  __shared__ int64_t s_n[R * TCAP];
  __shared__ int64_t s_taken[R * TCAP];
  __shared__ double s_b[R * TCAP];
  const int lane = threadIdx.x & 63, lg = lane & (W - 1), grp = lane / W;
  const int64_t i = blockIdx.x * static_cast<int64_t>(R) + grp;
  if (i >= n) return;
  int64_t lo, hi;
  bool bad;
  topk_row((gptr<Idx>)indptr, seeds, num_rows, nnz, i, &lo, &hi, &bad);
  if (bad) return;
  const int64_t base = static_cast<int64_t>(out_indptr[i]);
  const int64_t picks = static_cast<int64_t>(out_indptr[i + 1]) - base;
  if (picks <= 0) return;
  const int64_t u = static_cast<int64_t>(seeds[i]), deg = hi - lo;
  int64_t* start = s_start + grp * TCAP;
  int64_t* cnt = s_n + grp * TCAP;
  int64_t* taken = s_taken + grp * TCAP;
  double* bs = s_b + grp * TCAP;
  {
    const gptr<Idx> off = (gptr<Idx>)(tag_offset + u * (T + 1));
    for (int64_t t = lg; t < T; t += W) {
      int64_t s, m;
      biased_range(off, t, deg, &s, &m);
      start[t] = s, cnt[t] = m, taken[t] = 0, bs[t] = biased_bias(bias[t]);
    }
  }
  unit_sync<W>();
  // the entry at row-relative position pos to slot p of the seed
  auto emit = [&](int64_t p, int64_t pos) {
    if (pos >= deg) pos = deg - 1;  // (cannot happen: a pick lies in a range of the row)
    out_nbr[base + p] = indices[lo + pos];
    out_eids[base + p] = static_cast<Idx>(topk_eid((gptr<Idx>)data, lo + pos));
  };

  if (fanout < 0) {  // every entry of the positive-bias ranges, no draw
    int64_t at = 0;
    for (int64_t c0 = 0; c0 < T; c0 += W) {
      const int64_t t = c0 + lg;
      const int64_t len = (t < T && bs[t] > 0.0) ? cnt[t] : 0;
      int64_t inc = len;
#pragma unroll
      for (int d = 1; d < W; d <<= 1) {
        const int64_t y = __shfl_up(inc, d, W);
        if (lg >= d) inc += y;
      }
      const int64_t st = t < T ? start[t] : 0;
      for (int l = 0; l < W && c0 + l < T; ++l) {
        const int64_t L = __shfl(len, l, W);
        if (L == 0) continue;
        const int64_t S0 = __shfl(st, l, W), O = at + __shfl(inc, l, W) - L;
        for (int64_t x = lg; x < L; x += W)
          if (O + x < picks) emit(O + x, S0 + x);
      }
      at += __shfl(inc, W - 1, W);
    }
    return;
  }

  // one chunk of the rule's scan: the weight of this lane's tag and its inclusive sum within the chunk
  auto chunk = [&](int64_t c0, double* w) -> double {
    const int64_t t = c0 + lg;
    *w = t < T ? biased_weight(cnt[t] - taken[t], bs[t]) : 0.0;
    double x = *w;
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
      const double y = __shfl_up(x, d, W);
      if (lg >= d) x = biased_add(x, y);
    }
    return x;
  };
  const uint64_t key = rw_walk_key(rng_seed, static_cast<uint64_t>(u));
  const bool rep = replace != 0;
  double total = 0.0;
  // phase A: the tag of every pick, staged in out_eids
  for (int64_t p = 0; p < picks; ++p) {
    if (!rep || p == 0) {
      total = 0.0;
      for (int64_t c0 = 0; c0 < T; c0 += W) {
        double w;
        const double x = chunk(c0, &w);
        total = biased_add(total, __shfl(x, W - 1, W));
      }
    }
    const double target = biased_target(rw_draw(rw_step_key(key, static_cast<uint64_t>(p)), kBiasedSlotTag), total);
    int64_t found = -1, last = -1;
    double carry = 0.0;
    for (int64_t c0 = 0; c0 < T && found < 0; c0 += W) {
      double w;
      const double x = chunk(c0, &w);
      const double pre = biased_add(carry, x);
      const uint64_t hit = group_bits<W>(__ballot(w > 0.0 && pre > target), lane);
      const uint64_t pos = group_bits<W>(__ballot(w > 0.0), lane);
      if (hit) found = c0 + __ffsll(static_cast<unsigned long long>(hit)) - 1;
      if (pos) last = c0 + 63 - __clzll(static_cast<long long>(pos));
      carry = biased_add(carry, __shfl(x, W - 1, W));
    }
    const int64_t t = found >= 0 ? found : (last >= 0 ? last : 0);
    if (lg == 0) {
      out_eids[base + p] = static_cast<Idx>(t);
      if (!rep) taken[t] += 1;
    }
    unit_sync<W>();
  }
  if (rep) {
    for (int64_t p = lg; p < picks; p += W) {
      const int64_t t = static_cast<int64_t>(out_eids[base + p]);
      const uint64_t r = rw_draw(rw_step_key(key, static_cast<uint64_t>(p)), kBiasedSlotPos);
      emit(p, start[t] + static_cast<int64_t>(rw_index(r, static_cast<uint64_t>(cnt[t]))));
    }
    return;
  }
  // phase B: Floyd's step per pick, the position within the tag's range staged in out_nbr
  for (int64_t p = 0; p < picks; ++p) {
    const int64_t t = static_cast<int64_t>(out_eids[base + p]);
    int64_t j = 0;
    for (int64_t q0 = 0; q0 < p; q0 += W) {
      const int64_t q = q0 + lg;
      const bool same = q < p && static_cast<int64_t>(out_eids[base + q]) == t;
      j += __popcll(group_bits<W>(__ballot(same), lane));
    }
    const int64_t m = biased_floyd_m(cnt[t], taken[t], j);
    const uint64_t r = rw_draw(rw_step_key(key, static_cast<uint64_t>(p)), kBiasedSlotPos);
    const int64_t c = static_cast<int64_t>(rw_index(r, static_cast<uint64_t>(m + 1)));
    bool used = false;
    for (int64_t q0 = 0; q0 < p; q0 += W) {
      const int64_t q = q0 + lg;
      const bool hit = q < p && static_cast<int64_t>(out_eids[base + q]) == t && static_cast<int64_t>(out_nbr[base + q]) == c;
      used = used || group_bits<W>(__ballot(hit), lane) != 0;
    }
    if (lg == 0) out_nbr[base + p] = static_cast<Idx>(used ? m : c);
    unit_sync<W>();
  }
  // phase C: the gather
  for (int64_t p = lg; p < picks; p += W) {
    const int64_t t = static_cast<int64_t>(out_eids[base + p]);
    emit(p, start[t] + static_cast<int64_t>(out_nbr[base + p]));
  }
}

// ---- host side --------------------------------------------------------------------------------------
struct BiasedLayout {  // offsets into the workspace of dgla_sample_neighbors_biased
  SeedScan head;
  size_t flags, bytes;
};

BiasedLayout biased_layout(int64_t n) {
  BiasedLayout L{};
  Carver c;
  L.head = take_seed_scan(c, n, msd::scan_temp_bytes(n + 1, sizeof(int64_t)));
  L.flags = c.take(sizeof(int) * kFwWords);
  L.bytes = c.bytes();
  return L;
}

int biased_bad_tag(const char* who, int64_t T) { return fail(who, "a tag lies outside [0, " + std::to_string(T) + ")"); }
int biased_bad_eid(const char* who, int64_t nnz) {
  return fail(who, "an edge id of the csr lies outside [0, " + std::to_string(nnz) + ")");
}

// everything the two sort entry points refuse before they read an array
int check_sort(const char* who, const dgla_csr* csr, const void* tag, int tag_bits, int64_t num_tags, const void* out_indices,
               const void* out_data, const void* tag_pos) {
  if (check_csr(who, csr)) return -1;
  if (!idbits_ok(tag_bits)) return fail(who, "unsupported tag dtype of " + std::to_string(tag_bits) + " bits (int32 and int64 are accepted)");
  if (num_tags < 1) return fail(who, "num_tags must be positive, got " + std::to_string(num_tags));
  if (!tag && csr->nnz > 0) return fail(who, "tag is null");
  if (csr->nnz > 0 && (!out_indices || !out_data)) return fail(who, "out_indices or out_data is null");
  if (csr->num_rows > 0 && !tag_pos) return fail(who, "tag_pos is null");
  return 0;
}

// everything the two sampler entry points refuse before they read an array
int check_biased(const char* who, const dgla_csr* csr, const void* tag_offset, int64_t num_tags, const void* bias, int bias_dtype,
                 const void* seeds, int64_t num_seeds, int64_t fanout, const void* out_indptr, const void* out_nbr,
                 const void* out_eids) {
  if (check_csr(who, csr)) return -1;
  if (bias_dtype != kF32 && bias_dtype != kF64)
    return fail(who, "unsupported bias dtype " + std::to_string(bias_dtype) + " (fp32 and fp64 are accepted)");
  if (num_tags < 1) return fail(who, "num_tags must be positive, got " + std::to_string(num_tags));
  if (num_tags > kBiasedMaxTags)
    return fail(who, "num_tags " + std::to_string(num_tags) + " exceeds the limit of " + std::to_string(kBiasedMaxTags) + " tags");
  if (!bias) return fail(who, "bias is null");
  if (!tag_offset && csr->num_rows > 0) return fail(who, "tag_offset is null");
  if (check_seeds(who, seeds, num_seeds)) return -1;
  if (fanout < -1) return fail(who, "fanout must be -1 (all), 0 or positive, got " + std::to_string(fanout));
  return check_seed_outputs(who, out_indptr, out_nbr, out_eids);
}

// ---- the rules run by the CPU -----------------------------------------------------------------------
template <typename Idx, typename Tag>
int sort_by_tag_host(const char* who, const TypedCsr<Idx>& g, const Tag* tag, int64_t T, Idx* out_indices, Idx* out_data,
                     Idx* tag_pos) {
  auto bounds = [&](int64_t row, int64_t* lo, int64_t* hi) {
    int64_t a = static_cast<int64_t>(g.indptr[row]), b = static_cast<int64_t>(g.indptr[row + 1]);
    a = a < 0 ? 0 : (a > g.nnz ? g.nnz : a);
    b = b < a ? a : (b > g.nnz ? g.nnz : b);
    *lo = a, *hi = b;
  };
  int fl = 0;  // refusals that need the arrays, before anything is written
  for (int64_t row = 0; row < g.num_rows; ++row) {
    int64_t lo, hi;
    bounds(row, &lo, &hi);
    for (int64_t q = lo; q < hi; ++q) biased_tag(tag, g.nnz, T, topk_eid(g.data, q), &fl);
  }
  if (fl & kBiasedBadEid) return biased_bad_eid(who, g.nnz);
  if (fl & kBiasedBadTag) return biased_bad_tag(who, T);
  for (int64_t row = 0; row < g.num_rows; ++row) {
    int64_t lo, hi;
    bounds(row, &lo, &hi);
    Idx* c = tag_pos + row * (T + 1);
    for (int64_t j = 0; j <= T; ++j) c[j] = 0;
    for (int64_t q = lo; q < hi; ++q) c[biased_tag(tag, g.nnz, T, topk_eid(g.data, q), &fl) + 1] += 1;
    Idx sum = 0;  // slot t + 1 = the offset of tag t, then its cursor
    for (int64_t j = 1; j <= T; ++j) {
      const Idx own = c[j];
      c[j] = sum;
      sum += own;
    }
    for (int64_t q = lo; q < hi; ++q) {
      const int64_t e = topk_eid(g.data, q);
      const int64_t t = biased_tag(tag, g.nnz, T, e, &fl);
      const int64_t rank = static_cast<int64_t>(c[t + 1]);
      c[t + 1] += 1;
      out_indices[lo + rank] = g.indices[q];
      out_data[lo + rank] = static_cast<Idx>(e);
    }
  }
  return 0;
}

template <typename Idx, typename B>
int sample_biased_host(const char* who, const TypedCsr<Idx>& g, const Idx* tag_offset, int64_t T, const B* bias,
                       const SeedCsrOut<Idx>& o, int64_t n, int64_t fanout, bool rep, uint64_t rng_seed) {
  const Idx* seeds = o.seeds;
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo, hi;
    bool bad;
    topk_row(g.indptr, seeds, g.num_rows, g.nnz, i, &lo, &hi, &bad);
    if (bad) return bad_seed(who, g.num_rows);
  }
  const int W = biased_width(T);
  const int64_t TP = (T + W - 1) / W * W;
  std::vector<int64_t> start(TP, 0), cnt(TP, 0), taken(TP, 0), tags, rel;
  std::vector<double> bs(TP, 0.0), w(W), x(W);
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo, hi;
    bool bad;
    topk_row(g.indptr, seeds, g.num_rows, g.nnz, i, &lo, &hi, &bad);
    const int64_t u = static_cast<int64_t>(seeds[i]), deg = hi - lo;
    const Idx* off = tag_offset + u * (T + 1);
    const int64_t picks = biased_picks(biased_positive(off, bias, T, deg), fanout, rep);
    o.indptr[i] = static_cast<Idx>(at);
    if (picks == 0 || !o.nbr) {
      at += picks;
      continue;
    }
    for (int64_t t = 0; t < T; ++t) {
      biased_range(off, t, deg, &start[t], &cnt[t]);
      taken[t] = 0, bs[t] = biased_bias(bias[t]);
    }
    auto emit = [&](int64_t p, int64_t pos) {
      if (pos >= deg) pos = deg - 1;
      o.nbr[at + p] = g.indices[lo + pos];
      o.eids[at + p] = static_cast<Idx>(topk_eid(g.data, lo + pos));
    };
    if (fanout < 0) {
      int64_t p = 0;
      for (int64_t t = 0; t < T; ++t)
        if (bs[t] > 0.0)
          for (int64_t k = 0; k < cnt[t]; ++k) emit(p++, start[t] + k);
      at += picks;
      continue;
    }
    // one chunk of the scan, as the lanes run it
    auto chunk = [&](int64_t c0) {
      for (int l = 0; l < W; ++l) x[l] = w[l] = c0 + l < T ? biased_weight(cnt[c0 + l] - taken[c0 + l], bs[c0 + l]) : 0.0;
      biased_scan_host(x.data(), W);
    };
    const uint64_t key = rw_walk_key(rng_seed, static_cast<uint64_t>(u));
    tags.assign(picks, 0);
    rel.assign(picks, 0);
    double total = 0.0;
    for (int64_t p = 0; p < picks; ++p) {
      if (!rep || p == 0) {
        total = 0.0;
        for (int64_t c0 = 0; c0 < T; c0 += W) {
          chunk(c0);
          total = biased_add(total, x[W - 1]);
        }
      }
      const double target = biased_target(rw_draw(rw_step_key(key, static_cast<uint64_t>(p)), kBiasedSlotTag), total);
      int64_t found = -1, last = -1;
      double carry = 0.0;
      for (int64_t c0 = 0; c0 < T && found < 0; c0 += W) {
        chunk(c0);
        for (int l = 0; l < W; ++l) {
          if (w[l] > 0.0 && found < 0 && biased_add(carry, x[l]) > target) found = c0 + l;
          if (w[l] > 0.0) last = c0 + l;
        }
        carry = biased_add(carry, x[W - 1]);
      }
      const int64_t t = found >= 0 ? found : (last >= 0 ? last : 0);
      tags[p] = t;
      if (!rep) taken[t] += 1;
    }
    for (int64_t p = 0; p < picks; ++p) {
      const int64_t t = tags[p];
      const uint64_t r = rw_draw(rw_step_key(key, static_cast<uint64_t>(p)), kBiasedSlotPos);
      if (rep) {
        emit(p, start[t] + static_cast<int64_t>(rw_index(r, static_cast<uint64_t>(cnt[t]))));
        continue;
      }
      int64_t j = 0;
      for (int64_t q = 0; q < p; ++q) j += tags[q] == t;
      const int64_t m = biased_floyd_m(cnt[t], taken[t], j);
      const int64_t c = static_cast<int64_t>(rw_index(r, static_cast<uint64_t>(m + 1)));
      bool used = false;
      for (int64_t q = 0; q < p; ++q) used = used || (tags[q] == t && rel[q] == c);
      rel[p] = used ? m : c;
      emit(p, start[t] + rel[p]);
    }
    at += picks;
  }
  o.indptr[n] = static_cast<Idx>(at);
  return 0;
}

template <typename Idx, typename Tag, int NT, int G>
void launch_sort(const TypedCsr<Idx>& g, const Tag* tag, int64_t T, Idx* out_indices, Idx* out_data, Idx* tag_pos, int* flags,
                 hipStream_t s) {
  const dim3 grid(grid1(g.num_rows, NT / G)), block(NT);
  if (T <= kSortLdsTags)
    hipLaunchKernelGGL((tag_sort_kernel<Idx, Tag, NT, G, true>), grid, block, 0, s, g.indptr, g.indices, g.data, tag, g.num_rows,
                       g.nnz, T, out_indices, out_data, tag_pos, flags);
  else
    hipLaunchKernelGGL((tag_sort_kernel<Idx, Tag, NT, G, false>), grid, block, 0, s, g.indptr, g.indices, g.data, tag, g.num_rows,
                       g.nnz, T, out_indices, out_data, tag_pos, flags);
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

int dgla_sort_csr_by_tag(const dgla_csr* csr, const void* tag, int tag_bits, int64_t num_tags, void* out_indices, void* out_data,
                         void* tag_pos, void* hip_stream) {
  const char* who = "sort_csr_by_tag";
  if (check_sort(who, csr, tag, tag_bits, num_tags, out_indices, out_data, tag_pos)) return -1;
  if (csr->num_rows == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, tag_pos);
  Scratch scratch(s);
  if (scratch.take(nullptr, 0, sizeof(int) * kFwWords)) return -1;
  int* flags = reinterpret_cast<int*>(scratch.p);
  DGLA_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int) * kFwWords, s));
  const int64_t T = num_tags;
  const bool short_rows = csr->nnz / csr->num_rows <= kSortShortMean;
  int fl[kFwWords];
  const int rc = with_idx(csr->idtype_bits, [&](auto id) -> int {
    using Idx = decltype(id);
    return with_idx(tag_bits, [&](auto tg) -> int {
      using Tag = decltype(tg);
      const TypedCsr<Idx> g(csr);
      const Tag* tp = static_cast<const Tag*>(tag);
      Idx *oi = static_cast<Idx*>(out_indices), *od = static_cast<Idx*>(out_data), *pos = static_cast<Idx*>(tag_pos);
      if (short_rows)
        launch_sort<Idx, Tag, 64, 16>(g, tp, T, oi, od, pos, flags, s);
      else
        launch_sort<Idx, Tag, 64, 64>(g, tp, T, oi, od, pos, flags, s);
      if (read_back(fl, flags, sizeof(fl), s)) return -1;
      if (fl[kFwHub]) {  // the rows the lane groups left to a workgroup
        launch_sort<Idx, Tag, 256, 256>(g, tp, T, oi, od, pos, flags, s);
        if (read_back(fl, flags, sizeof(fl), s)) return -1;
      }
      return 0;
    });
  });
  if (rc) return -1;
  if (fl[kFwBadEid]) return biased_bad_eid(who, csr->nnz);
  if (fl[kFwBadTag]) return biased_bad_tag(who, T);
  return 0;
}

int dgla_sort_csr_by_tag_host(const dgla_csr* csr, const void* tag, int tag_bits, int64_t num_tags, void* out_indices,
                              void* out_data, void* tag_pos) {
  const char* who = "sort_csr_by_tag_host";
  if (check_sort(who, csr, tag, tag_bits, num_tags, out_indices, out_data, tag_pos)) return -1;
  return with_idx(csr->idtype_bits, [&](auto id) -> int {
    using Idx = decltype(id);
    return with_idx(tag_bits, [&](auto tg) -> int {
      using Tag = decltype(tg);
      return sort_by_tag_host<Idx, Tag>(who, TypedCsr<Idx>(csr), static_cast<const Tag*>(tag), num_tags,
                                        static_cast<Idx*>(out_indices), static_cast<Idx*>(out_data), static_cast<Idx*>(tag_pos));
    });
  });
}

size_t dgla_sample_neighbors_biased_workspace_bytes(int idtype_bits, int64_t num_seeds) {
  if (!idbits_ok(idtype_bits) || num_seeds <= 0) return 0;
  return biased_layout(num_seeds).bytes;
}

int dgla_sample_neighbors_biased(const dgla_csr* csr, const void* tag_offset, int64_t num_tags, const void* bias, int bias_dtype,
                                 const void* seeds, int64_t num_seeds, int64_t fanout, int replace, uint64_t rng_seed,
                                 void* out_indptr, void* out_nbr, void* out_eids, void* workspace, size_t workspace_bytes,
                                 void* hip_stream) {
  const char* who = "sample_neighbors_biased";
  if (check_biased(who, csr, tag_offset, num_tags, bias, bias_dtype, seeds, num_seeds, fanout, out_indptr, out_nbr, out_eids))
    return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_indptr);
  const int64_t n = num_seeds, T = num_tags;
  if (n == 0) {  // (out_indptr[0] = 0, in either id width)
    hipLaunchKernelGGL(biased_clear_kernel, dim3(1), dim3(64), 0, s, static_cast<int*>(out_indptr), csr->idtype_bits / 32);
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const BiasedLayout L = biased_layout(n);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  int64_t* picks = reinterpret_cast<int64_t*>(scratch.p + L.head.picks);
  int* flags = reinterpret_cast<int*>(scratch.p + L.flags);
  hipLaunchKernelGGL(biased_clear_kernel, dim3(1), dim3(64), 0, s, flags, static_cast<int>(kFwWords));
  const int rc = with_idx(csr->idtype_bits, [&](auto id) -> int {
    using Idx = decltype(id);
    return with_float(bias_dtype, [&](auto bt) -> int {
      using B = decltype(bt);
      const TypedCsr<Idx> g(csr);
      const SeedCsrOut<Idx> o(seeds, out_indptr, out_nbr, out_eids);
      const Idx* off = static_cast<const Idx*>(tag_offset);
      const B* b = static_cast<const B*>(bias);
      hipLaunchKernelGGL((biased_count_kernel<Idx, B>), dim3(grid1(n + 1, kBiasedCountBlock)), dim3(kBiasedCountBlock), 0, s,
                         g.indptr, off, b, o.seeds, n, g.num_rows, g.nnz, T, fanout, replace, picks, flags);
      if (msd::exclusive_scan<int64_t, Idx>(picks, o.indptr, n + 1, scratch.p + L.head.scan, s)) return -1;
      if (fanout < 0) {  // the sizes depend on the graph: the flag words come back before the pick launch
        int fl[kFwWords];
        if (read_back(fl, flags, sizeof(fl), s)) return -1;
        if (fl[kFwBadSeed]) return bad_seed(who, g.num_rows);
      }
      if (!o.nbr || fanout == 0) return 0;
      if (biased_width(T) == 16)
        hipLaunchKernelGGL((biased_pick_kernel<Idx, B, 16, 16>), dim3(grid1(n, 4)), dim3(64), 0, s, g.indptr, g.indices, g.data, off,
                           b, o.seeds, n, g.num_rows, g.nnz, T, fanout, replace, rng_seed, o.indptr, o.nbr, o.eids);
      else if (T <= kBiasedCapSmall)
        hipLaunchKernelGGL((biased_pick_kernel<Idx, B, 64, kBiasedCapSmall>), dim3(grid1(n, 1)), dim3(64), 0, s, g.indptr, g.indices,
                           g.data, off, b, o.seeds, n, g.num_rows, g.nnz, T, fanout, replace, rng_seed, o.indptr, o.nbr, o.eids);
      else
        hipLaunchKernelGGL((biased_pick_kernel<Idx, B, 64, kBiasedMaxTags>), dim3(grid1(n, 1)), dim3(64), 0, s, g.indptr, g.indices,
                           g.data, off, b, o.seeds, n, g.num_rows, g.nnz, T, fanout, replace, rng_seed, o.indptr, o.nbr, o.eids);
      return 0;
    });
  });
  if (rc) return -1;
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_sample_neighbors_biased_host(const dgla_csr* csr, const void* tag_offset, int64_t num_tags, const void* bias,
                                      int bias_dtype, const void* seeds, int64_t num_seeds, int64_t fanout, int replace,
                                      uint64_t rng_seed, void* out_indptr, void* out_nbr, void* out_eids) {
  const char* who = "sample_neighbors_biased_host";
  if (check_biased(who, csr, tag_offset, num_tags, bias, bias_dtype, seeds, num_seeds, fanout, out_indptr, out_nbr, out_eids))
    return -1;
  return with_idx(csr->idtype_bits, [&](auto id) -> int {
    using Idx = decltype(id);
    return with_float(bias_dtype, [&](auto bt) -> int {
      using B = decltype(bt);
      return sample_biased_host<Idx, B>(who, TypedCsr<Idx>(csr), static_cast<const Idx*>(tag_offset), num_tags,
                                        static_cast<const B*>(bias), SeedCsrOut<Idx>(seeds, out_indptr, out_nbr, out_eids),
                                        num_seeds, fanout, replace != 0, rng_seed);
    });
  });
}

}  // extern "C"
