// Per-edge-type neighbour sampling on the device: dgl.sampling.sample_etype_neighbors.
//
// Reference: CSRRowWisePerEtypePick (src/array/cpu/rowwise_pick.h:334) behind python/dgl/sampling/neighbor.py:69 exists for
// the CPU only, so a mini-batch step on a homogenised graph copies its frontier to the host and back.
//
// MI355X-first choices:
//  * The rule is that of csrc/etype_step.h, compiled here for the kernels and for the host twin.
//  * A lane group owns a seed (16 lanes when T <= 16, else a wavefront) and A LANE OWNS AN EDGE TYPE, in chunks of the
//    group's width.  etype_offset and fanout are staged in LDS once per workgroup (T <= 1024: 16 KB at most).
//  * The lane bisects both boundaries of its type in the row side by side: log2(deg) dependent steps of two loads,
//    issued by all lanes of the group at once, so T bisections cost the latency of one.
//  * The per-type pick counts become slice offsets through an integer lane scan; no atomics, and the slices of a seed
//    follow each other by type.
//  * Unweighted ranges are picked by their own lane: Floyd's step with the positions in registers up to a fan-out of 32
//    (every loop unrolled to that bound and predicated), staged in the range's own output slice beyond.  Nothing but
//    the gather of the picks touches memory: the cost per seed does not grow with its degree.
//  * Weighted ranges, and ranges taken whole, are streamed by the WHOLE group with coalesced loads, one type after the
//    other: exponential-clock keys are recomputed in registers from the counter-based generator, one pick per round by a
//    lane argmin.  No key array, no sort.
//  * One kernel body serves the count pass and the pick pass (count + device scan + fill).  The entry point reads
//    nothing back and, given a workspace, allocates nothing: the call can be captured.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>

#include "host_util.h"
#include "sort.hip.h"
#include "etype_step.h"

namespace dgla {
namespace {

constexpr int kEtypeBlock = 256;

__global__ void etype_zero_kernel(int* words, int n) {
  if (static_cast<int>(threadIdx.x) < n) words[threadIdx.x] = 0;
}

// the bits of this lane's group in a wavefront ballot
template <int W>
__device__ __forceinline__ uint64_t etype_bits(uint64_t ballot, int lane) {
  if constexpr (W >= 64) {
    return ballot;
  } else {
    return (ballot >> (lane & ~(W - 1))) & ((uint64_t(1) << W) - 1);
  }
}

template <int W, typename T>
__device__ __forceinline__ T etype_bcast(T v, int l) {
  return static_cast<T>(__shfl(static_cast<long long>(v), l, W));
}

// what the group needs to know about one range that it serves together
template <typename P>
struct EtypeRange {
  int64_t start, n, b0, b1, f, cnt, pos, slot;   // pos = P_t, slot = the first output slot of the range
  const P* prob;                                 // nullptr: every entry weighs 1
};

// PICK = false: picks[i] = the number of picks of seed i (picks[n] = 0 closes the scan).  PICK = true: the picks.
template <typename Idx, typename P, int W, bool PICK>
__global__ __launch_bounds__(kEtypeBlock) void etype_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                            const Idx* __restrict__ data, const int64_t* __restrict__ etype_offset,
                                                            const int64_t* __restrict__ fanout, const P* const* __restrict__ prob,
                                                            const Idx* __restrict__ seeds, int64_t n, int64_t num_rows, int64_t nnz,
                                                            int64_t T, int replace, uint64_t rng_seed, int64_t* __restrict__ picks,
                                                            const Idx* __restrict__ out_indptr, Idx* out_nbr, Idx* out_eids,
                                                            int64_t cap) {
  constexpr int R = kEtypeBlock / W;
  extern __shared__ int64_t s_tab[];   // etype_offset[T + 1], then fanout[T]
  int64_t* s_off = s_tab;
  int64_t* s_fan = s_tab + T + 1;
  for (int64_t j = threadIdx.x; j <= T; j += kEtypeBlock) s_off[j] = etype_offset[j];
  for (int64_t j = threadIdx.x; j < T; j += kEtypeBlock) s_fan[j] = fanout[j];
  __syncthreads();
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (W - 1), grp = threadIdx.x / W;
  const int64_t i = blockIdx.x * static_cast<int64_t>(R) + grp;
  if (i > n || (PICK && i == n)) return;
  int64_t lo = 0, hi = 0;
  bool bad = true;
  if (i < n) topk_row((gptr<Idx>)indptr, seeds, num_rows, nnz, i, &lo, &hi, &bad);
  if (bad) {  // (the closing slot, or a seed outside the graph: an empty row that touches no memory)
    if (!PICK && lg == 0) picks[i] = 0;
    return;
  }
  const int64_t u = static_cast<int64_t>(seeds[i]), deg = hi - lo;
  const bool rep = replace != 0;
  int64_t base = 0;
  if constexpr (PICK) base = static_cast<int64_t>(out_indptr[i]);
  const gptr<Idx> dat = (gptr<Idx>)data;

  // the entry at row-relative position pos to output slot `slot`
  auto emit = [&](int64_t slot, int64_t pos) {
    if (slot >= cap || pos >= deg) return;  // (pos < deg always: a pick lies in a range of the row)
    out_nbr[slot] = indices[lo + pos];
    out_eids[slot] = static_cast<Idx>(topk_eid(dat, lo + pos));
  };
  // the weight of range-relative position x of a range the group serves
  auto weight = [&](const EtypeRange<P>& g, int64_t x) -> double {
    if (x >= g.n) return 0.0;
    if (!g.prob) return 1.0;
    return etype_weight<P>(g.prob, topk_eid(dat, lo + g.start + x), g.b0, g.b1);
  };
  // lane l's range to every lane of the group
  auto share = [&](const EtypeRange<P>& mine, int l) {
    EtypeRange<P> g;
    g.start = etype_bcast<W>(mine.start, l), g.n = etype_bcast<W>(mine.n, l);
    g.b0 = etype_bcast<W>(mine.b0, l), g.b1 = etype_bcast<W>(mine.b1, l);
    g.f = etype_bcast<W>(mine.f, l), g.cnt = etype_bcast<W>(mine.cnt, l);
    g.pos = etype_bcast<W>(mine.pos, l), g.slot = etype_bcast<W>(mine.slot, l);
    g.prob = reinterpret_cast<const P*>(etype_bcast<W>(reinterpret_cast<uint64_t>(mine.prob), l));
    return g;
  };

  int64_t at = 0;
  for (int64_t c0 = 0; c0 < T; c0 += W) {
    const int64_t t = c0 + lg;
    const bool live = t < T;
    EtypeRange<P> my{};
    my.b0 = live ? s_off[t] : 0, my.b1 = live ? s_off[t + 1] : 0, my.f = live ? s_fan[t] : 0;
    if (live && my.f != 0 && deg > 0) etype_range(dat, lo, deg, my.b0, my.b1, &my.start, &my.n);
    my.prob = (prob && live) ? prob[t] : nullptr;
    my.pos = my.n;
    // P_t of the weighted ranges: the group streams them, one after the other
    for (uint64_t todo = etype_bits<W>(__ballot(my.prob && my.n > 0), lane); todo; todo &= todo - 1) {
      const int l = __ffsll(static_cast<unsigned long long>(todo)) - 1;
      const EtypeRange<P> g = share(my, l);
      int64_t count = 0;
      for (int64_t x0 = 0; x0 < g.n; x0 += W)
        count += __popcll(etype_bits<W>(__ballot(weight(g, x0 + lg) > 0.0), lane));
      if (lg == l) my.pos = count;
    }
    my.cnt = etype_picks(my.pos, my.f, rep);
    int64_t inc = my.cnt;
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
      const int64_t y = __shfl_up(inc, d, W);
      if (lg >= d) inc += y;
    }
    my.slot = base + at + inc - my.cnt;
    at += __shfl(inc, W - 1, W);
    if constexpr (PICK) {
      const bool whole = my.f < 0 || (!rep && my.pos <= my.f);
      const bool shared = my.cnt > 0 && (my.prob || whole);
      // ranges the lane picks alone: unweighted draws, arithmetic and the gather of the picks only
      if (my.cnt > 0 && !shared) {
        const uint64_t key = etype_key(rng_seed, u, t);
        if (rep) {
          for (int64_t k = 0; k < my.f; ++k)
            emit(my.slot + k, my.start + static_cast<int64_t>(rw_index(rw_draw(key, static_cast<uint64_t>(k)), static_cast<uint64_t>(my.n))));
        } else if (my.f <= kEtypeRegPicks) {
          int64_t chosen[kEtypeRegPicks];
#pragma unroll
          for (int m = 0; m < kEtypeRegPicks; ++m) {
            if (m < my.f) {
              int64_t c, j;
              etype_floyd(key, my.n, my.f, m, &c, &j);
              bool dup = false;
#pragma unroll
              for (int q = 0; q < kEtypeRegPicks; ++q)
                if (q < m) dup = dup || chosen[q] == c;
              chosen[m] = dup ? j : c;
            }
          }
#pragma unroll
          for (int m = 0; m < kEtypeRegPicks; ++m)
            if (m < my.f) emit(my.slot + m, my.start + chosen[m]);
        } else {  // the positions wait in the range's own slice of out_nbr, which this lane alone owns
          for (int64_t m = 0; m < my.f; ++m) {
            int64_t c, j;
            etype_floyd(key, my.n, my.f, m, &c, &j);
            bool dup = false;
            for (int64_t q = 0; q < m && my.slot + q < cap; ++q) dup = dup || static_cast<int64_t>(out_nbr[my.slot + q]) == c;
            if (my.slot + m < cap) out_nbr[my.slot + m] = static_cast<Idx>(dup ? j : c);
          }
          for (int64_t m = 0; m < my.f && my.slot + m < cap; ++m) emit(my.slot + m, my.start + static_cast<int64_t>(out_nbr[my.slot + m]));
        }
      }
      // ranges the group serves together: taken whole, or weighted
      for (uint64_t todo = etype_bits<W>(__ballot(shared), lane); todo; todo &= todo - 1) {
        const int l = __ffsll(static_cast<unsigned long long>(todo)) - 1;
        const EtypeRange<P> g = share(my, l);
        const uint64_t key = etype_key(rng_seed, u, c0 + l);
        if (g.f < 0 || (!rep && g.pos <= g.f)) {  // every positive entry in position order
          int64_t done = 0;
          for (int64_t x0 = 0; x0 < g.n; x0 += W) {
            const bool on = weight(g, x0 + lg) > 0.0;
            const uint64_t bits = etype_bits<W>(__ballot(on), lane);
            if (on) emit(g.slot + done + __popcll(bits & ((uint64_t(1) << lg) - 1)), g.start + x0 + lg);
            done += __popcll(bits);
          }
        } else if (!rep) {  // the cnt smallest (key, position): one round per pick, keys recomputed
          double last_key = -1.0;  // keys are >= 0
          int64_t last_x = -1;
          for (int64_t p = 0; p < g.cnt; ++p) {
            double best = __builtin_huge_val();
            int64_t best_x = 0x7fffffffffffffffLL;
            for (int64_t x = lg; x < g.n; x += W) {
              const double w = weight(g, x);
              if (!(w > 0.0)) continue;
              const double k = etype_clock(key, x, w);
              if (etype_before(last_key, last_x, k, x) && etype_before(k, x, best, best_x)) best = k, best_x = x;
            }
#pragma unroll
            for (int m = W / 2; m >= 1; m >>= 1) {
              const double ok = __shfl_xor(best, m, W);
              const int64_t ox = __shfl_xor(best_x, m, W);
              if (etype_before(ok, ox, best, best_x)) best = ok, best_x = ox;
            }
            if (lg == 0 && best_x < g.n) emit(g.slot + p, g.start + best_x);
            last_key = best, last_x = best_x;
          }
        } else {  // with replacement: the total, then one prefix walk per pick, in the rule's order of additions
          auto chunk = [&](int64_t x0, double* w) -> double {
            *w = weight(g, x0 + lg);
            double x = *w;
#pragma unroll
            for (int d = 1; d < W; d <<= 1) {
              const double y = __shfl_up(x, d, W);
              if (lg >= d) x = biased_add(x, y);
            }
            return x;
          };
          double total = 0.0;
          for (int64_t x0 = 0; x0 < g.n; x0 += W) {
            double w;
            const double x = chunk(x0, &w);
            total = biased_add(total, __shfl(x, W - 1, W));
          }
          for (int64_t p = 0; p < g.cnt; ++p) {
            const double target = biased_target(rw_draw(key, static_cast<uint64_t>(p)), total);
            int64_t found = -1, last = -1;
            double carry = 0.0;
            for (int64_t x0 = 0; x0 < g.n && found < 0; x0 += W) {
              double w;
              const double x = chunk(x0, &w);
              const uint64_t hit = etype_bits<W>(__ballot(w > 0.0 && biased_add(carry, x) > target), lane);
              const uint64_t on = etype_bits<W>(__ballot(w > 0.0), lane);
              if (hit) found = x0 + __ffsll(static_cast<unsigned long long>(hit)) - 1;
              if (on) last = x0 + 63 - __clzll(static_cast<long long>(on));
              carry = biased_add(carry, __shfl(x, W - 1, W));
            }
            if (found < 0) found = last;
            if (lg == 0 && found >= 0) emit(g.slot + p, g.start + found);
          }
        }
      }
    }
  }
  if (!PICK && lg == 0) picks[i] = at;
}

// ---- host side --------------------------------------------------------------------------------------
struct EtypeLayout {  // offsets into the workspace of dgla_sample_etype_neighbors
  SeedScan head;
  size_t bytes;
};

EtypeLayout etype_layout(int64_t n) {
  EtypeLayout L{};
  Carver c;
  L.head = take_seed_scan(c, n, msd::scan_temp_bytes(n + 1, sizeof(int64_t)));
  L.bytes = c.bytes();
  return L;
}

// everything the two entry points refuse before they read an array
int check_etype(const char* who, const dgla_csr* csr, const int64_t* etype_offset, const int64_t* fanout, int64_t T,
                const void* const* prob, int prob_dtype, const void* seeds, int64_t num_seeds, const void* out_indptr,
                const void* out_nbr, const void* out_eids, int64_t out_capacity) {
  if (check_csr(who, csr)) return -1;
  if (T < 1) return fail(who, "num_etypes must be positive, got " + std::to_string(T));
  if (T > kEtypeMaxTypes)
    return fail(who, "num_etypes " + std::to_string(T) + " exceeds the limit of " + std::to_string(kEtypeMaxTypes) + " edge types");
  if (!etype_offset) return fail(who, "etype_offset is null");
  if (!fanout) return fail(who, "fanout is null");
  if (prob && prob_dtype != kF32 && prob_dtype != kF64 && prob_dtype != kEtypeU8)
    return fail(who, "unsupported prob dtype " + std::to_string(prob_dtype) + " (fp32, fp64 and uint8 are accepted)");
  if (check_seeds(who, seeds, num_seeds) || check_seed_outputs(who, out_indptr, out_nbr, out_eids)) return -1;
  if (out_nbr && out_capacity < 0) return fail(who, "negative out_capacity");
  return 0;
}

// f(P{}) with P = float, double or uint8_t: the prob type of a call (float when there is none)
template <typename F>
int with_prob(const void* prob, int dtype, F&& f) {
  if (!prob || dtype == kF32) return f(float{});
  if (dtype == kF64) return f(double{});
  return f(uint8_t{});
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename Idx, typename P>
int sample_etype_host(const char* who, const TypedCsr<Idx>& g, const int64_t* off, const int64_t* fan, int64_t T,
                      const P* const* prob, const SeedCsrOut<Idx>& o, int64_t n, bool rep, uint64_t rng_seed, int64_t cap) {
  const int W = etype_width(T);
  std::vector<double> w(W), x(W);
  std::vector<int64_t> chosen;
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo, hi;
    bool bad;
    topk_row(g.indptr, o.seeds, g.num_rows, g.nnz, i, &lo, &hi, &bad);
    o.indptr[i] = static_cast<Idx>(at);
    if (bad) continue;
    const int64_t u = static_cast<int64_t>(o.seeds[i]), deg = hi - lo;
    auto emit = [&](int64_t slot, int64_t pos) {
      if (slot >= cap || pos >= deg) return;
      o.nbr[slot] = g.indices[lo + pos];
      o.eids[slot] = static_cast<Idx>(topk_eid(g.data, lo + pos));
    };
    for (int64_t t = 0; t < T; ++t) {
      const int64_t b0 = off[t], b1 = off[t + 1], f = fan[t];
      int64_t start = 0, nt = 0;
      if (f != 0 && deg > 0) etype_range(g.data, lo, deg, b0, b1, &start, &nt);
      const P* pt = prob ? prob[t] : nullptr;
      auto weight = [&](int64_t k) -> double {
        if (k >= nt) return 0.0;
        return pt ? etype_weight<P>(pt, topk_eid(g.data, lo + start + k), b0, b1) : 1.0;
      };
      int64_t pos = nt;
      if (pt) {
        pos = 0;
        for (int64_t k = 0; k < nt; ++k) pos += weight(k) > 0.0;
      }
      const int64_t cnt = etype_picks(pos, f, rep), slot = at;
      at += cnt;
      if (!o.nbr || cnt == 0) continue;
      const uint64_t key = etype_key(rng_seed, u, t);
      if (f < 0 || (!rep && pos <= f)) {
        int64_t done = 0;
        for (int64_t k = 0; k < nt; ++k)
          if (weight(k) > 0.0) emit(slot + done++, start + k);
      } else if (!pt && rep) {
        for (int64_t k = 0; k < f; ++k)
          emit(slot + k, start + static_cast<int64_t>(rw_index(rw_draw(key, static_cast<uint64_t>(k)), static_cast<uint64_t>(nt))));
      } else if (!pt) {
        chosen.assign(f, 0);
        for (int64_t m = 0; m < f; ++m) {
          int64_t c, j;
          etype_floyd(key, nt, f, m, &c, &j);
          bool dup = false;
          for (int64_t q = 0; q < m; ++q) dup = dup || chosen[q] == c;
          chosen[m] = dup ? j : c;
          emit(slot + m, start + chosen[m]);
        }
      } else if (!rep) {
        double last_key = -1.0;
        int64_t last_x = -1;
        for (int64_t p = 0; p < cnt; ++p) {
          double best = __builtin_huge_val();
          int64_t best_x = 0x7fffffffffffffffLL;
          for (int64_t k = 0; k < nt; ++k) {
            const double wk = weight(k);
            if (!(wk > 0.0)) continue;
            const double ck = etype_clock(key, k, wk);
            if (etype_before(last_key, last_x, ck, k) && etype_before(ck, k, best, best_x)) best = ck, best_x = k;
          }
          if (best_x < nt) emit(slot + p, start + best_x);
          last_key = best, last_x = best_x;
        }
      } else {
        auto chunk = [&](int64_t x0) {  // as the lanes run it
          for (int l = 0; l < W; ++l) x[l] = w[l] = weight(x0 + l);
          biased_scan_host(x.data(), W);
        };
        double total = 0.0;
        for (int64_t x0 = 0; x0 < nt; x0 += W) {
          chunk(x0);
          total = biased_add(total, x[W - 1]);
        }
        for (int64_t p = 0; p < cnt; ++p) {
          const double target = biased_target(rw_draw(key, static_cast<uint64_t>(p)), total);
          int64_t found = -1, last = -1;
          double carry = 0.0;
          for (int64_t x0 = 0; x0 < nt && found < 0; x0 += W) {
            chunk(x0);
            for (int l = 0; l < W; ++l) {
              if (w[l] > 0.0 && found < 0 && biased_add(carry, x[l]) > target) found = x0 + l;
              if (w[l] > 0.0) last = x0 + l;
            }
            carry = biased_add(carry, x[W - 1]);
          }
          if (found < 0) found = last;
          if (found >= 0) emit(slot + p, start + found);
        }
      }
    }
  }
  o.indptr[n] = static_cast<Idx>(at);
  return 0;
}

template <typename Idx, typename P, int W>
void launch_etype(const TypedCsr<Idx>& g, const int64_t* off, const int64_t* fan, int64_t T, const P* const* prob,
                  const SeedCsrOut<Idx>& o, int64_t n, int replace, uint64_t rng_seed, int64_t* picks, int64_t cap, bool pick,
                  hipStream_t s) {
  const size_t lds = sizeof(int64_t) * static_cast<size_t>(2 * T + 1);
  const dim3 grid(grid1(pick ? n : n + 1, kEtypeBlock / W)), block(kEtypeBlock);
  if (pick)
    hipLaunchKernelGGL((etype_kernel<Idx, P, W, true>), grid, block, lds, s, g.indptr, g.indices, g.data, off, fan, prob, o.seeds, n,
                       g.num_rows, g.nnz, T, replace, rng_seed, picks, o.indptr, o.nbr, o.eids, cap);
  else
    hipLaunchKernelGGL((etype_kernel<Idx, P, W, false>), grid, block, lds, s, g.indptr, g.indices, g.data, off, fan, prob, o.seeds, n,
                       g.num_rows, g.nnz, T, replace, rng_seed, picks, o.indptr, o.nbr, o.eids, cap);
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_sample_etype_neighbors_workspace_bytes(int idtype_bits, int64_t num_seeds) {
  if (!idbits_ok(idtype_bits) || num_seeds <= 0) return 0;
  return etype_layout(num_seeds).bytes;
}

int dgla_sample_etype_neighbors(const dgla_csr* csr, const int64_t* etype_offset, const int64_t* fanout, int64_t num_etypes,
                                const void* const* prob, int prob_dtype, const void* seeds, int64_t num_seeds, int replace,
                                uint64_t rng_seed, void* out_indptr, void* out_nbr, void* out_eids, int64_t out_capacity,
                                void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "sample_etype_neighbors";
  if (check_etype(who, csr, etype_offset, fanout, num_etypes, prob, prob_dtype, seeds, num_seeds, out_indptr, out_nbr, out_eids,
                  out_capacity))
    return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_indptr);
  const int64_t n = num_seeds, T = num_etypes;
  if (n == 0) {  // (out_indptr[0] = 0, in either id width)
    hipLaunchKernelGGL(etype_zero_kernel, dim3(1), dim3(64), 0, s, static_cast<int*>(out_indptr), csr->idtype_bits / 32);
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const EtypeLayout L = etype_layout(n);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  int64_t* picks = reinterpret_cast<int64_t*>(scratch.p + L.head.picks);
  const int rc = with_idx(csr->idtype_bits, [&](auto id) -> int {
    using Idx = decltype(id);
    return with_prob(prob, prob_dtype, [&](auto pt) -> int {
      using P = decltype(pt);
      const TypedCsr<Idx> g(csr);
      const P* const* pp = reinterpret_cast<const P* const*>(prob);
      const SeedCsrOut<Idx> o(seeds, out_indptr, out_nbr, out_eids);
      auto pass = [&](bool pick) {
        if (etype_width(T) == 16)
          launch_etype<Idx, P, 16>(g, etype_offset, fanout, T, pp, o, n, replace, rng_seed, picks, out_capacity, pick, s);
        else
          launch_etype<Idx, P, 64>(g, etype_offset, fanout, T, pp, o, n, replace, rng_seed, picks, out_capacity, pick, s);
      };
      pass(false);
      if (msd::exclusive_scan<int64_t, Idx>(picks, o.indptr, n + 1, scratch.p + L.head.scan, s)) return -1;
      if (o.nbr && out_capacity > 0) pass(true);
      return 0;
    });
  });
  if (rc) return -1;
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_sample_etype_neighbors_host(const dgla_csr* csr, const int64_t* etype_offset, const int64_t* fanout, int64_t num_etypes,
                                     const void* const* prob, int prob_dtype, const void* seeds, int64_t num_seeds, int replace,
                                     uint64_t rng_seed, void* out_indptr, void* out_nbr, void* out_eids, int64_t out_capacity) {
  const char* who = "sample_etype_neighbors_host";
  if (check_etype(who, csr, etype_offset, fanout, num_etypes, prob, prob_dtype, seeds, num_seeds, out_indptr, out_nbr, out_eids,
                  out_capacity))
    return -1;
  for (int64_t t = 0; t < num_etypes; ++t)
    if (etype_offset[0] != 0 || etype_offset[t + 1] < etype_offset[t]) return fail(who, "etype_offset must be non-decreasing and start at 0");
  return with_idx(csr->idtype_bits, [&](auto id) -> int {
    using Idx = decltype(id);
    return with_prob(prob, prob_dtype, [&](auto pt) -> int {
      using P = decltype(pt);
      return sample_etype_host<Idx, P>(who, TypedCsr<Idx>(csr), etype_offset, fanout, num_etypes,
                                       reinterpret_cast<const P* const*>(prob),
                                       SeedCsrOut<Idx>(seeds, out_indptr, out_nbr, out_eids), num_seeds, replace != 0, rng_seed,
                                       out_capacity);
    });
  });
}

}  // extern "C"
