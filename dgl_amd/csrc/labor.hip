// Layer-neighbour (LABOR-0) sampling on the device: dgl.sampling.sample_labors, dgl.dataloading.LaborSampler.
//
// Reference: CSRLaborSampling<kDGLCUDA> (src/array/cuda/labor_sampling.cu over src/array/labor_pick.h): a chain of
// cub / thrust passes (degrees, a segmented sort or reduce for the per-row scale, a Philox draw per (seed, neighbour)
// hashed from the neighbour id, DeviceSelect for the compaction) through temporaries of nnz-of-the-seeds size.
//
// MI355X-first choices:
//  * The rule is the one of csrc/labor_step.h, compiled here for the kernels and for dgla_labor_scale_host /
//    dgla_labor_pick_host: a counter-based variate keyed by (seed, neighbour id), three mix64 in registers, no state
//    and no table.  The result is a pure function of its arguments, whatever the launch geometry.
//  * LABOR reads EVERY neighbour of every seed (sample_pick_kernel reads O(fanout) per seed), so the hot path is a row
//    stream: a GROUP of G lanes strides one row with coalesced loads, the keep flags of a step come from one __ballot
//    (64 bits), and a kept entry goes to (row start) + (kept so far) + popcount(the group's lower lanes): CSR order is
//    preserved without atomics and without a sort.
//  * G is 16 or 64, chosen per call from the relation's mean degree (nnz / num_rows <= 32 -> 16): a wavefront then
//    serves four short rows at once instead of idling 3/4 of its lanes, and a hub row is still streamed 64 ids at a
//    time.  Both widths write the same bits (the sum order of the importances is part of the rule, labor_step.h).
//  * count and fill both evaluate the rule.  A keep bitmask written by count would save fill nothing but ALU: fill
//    must read the ids (and the weights) of the kept entries anyway, and at k / d >= 1 / 16 nearly every 64-byte line
//    of a row holds one.  Bytes per call: 2 * (sum of deg(seed)) ids, the second read of a row served by L2 / the
//    Infinity Cache when the rows of a call fit there, plus one gathered weight per neighbour and
//    pass when weighted, plus the outputs.  (A bitmask would also need a workspace sized by the seeds' degrees, which
//    the host does not know before count has run; what it would save on long rows is in DESIGN.md 3.15, "Measured".)
//  * The per-row importance sum S is computed by count (which has every a(q) in registers) and handed to fill through
//    the workspace: 8 bytes per seed instead of a second sweep of the row inside fill.
//  * No atomics anywhere; the offsets come from the library's scan (csrc/sort.hip.h).
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>
#include <vector>

#include "host_util.h"
#include "labor_step.h"
#include "sort.hip.h"

namespace dgla {
namespace {

constexpr int kLaborBlock = 256;        // threads per workgroup: 256 / G rows
constexpr int64_t kLaborShortMean = 32; // mean degree up to which a row gets 16 lanes

int labor_group(const dgla_csr* c) {
  const int64_t rows = c->num_rows > 0 ? c->num_rows : 1;
  return c->nnz / rows <= kLaborShortMean ? 16 : 64;
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

template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {  // xor butterfly: every lane of the group ends with the same bits
#pragma unroll
  for (int s = G / 2; s >= 1; s >>= 1) v += __shfl_xor(v, s, G);
  return v;
}

// [lo, hi) of seed row `row`; a seed outside [0, num_rows) is an empty row and touches no memory
template <typename Idx>
__device__ __forceinline__ void seed_row(gptr<Idx> indptr, const Idx* __restrict__ seeds, int64_t num_rows, int64_t row,
                                         int64_t* lo, int64_t* hi) {
  const int64_t s = static_cast<int64_t>(seeds[row]);
  *lo = *hi = 0;
  if (s >= 0 && s < num_rows) {
    *lo = static_cast<int64_t>(indptr[s]);
    *hi = static_cast<int64_t>(indptr[s + 1]);
  }
}

template <typename Idx, typename W>
__device__ __forceinline__ double weight_at(gptr<Idx> data, gptr<W> prob, int64_t q) {
  return rw_weight(prob[data ? static_cast<int64_t>(data[q]) : q]);
}

// One sweep of row [lo, hi) by a group of G lanes (lg = lane in the group, lane = lane in the wavefront): 64 positions
// per outer step in 64 / G sub-steps, so lane lg owns the classes lg, lg + G, ... of the importance sum.  Returns the
// kept count (the same in every lane of the group).  !FILL: *S = the row's importance sum (weighted).  FILL: kept
// entries go to out_base + their rank; `cap` bounds every write.
template <typename Idx, typename W, bool WEIGHTED, int G, bool FILL>
__device__ __forceinline__ int64_t labor_sweep(gptr<Idx> indices, gptr<Idx> data, gptr<W> prob, int64_t lo, int64_t hi,
                                               bool all, int64_t k, uint64_t seed, double c, int lg, int lane, double* S,
                                               Idx* __restrict__ out_nbr, Idx* __restrict__ out_eid,
                                               W* __restrict__ out_imp, int64_t out_base, int64_t cap, double factor) {
  constexpr int R = 64 / G;
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  int64_t run = 0;
  const int64_t d = hi - lo;
  for (int64_t base = lo; base < hi; base += 64) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (base + r * G >= hi) break;  // (the same for every lane of the group)
      const int64_t q = base + r * G + lg;
      bool keep = false;
      Idx t = 0;
      double a = 0.0;
      if (q < hi) {
        t = indices[q];
        if constexpr (WEIGHTED) {
          keep = labor_keep_weighted(seed, static_cast<int64_t>(t), c, weight_at<Idx, W>(data, prob, q), &a);
        } else {
          keep = all || labor_keep_uniform(seed, static_cast<int64_t>(t), d, k);
        }
      }
      const uint64_t sub = group_bits<G>(__ballot(keep), lane);
      if (keep) {
        if constexpr (WEIGHTED && !FILL) acc[r] += a;
        if constexpr (FILL) {
          const int64_t pos = out_base + run + __popcll(sub & ((uint64_t(1) << lg) - 1));
          if (pos < cap) {
            out_nbr[pos] = t;
            out_eid[pos] = data ? data[q] : static_cast<Idx>(q);
            if constexpr (WEIGHTED) out_imp[pos] = static_cast<W>(a * factor);
          }
        }
      }
      run += __popcll(sub);
    }
  }
  if constexpr (WEIGHTED && !FILL) {
#pragma unroll
    for (int s = R / 2; s >= 1; s >>= 1)  // classes j and j + s * G of this lane: the tree's strides 32 .. G
#pragma unroll
      for (int r = 0; r < s; ++r) acc[r] += acc[r + s];
    *S = group_sum<G>(acc[0]);            // strides G / 2 .. 1
  }
  return run;
}

// ---- count ------------------------------------------------------------------------------------------
// cnt[row] = kept entries of seed row `row` (int64; cnt[n] = 0 closes the scan), S[row] = its importance sum
template <typename Idx, typename W, bool WEIGHTED, int G>
__global__ __launch_bounds__(kLaborBlock) void labor_count_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                  const Idx* __restrict__ data, const W* __restrict__ prob,
                                                                  const double* __restrict__ cs, const Idx* __restrict__ seeds,
                                                                  int64_t n, int64_t num_rows, int64_t k, uint64_t seed,
                                                                  int64_t* __restrict__ cnt, double* __restrict__ S) {
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t row = blockIdx.x * static_cast<int64_t>(kLaborBlock / G) + threadIdx.x / G;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n] = 0;
  if (row >= n) return;  // (whole groups leave)
  int64_t lo, hi;
  seed_row((gptr<Idx>)indptr, seeds, num_rows, row, &lo, &hi);
  const bool all = !WEIGHTED && (k < 0 || hi - lo <= k);
  int64_t kept;
  double sum = 0.0;
  if (all) {
    kept = hi - lo;
  } else {
    kept = labor_sweep<Idx, W, WEIGHTED, G, false>((gptr<Idx>)indices, (gptr<Idx>)data, (gptr<W>)prob, lo, hi, false, k, seed,
                                                   WEIGHTED ? cs[row] : 0.0, lg, lane, &sum, nullptr, nullptr, nullptr, 0,
                                                   0, 0.0);
  }
  if (lg == 0) {
    cnt[row] = kept;
    if (WEIGHTED) S[row] = sum;
  }
}

// out_indptr = the scanned offsets in the id type, *total = their last entry
template <typename Idx>
__global__ __launch_bounds__(kLaborBlock) void labor_indptr_kernel(const int64_t* __restrict__ offs, int64_t n,
                                                                   Idx* __restrict__ out_indptr, int64_t* __restrict__ total) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kLaborBlock) + threadIdx.x;
  if (i <= n) out_indptr[i] = static_cast<Idx>(offs ? offs[i] : 0);
  if (i == 0) *total = offs ? offs[n] : 0;
}

// ---- fill -------------------------------------------------------------------------------------------
template <typename Idx, typename W, bool WEIGHTED, int G>
__global__ __launch_bounds__(kLaborBlock) void labor_fill_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                                 const Idx* __restrict__ data, const W* __restrict__ prob,
                                                                 const double* __restrict__ cs, const Idx* __restrict__ seeds,
                                                                 int64_t n, int64_t num_rows, int64_t k, uint64_t seed,
                                                                 const int64_t* __restrict__ offs, const double* __restrict__ S,
                                                                 Idx* __restrict__ out_nbr, Idx* __restrict__ out_eid,
                                                                 W* __restrict__ out_imp, int64_t cap) {
  const int lane = threadIdx.x & 63, lg = threadIdx.x & (G - 1);
  const int64_t row = blockIdx.x * static_cast<int64_t>(kLaborBlock / G) + threadIdx.x / G;
  if (row >= n) return;
  const int64_t at = offs[row], kept = offs[row + 1] - at;
  if (kept <= 0) return;
  int64_t lo, hi;
  seed_row((gptr<Idx>)indptr, seeds, num_rows, row, &lo, &hi);
  const bool all = !WEIGHTED && (k < 0 || hi - lo <= k);
  const double factor = WEIGHTED ? labor_importance_factor(kept, S[row]) : 0.0;
  (void)labor_sweep<Idx, W, WEIGHTED, G, true>((gptr<Idx>)indices, (gptr<Idx>)data, (gptr<W>)prob, lo, hi, all, k, seed,
                                               WEIGHTED ? cs[row] : 0.0, lg, lane, nullptr, out_nbr, out_eid, out_imp, at,
                                               cap, factor);
}

// ---- scale ------------------------------------------------------------------------------------------
template <typename Idx, typename W, int G>
__global__ __launch_bounds__(kLaborBlock) void labor_scale_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ data,
                                                                  const W* __restrict__ prob, const Idx* __restrict__ seeds,
                                                                  int64_t n, int64_t num_rows, int64_t k,
                                                                  double* __restrict__ cs) {
  const int lg = threadIdx.x & (G - 1);
  const int64_t row = blockIdx.x * static_cast<int64_t>(kLaborBlock / G) + threadIdx.x / G;
  if (row >= n) return;
  int64_t lo, hi;
  seed_row((gptr<Idx>)indptr, seeds, num_rows, row, &lo, &hi);
  gptr<Idx> dat = (gptr<Idx>)data;
  gptr<W> pr = (gptr<W>)prob;
  const double c = labor_scale_row(
      k,
      [&](int64_t* P, double* Wsum) {
        long long p = 0;
        double w = 0.0;
        for (int64_t q = lo + lg; q < hi; q += G) {
          const double x = weight_at<Idx, W>(dat, pr, q);
          if (x > 0.0) ++p, w += x;
        }
        *P = group_sum<G>(p);
        *Wsum = group_sum<G>(w);
      },
      [&](double cc, int64_t* m, double* U) {
        long long sat = 0;
        double u = 0.0;
        for (int64_t q = lo + lg; q < hi; q += G) {
          const double x = weight_at<Idx, W>(dat, pr, q);
          if (x > 0.0) {
            if (labor_saturated(cc, x)) ++sat; else u += x;
          }
        }
        *m = group_sum<G>(sat);
        *U = group_sum<G>(u);
      });
  if (lg == 0) cs[row] = c;
}

// ---- host side --------------------------------------------------------------------------------------
struct LaborLayout {  // offsets into the workspace shared by dgla_labor_count and dgla_labor_fill
  size_t offs, S, scan, bytes;
};

LaborLayout labor_layout(int64_t n) {
  LaborLayout L{};
  Carver c;
  L.offs = c.take(sizeof(int64_t) * static_cast<size_t>(n + 1));
  L.S = c.take(sizeof(double) * static_cast<size_t>(n));
  L.scan = c.take(msd::scan_temp_bytes(n + 1, sizeof(int64_t)));
  L.bytes = c.bytes();
  return L;
}

// everything the entry points refuse; `weighted_only`: the scale has no uniform form
int check_labor(const char* who, const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, bool need_c,
                const void* seeds, int64_t n, bool weighted_only) {
  if (check_csr(who, csr, kCsrCols | kCsrEmptyIndptr)) return -1;
  if (n < 0) return fail(who, "negative size");
  if (n >= (int64_t(1) << 31)) return fail(who, "num_seeds must be below 2^31, got " + std::to_string(n));
  if (n > 0 && !seeds) return fail(who, "seeds is null");
  if (weighted_only && !prob) return fail(who, "prob is null (the scale belongs to the weighted form)");
  if (prob && prob_dtype != kF32 && prob_dtype != kF64) return fail(who, "prob must be float32 or float64");
  if (prob && need_c && n > 0 && !c) return fail(who, "c is null (dgla_labor_scale writes it)");
  return 0;
}

// f(integral_constant<int, G>): the group width of a call
template <typename F>
decltype(auto) with_group(const dgla_csr* csr, F&& f) {
  if (labor_group(csr) == 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 64>{});
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename Idx>
void host_row(const TypedCsr<Idx>& g, const Idx* seeds, int64_t i, int64_t* lo, int64_t* hi) {
  const int64_t s = static_cast<int64_t>(seeds[i]);
  *lo = *hi = 0;
  if (s >= 0 && s < g.num_rows) *lo = static_cast<int64_t>(g.indptr[s]), *hi = static_cast<int64_t>(g.indptr[s + 1]);
}

template <typename Idx, typename W>
void scale_host(const TypedCsr<Idx>& g, const W* prob, const Idx* seeds, int64_t n, int64_t k, double* cs) {
  const Idx* data = g.data;
  for (int64_t i = 0; i < n; ++i) {
    int64_t lo, hi;
    host_row(g, seeds, i, &lo, &hi);
    auto weight = [&](int64_t q) { return rw_weight(prob[data ? static_cast<int64_t>(data[q]) : q]); };
    cs[i] = labor_scale_row(
        k,
        [&](int64_t* P, double* Wsum) {
          *P = 0, *Wsum = 0.0;
          for (int64_t q = lo; q < hi; ++q) {
            const double x = weight(q);
            if (x > 0.0) ++*P, *Wsum += x;
          }
        },
        [&](double c, int64_t* m, double* U) {
          *m = 0, *U = 0.0;
          for (int64_t q = lo; q < hi; ++q) {
            const double x = weight(q);
            if (x > 0.0) {
              if (labor_saturated(c, x)) ++*m; else *U += x;
            }
          }
        });
  }
}

// out_nbr == NULL: out_indptr only (the sizes)
template <typename Idx, typename W, bool WEIGHTED>
void pick_host(const TypedCsr<Idx>& g, const W* prob, const double* cs, const Idx* seeds, int64_t n, int64_t k, uint64_t seed,
               Idx* out_indptr, Idx* out_nbr, Idx* out_eid, W* out_imp) {
  const Idx *indices = g.indices, *data = g.data;
  int64_t at = 0;
  std::vector<double> as;
  for (int64_t i = 0; i < n; ++i) {
    out_indptr[i] = static_cast<Idx>(at);
    int64_t lo, hi;
    host_row(g, seeds, i, &lo, &hi);
    const int64_t d = hi - lo;
    const bool all = !WEIGHTED && (k < 0 || d <= k);
    double acc[kLaborClasses] = {};
    as.clear();
    const int64_t start = at;
    for (int64_t q = lo; q < hi; ++q) {
      const int64_t t = static_cast<int64_t>(indices[q]);
      double a = 0.0;
      bool keep;
      if (WEIGHTED)
        keep = labor_keep_weighted(seed, t, cs[i], rw_weight(prob[data ? static_cast<int64_t>(data[q]) : q]), &a);
      else
        keep = all || labor_keep_uniform(seed, t, d, k);
      if (!keep) continue;
      if (out_nbr) {
        out_nbr[at] = indices[q];
        out_eid[at] = data ? data[q] : static_cast<Idx>(q);
      }
      if (WEIGHTED) acc[(q - lo) % kLaborClasses] += a, as.push_back(a);
      ++at;
    }
    if (WEIGHTED && out_nbr && out_imp && at > start) {
      const double factor = labor_importance_factor(at - start, labor_class_tree(acc));
      for (int64_t j = start; j < at; ++j) out_imp[j] = static_cast<W>(as[j - start] * factor);
    }
  }
  out_indptr[n] = static_cast<Idx>(at);
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_labor_workspace_bytes(int idtype_bits, int64_t num_seeds) {
  if (!idbits_ok(idtype_bits) || num_seeds <= 0 || num_seeds >= (int64_t(1) << 31)) return 0;
  return labor_layout(num_seeds).bytes;
}

int dgla_labor_scale(const dgla_csr* csr, const void* prob, int prob_dtype, const void* seeds, int64_t num_seeds,
                     int64_t fanout, double* c, void* hip_stream) {
  if (check_labor("labor_scale", csr, prob, prob_dtype, c, true, seeds, num_seeds, true)) return -1;
  if (num_seeds == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, c);
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    with_weight(prob, prob_dtype, [&](auto wtag, auto) {
      using W = decltype(wtag);
      with_group(csr, [&](auto grp) {
        constexpr int G = decltype(grp)::value;
        hipLaunchKernelGGL((labor_scale_kernel<Idx, W, G>), dim3(grid1(num_seeds, kLaborBlock / G)), dim3(kLaborBlock), 0, s,
                           g.indptr, g.data, static_cast<const W*>(prob), static_cast<const Idx*>(seeds), num_seeds, g.num_rows,
                           fanout, c);
      });
    });
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_labor_count(const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, const void* seeds,
                     int64_t num_seeds, int64_t fanout, uint64_t seed, void* out_indptr, int64_t* total, void* workspace,
                     size_t workspace_bytes, void* hip_stream) {
  const char* who = "labor_count";
  if (check_labor(who, csr, prob, prob_dtype, c, true, seeds, num_seeds, false)) return -1;
  if (!out_indptr || !total) return fail(who, "out_indptr / total are null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int64_t n = num_seeds;
  const bool rows = n > 0 && csr->nnz > 0;  // otherwise every row is empty: no graph memory is read
  LaborLayout L{};
  if (rows) {
    L = labor_layout(n);
    if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  }
  const DeviceGuard dev(s, total);
  char* ws = static_cast<char*>(workspace);
  int64_t* offs = rows ? reinterpret_cast<int64_t*>(ws + L.offs) : nullptr;
  if (rows) {
    double* S = reinterpret_cast<double*>(ws + L.S);
    with_idx(csr->idtype_bits, [&](auto tag) {
      using Idx = decltype(tag);
      const TypedCsr<Idx> g(csr);
      with_weight(prob, prob_dtype, [&](auto wtag, auto weighted) {
        using W = decltype(wtag);
        constexpr bool WEIGHTED = decltype(weighted)::value;
        with_group(csr, [&](auto grp) {
          constexpr int G = decltype(grp)::value;
          hipLaunchKernelGGL((labor_count_kernel<Idx, W, WEIGHTED, G>), dim3(grid1(n, kLaborBlock / G)), dim3(kLaborBlock), 0,
                             s, g.indptr, g.indices, g.data, static_cast<const W*>(prob), c, static_cast<const Idx*>(seeds), n,
                             g.num_rows, fanout, seed, offs, S);
        });
      });
    });
    DGLA_CHECK_HIP(hipGetLastError());
    if (msd::exclusive_scan<int64_t, int64_t>(offs, offs, n + 1, ws + L.scan, s)) return -1;
  }
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    hipLaunchKernelGGL(labor_indptr_kernel<Idx>, dim3(grid1(n + 1, kLaborBlock)), dim3(kLaborBlock), 0, s, offs, n,
                       static_cast<Idx*>(out_indptr), total);
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_labor_fill(const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, const void* seeds,
                    int64_t num_seeds, int64_t fanout, uint64_t seed, int64_t capacity, void* out_nbr, void* out_eid,
                    void* out_imp, const void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "labor_fill";
  if (check_labor(who, csr, prob, prob_dtype, c, true, seeds, num_seeds, false)) return -1;
  if (capacity < 0) return fail(who, "negative capacity");
  if (num_seeds == 0 || csr->nnz == 0 || capacity == 0) return 0;  // nothing was counted
  if (!out_nbr || !out_eid || (prob && !out_imp)) return fail(who, "out_nbr / out_eid / out_imp are null");
  const int64_t n = num_seeds;
  const LaborLayout L = labor_layout(n);
  if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;  // (the workspace labor_count filled)
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_nbr);
  const char* ws = static_cast<const char*>(workspace);
  const int64_t* offs = reinterpret_cast<const int64_t*>(ws + L.offs);
  const double* S = reinterpret_cast<const double*>(ws + L.S);
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    with_weight(prob, prob_dtype, [&](auto wtag, auto weighted) {
      using W = decltype(wtag);
      constexpr bool WEIGHTED = decltype(weighted)::value;
      with_group(csr, [&](auto grp) {
        constexpr int G = decltype(grp)::value;
        hipLaunchKernelGGL((labor_fill_kernel<Idx, W, WEIGHTED, G>), dim3(grid1(n, kLaborBlock / G)), dim3(kLaborBlock), 0, s,
                           g.indptr, g.indices, g.data, static_cast<const W*>(prob), c, static_cast<const Idx*>(seeds), n,
                           g.num_rows, fanout, seed, offs, S, static_cast<Idx*>(out_nbr), static_cast<Idx*>(out_eid),
                           static_cast<W*>(out_imp), capacity);
      });
    });
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_labor_scale_host(const dgla_csr* csr, const void* prob, int prob_dtype, const void* seeds, int64_t num_seeds,
                          int64_t fanout, double* c) {
  if (check_labor("labor_scale_host", csr, prob, prob_dtype, c, true, seeds, num_seeds, true)) return -1;
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    with_weight(prob, prob_dtype, [&](auto wtag, auto) {
      using W = decltype(wtag);
      scale_host<Idx, W>(TypedCsr<Idx>(csr), static_cast<const W*>(prob), static_cast<const Idx*>(seeds), num_seeds, fanout, c);
    });
  });
  return 0;
}

int dgla_labor_pick_host(const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, const void* seeds,
                         int64_t num_seeds, int64_t fanout, uint64_t seed, void* out_indptr, void* out_nbr, void* out_eid,
                         void* out_imp) {
  const char* who = "labor_pick_host";
  if (check_labor(who, csr, prob, prob_dtype, c, true, seeds, num_seeds, false)) return -1;
  if (!out_indptr) return fail(who, "out_indptr is null");
  if (out_nbr && !out_eid) return fail(who, "out_eid is null");
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    with_weight(prob, prob_dtype, [&](auto wtag, auto weighted) {
      using W = decltype(wtag);
      pick_host<Idx, W, decltype(weighted)::value>(TypedCsr<Idx>(csr), static_cast<const W*>(prob), c,
                                                   static_cast<const Idx*>(seeds), num_seeds, fanout, seed, static_cast<Idx*>(out_indptr),
                                                   static_cast<Idx*>(out_nbr), static_cast<Idx*>(out_eid),
                                                   static_cast<W*>(out_imp));
    });
  });
  return 0;
}

}  // extern "C"
