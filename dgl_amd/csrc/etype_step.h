// The rule of per-edge-type neighbour sampling (include/dgl_amd.h, "Per-edge-type neighbour sampling"): ONE definition,
// compiled for the device (csrc/etype.hip) and for the host twin (dgla_sample_etype_neighbors_host), so the two cannot
// drift.
//
// Input.  One CSR of a homogenised graph (indptr, indices, data = the edge-id map or NULL), etype_offset[T + 1] (int64,
// non-decreasing from 0: edge id e has type t iff etype_offset[t] <= e < etype_offset[t + 1]), fanout[T] (int64, negative
// = all), optionally prob[T] (per type a pointer or NULL; prob[t] is indexed by e - etype_offset[t]; fp32, fp64 or uint8,
// one type per call), replace, the seeds and an rng seed.  Every row is taken to be ordered by edge type.
//
// For seed row u with deg entries (row bounds clamped into [0, nnz] as in topk_row):
//  * range of type t: lower(b) = the first row-relative position whose edge id is >= b, by bisection over the row.
//    start_t = lower(etype_offset[t]), end_t = max(start_t, lower(etype_offset[t + 1])), n_t = end_t - start_t.  On a row
//    that is not ordered the picks are unspecified, but every position lies in [0, deg] and no range is negative.
//  * weight of an entry of the range, when prob[t] is given: (double)prob[t][e - etype_offset[t]] when that is a positive
//    finite number, else 0; an entry whose edge id is not of type t (an unordered row) weighs 0 and reads nothing; a mask
//    byte weighs 0 or 1.  P_t = the number of entries with a positive weight (n_t without prob[t]).
//  * picks of (u, t), f = fanout[t]:  f < 0: P_t.  replace: f if P_t > 0, else 0.  Otherwise min(f, P_t).
//  * generator: key = rw_step_key(rw_walk_key(rng seed, u), t) (ROW ID and TYPE, so a seed listed twice draws the same
//    picks, and the picks depend neither on the launch geometry nor on the fan-outs of other types); r(k) = rw_draw(key, k)
//    with k a draw index or a range-relative position.
//  * unweighted: every entry in position order when picks == n_t without replacement; with replacement pick k is
//    start_t + rw_index(r(k), n_t); else Floyd's subset: for m = 0 .. f - 1, j = n_t - f + m, c = rw_index(r(m), j + 1),
//    pick m is j when an earlier pick of the range took c, else c.
//  * weighted: every positive entry in position order when picks == P_t without replacement.  Otherwise, without
//    replacement, the `picks` smallest (key, position) in that order, key(x) = etype_neglog(r(x)) / w(x) (the exponential
//    clock of weighted_pick_kernel; etype_neglog is written out below so that both sides round alike).  With replacement,
//    the weights are summed in chunks of W positions (W = 16 when T <= 16, else 64) by the Hillis-Steele network within a
//    chunk and a carry between chunks (biased_scan_host); target = rw_uniform(r(k)) * total, and the pick is the first
//    position with a positive weight and prefix > target, or (rounding) the last positive one.
//  * output: the picks of a seed follow each other by ascending type, then pick order.  Slots at or beyond the caller's
//    capacity are neither written nor read.
//
// Integer arithmetic and IEEE fp64 add, multiply, divide in a fixed order with contraction off: host == device, bit for
// bit.
#pragma once
#include <stdint.h>

#include "biased_step.h"   // biased_add, biased_target, biased_scan_host; topk_row, topk_eid and the generator

namespace dgla {

constexpr int kEtypeMaxTypes = 1024;   // the largest T: etype_offset and fanout fit in 16 KB of LDS
constexpr int kEtypeU8 = 4;            // the prob dtype code of a bool / uint8 mask (DGLA_ETYPE_U8)
constexpr int kEtypeRegPicks = 32;     // Floyd's positions of a range live in registers up to this fan-out

// the width of the lane group that owns a seed
DGLA_RW_HD int etype_width(int64_t num_types) { return num_types <= 16 ? 16 : 64; }

DGLA_RW_HD uint64_t etype_key(uint64_t rng_seed, int64_t u, int64_t t) {
  return rw_step_key(rw_walk_key(rng_seed, static_cast<uint64_t>(u)), static_cast<uint64_t>(t));
}

// start_t and n_t: the two bisections run side by side, so that their loads are in flight together
template <typename IdxPtr>
DGLA_RW_HD void etype_range(IdxPtr data, int64_t lo, int64_t deg, int64_t b0, int64_t b1, int64_t* start, int64_t* n) {
  int64_t a0 = 0, h0 = deg, a1 = 0, h1 = deg;
  while (a0 < h0 || a1 < h1) {
    if (a0 < h0) {
      const int64_t m = a0 + ((h0 - a0) >> 1);
      if (topk_eid(data, lo + m) >= b0) h0 = m; else a0 = m + 1;
    }
    if (a1 < h1) {
      const int64_t m = a1 + ((h1 - a1) >> 1);
      if (topk_eid(data, lo + m) >= b1) h1 = m; else a1 = m + 1;
    }
  }
  *start = a0;
  *n = a1 > a0 ? a1 - a0 : 0;
}

// the weight of the entry with edge id e in the range of a type with ids [b0, b1)
template <typename P, typename ProbPtr>
DGLA_RW_HD double etype_weight(ProbPtr prob, int64_t e, int64_t b0, int64_t b1) {
  if (e < b0 || e >= b1) return 0.0;
  const double w = static_cast<double>(prob[e - b0]);
  return (w > 0.0 && w <= 1.7976931348623157e308) ? w : 0.0;
}

DGLA_RW_HD int64_t etype_picks(int64_t P, int64_t f, bool replace) {
  if (f < 0) return P;
  if (replace) return P > 0 ? f : 0;
  return f < P ? f : P;
}

// -ln(u) for u = ((r >> 11) + 1) * 2^-53 in (0, 1]: u = m * 2^(e - 53) with m in (sqrt(1/2), sqrt(2)], ln(m) =
// 2 atanh(s), s = (m - 1) / (m + 1), as an odd series in s by Horner's rule.  Plain fp64 operations in a fixed order.
DGLA_RW_HD double etype_neglog(uint64_t r) {
#pragma clang fp contract(off)
  const double k = static_cast<double>((r >> 11) + 1);   // exact: at most 2^53
  uint64_t bits;
  __builtin_memcpy(&bits, &k, 8);
  int64_t e = static_cast<int64_t>((bits >> 52) & 0x7FF) - 1023;
  bits = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
  double m;
  __builtin_memcpy(&m, &bits, 8);
  if (m > 1.4142135623730951) {
    m = m * 0.5;
    e += 1;
  }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 25.0;
  p = p * z + 1.0 / 23.0;
  p = p * z + 1.0 / 21.0;
  p = p * z + 1.0 / 19.0;
  p = p * z + 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  p = p * z + 1.0;
  const double lnm = 2.0 * s * p;
  const double v = static_cast<double>(53 - e) * 0.6931471805599453 - lnm;
  return v > 0.0 ? v : 0.0;
}

// the exponential-clock key of range-relative position x with weight w > 0
DGLA_RW_HD double etype_clock(uint64_t key, int64_t x, double w) {
#pragma clang fp contract(off)
  return etype_neglog(rw_draw(key, static_cast<uint64_t>(x))) / w;
}

// is (ka, xa) before (kb, xb)?
DGLA_RW_HD bool etype_before(double ka, int64_t xa, double kb, int64_t xb) { return ka < kb || (ka == kb && xa < xb); }

// Floyd's draw m of a range of n entries with fan-out f: the candidate and the fall-back
DGLA_RW_HD void etype_floyd(uint64_t key, int64_t n, int64_t f, int64_t m, int64_t* c, int64_t* j) {
  *j = n - f + m;
  *c = static_cast<int64_t>(rw_index(rw_draw(key, static_cast<uint64_t>(m)), static_cast<uint64_t>(*j + 1)));
}

}  // namespace dgla
