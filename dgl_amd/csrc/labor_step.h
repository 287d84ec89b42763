// The rule of dgl_amd.sampling.sample_labors (include/dgl_amd.h, "Layer-neighbour sampling"): ONE definition, compiled
// for the device (csrc/labor.hip) and for the host (dgla_labor_scale_host, dgla_labor_pick_host), so the two cannot
// drift.  The generator and the draws are those of csrc/random_walk_step.h, included below and used unchanged.
// LABOR-0 of Balin and Catalyurek, "Layer-Neighbor Sampling -- Defusing Neighborhood Explosion in GNNs"
// (arXiv:2210.13339): one random variate per SOURCE NODE instead of one per edge.
//
// Setting.  One relation as a CSR whose rows are the seed side (the in-edge CSR for edge_dir = "in", the out-edge CSR
// for "out"): indptr, indices (neighbour ids), data (the edge-id map or NULL).  Parameters: seeds[n], a fanout k (an
// int >= 0, or negative for "all"), a 64-bit seed and optionally prob, indexed by EDGE ID (fp32 or fp64).  A seed
// outside [0, num_rows) is a row of degree 0 and touches no memory through that id.
//
// Variate.  r(t) = rw_draw(rw_step_key(rw_walk_key(seed, t), 0), 0) for neighbour node id t: a function of (seed, t)
// only.  The seed row, the relation, the layer and the position in `seeds` do not enter it, so every seed of a call
// (and every relation and layer that is given the same seed) sees the same variate for a shared neighbour.
//
// Uniform rule (no prob).  Row i with lo = indptr[seeds[i]], hi = indptr[seeds[i] + 1], d = hi - lo.  If k < 0 or
// d <= k every position is kept.  Otherwise position q is kept iff rw_index(r(indices[q]), d) < k (the multiply-high of
// the generator: integers only; the inclusion probability is k / d to within 2^-64).
//
// Weighted rule.  w'(q) = rw_weight(prob[data ? data[q] : q]) (negative and NaN weights count as 0).  P = the number of
// positions of the row with w' > 0, W = their sum.  With the row's scale c_i (below), p(q) = min(1, c_i * w'(q)), ONE
// fp64 multiply, and q is kept iff c_i > 0, w'(q) > 0 and rw_uniform(r(indices[q])) < p(q).  The scale also carries
// the two special rows, so that the pick needs nothing but c_i:
//   W not finite (an infinite weight, or a sum that overflows)  ->  c_i = 0:     p = 0, nothing is kept;
//   else k < 0 or P <= k                                        ->  c_i = +inf:  p = 1 exactly where w' > 0;
//   else                                                        ->  c_i finite, by the iteration below.
//
// Scale.  c_i solves sum_q min(1, c * w'(q)) = k (the paper's definition: the expected number of kept edges is k), by
// the finite saturation iteration:  c <- k / W;  repeat  m = #{q: c * w'(q) >= 1},  U = sum of w'(q) over c * w'(q) < 1
// (w' > 0),  and, when m differs from the m of the pass before (0 before the first),  c <- (k - m) / U;  stop when m no
// longer changes.  c only rises and m < k holds throughout (sum min(1, c w') <= k is kept by every update, and P > k).
// The passes are bounded by kLaborMaxPasses = 64; when the bound is reached the current c is used.  (A pass whose
// rounding gives m >= k or U <= 0 also stops with the current c.)  THE LAW STAYS EXACT FOR ANY c: the importances below
// use the actual p, so a c that is off changes only the expected count, never the unbiasedness (node2vec's bounded step
// makes the same kind of statement).  The order of the additions in W and U is free, so the scale is a SEPARATE STEP
// with its own output double c[n]; device and host scales agree to rounding, not bit for bit, and the pick takes c as
// an input.
//
// Importances (weighted form only; the reference returns an empty tensor for unweighted LABOR-0).  For a kept q,
// a(q) = w'(q) / p(q).  The output is a(q) * (n_i / S_i) stored in prob's dtype, with n_i the row's kept count and S_i
// the sum of a over the row's kept positions, so a row's importances sum to n_i and fn.mean over the block stays an
// unbiased estimate.  fp64 throughout.  So that S_i has ONE value, its order of additions is part of the rule: a kept
// position q belongs to class (q - lo) mod 64; each class is summed in ascending q starting from 0.0; the 64 class sums
// are combined by the tree  for s = 32, 16, 8, 4, 2, 1: acc[j] += acc[j + s] for j < s;  S_i = acc[0].  (A group of G
// lanes owns the classes lane, lane + G, ... and finishes with an xor butterfly; fp64 addition commutes, so every
// lane ends with the bits of acc[0].)
//
// Order.  Output goes seed by seed in the given order and, within a seed, in ascending CSR position.  For every kept
// edge: the neighbour id indices[q], the edge id (data[q], or q) and, weighted, the importance.
//
// What follows from the rule.  The result is a pure function of (graph, seeds, k, seed, prob, c), whatever the launch
// geometry.  A neighbour shared by two seeds of equal degree is kept by both or by neither; uniform, a neighbour kept by
// a seed of degree d is kept by every seed of degree <= d that has it; the picks for k are a subset of the picks for
// k' > k; a duplicated neighbour of a multigraph row is kept or dropped with all its copies; the order of `seeds`
// permutes the output rows and changes nothing else.
//
// Integer arithmetic, one fp64 multiply, fp64 compares and, for the importances, IEEE fp64 divisions and additions in a
// fixed order: pick on the device and pick on the host agree bit for bit from the same c.  No expression here has the
// shape a * b + c, so no contraction into a fused multiply-add can separate the two compilations.
#pragma once
#include "random_walk_step.h"

namespace dgla {

constexpr int kLaborMaxPasses = 64;  // passes of the saturation iteration
constexpr int kLaborClasses = 64;    // classes of the importance sum S_i

DGLA_RW_HD uint64_t labor_variate(uint64_t seed, int64_t t) {
  return rw_draw(rw_step_key(rw_walk_key(seed, static_cast<uint64_t>(t)), 0), 0);
}

// uniform rule, for a row of degree d > k >= 0
DGLA_RW_HD bool labor_keep_uniform(uint64_t seed, int64_t t, int64_t d, int64_t k) {
  return rw_index(labor_variate(seed, t), static_cast<uint64_t>(d)) < static_cast<uint64_t>(k);
}

// weighted rule for one position of weight w = w'(q) under the row's scale c; *a = w / p when kept
DGLA_RW_HD bool labor_keep_weighted(uint64_t seed, int64_t t, double c, double w, double* a) {
  if (!(w > 0.0) || !(c > 0.0)) return false;  // (c = 0 with an infinite weight: 0 * inf is NaN, not 0)
  const double cw = c * w;
  const double p = cw < 1.0 ? cw : 1.0;
  if (!(rw_uniform(labor_variate(seed, t)) < p)) return false;
  *a = w / p;
  return true;
}

// what a saturation pass contributes for one position: saturated (c * w >= 1) or its weight to U
DGLA_RW_HD bool labor_saturated(double c, double w) { return c * w >= 1.0; }

// The scale's decisions, given a way to sweep the row.  first(&P, &W): the number and the sum of the positive weights;
// pass(c, &m, &U): one saturation pass.  Device (a group of lanes per row) and host (a loop) hand in their own sweeps;
// every lane of a group gets the same P, W, m, U, so the control flow below is uniform over the group.
template <typename First, typename Pass>
DGLA_RW_HD double labor_scale_row(int64_t k, First first, Pass pass) {
  int64_t P;
  double W;
  first(&P, &W);
  if (!(W <= 1.7976931348623157e308)) return 0.0;                     // not finite: nothing is kept
  if (k < 0 || P <= k) return __builtin_huge_val();                   // every positive weight, p = 1
  double c = static_cast<double>(k) / W;
  int64_t m_prev = 0;
  for (int it = 0; it < kLaborMaxPasses; ++it) {
    int64_t m;
    double U;
    pass(c, &m, &U);
    if (m == m_prev || m >= k || !(U > 0.0)) break;
    c = static_cast<double>(k - m) / U;
    m_prev = m;
  }
  return c;
}

// the tree of the importance sum over the 64 class sums (host form; the device finishes with a butterfly)
inline double labor_class_tree(double* acc) {
  for (int s = kLaborClasses / 2; s >= 1; s >>= 1)
    for (int j = 0; j < s; ++j) acc[j] += acc[j + s];
  return acc[0];
}

// the factor of a row's importances
DGLA_RW_HD double labor_importance_factor(int64_t n_kept, double S) { return static_cast<double>(n_kept) / S; }

}  // namespace dgla
