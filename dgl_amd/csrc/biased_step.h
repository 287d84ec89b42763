// The rules of the tag sort and of tag-biased neighbour sampling (include/dgl_amd.h, "Tag-biased neighbour sampling"):
// ONE definition, compiled for the device (csrc/biased.hip) and for the host twins (dgla_sort_csr_by_tag_host,
// dgla_sample_neighbors_biased_host), so the two cannot drift.
//
// Tag sort (the rule of CSRSortByTag, src/array/cpu/csr_sort.cc).  Input: one CSR (indptr, indices, data = the edge-id
// map or NULL), tag[nnz] indexed by EDGE ID (int32 or int64) and T = num_tags.  Output: out_indices, out_data (always
// materialised: the edge id, or the old position when data was NULL) and tag_pos[num_rows, T + 1], row-relative offsets.
// Within a row the entries are ordered by tag and, among equal tags, by their original position: a stable counting
// sort, so the result is a function of the inputs.  A tag outside [0, T) and an edge id outside [0, nnz) are reported
// (biased_bad_tag / biased_bad_eid below); row bounds are clamped into [0, nnz] as in topk_row.
//
// Biased picks.  Input: a CSR already sorted by tag, tag_offset[num_rows, T + 1] indexed by NODE ID, bias[T] (fp32 or
// fp64), the seeds, fanout, replace and an rng seed.  For seed row u with deg entries:
//  * range of tag t: start_t = clamp(tag_offset[u][t], 0, deg), end_t = max(start_t, clamp(tag_offset[u][t + 1], 0, deg)),
//    n_t = end_t - start_t: malformed offsets address nothing outside the row and no range is negative.
//  * b_t = (double)bias[t] when that is a positive finite number, else 0 (NaN, negative and infinite biases count as 0).
//  * P = sum of n_t over the tags with b_t > 0.  picks = P for fanout == -1; fanout if P > 0 else 0 with replacement;
//    min(fanout, P) otherwise (GetSamplingBiasedNumPicksFn).
//  * fanout == -1: every entry of the positive-bias ranges, by ascending tag and position.  No draw.
//  * Generator: key = rw_walk_key(rng seed, u) (the ROW ID, so a seed listed twice draws the same picks and the picks
//    do not depend on the launch geometry), step = rw_step_key(key, p) for pick p, slot 0 draws the tag and slot 1 the
//    position.
//  * Tag of pick p: weights w_t = (double)(n_t - taken_t) * b_t (taken_t = 0 with replacement, else the number of earlier
//    picks of the row with tag t).  The tags are scanned in chunks of W lanes (W = 16 when T <= 16, else 64): within a
//    chunk the inclusive sums come from the Hillis-Steele network (for d = 1, 2, .. W/2: x[l] += x[l - d] for l >= d, all
//    lanes at once), prefix_t = carry + x[l], and the carry of the next chunk is carry + x[W - 1].  total = the last
//    carry, target = rw_uniform(r) * total, and the tag is the first t with w_t > 0 and prefix_t > target; when rounding
//    leaves none, the last tag with w_t > 0.  The order of the additions is part of the rule: the host twin runs the
//    same network (biased_scan_host).  fp contraction is off in every function that forms or adds weights.
//  * Position, with replacement: start_t + rw_index(r, n_t).
//  * Position, without replacement: Floyd's subset algorithm per tag, no rejection loop.  With k_t the number of picks
//    of the row that drew tag t and j the number of EARLIER picks that drew it, m = n_t - k_t + j and
//    c = rw_index(r, m + 1); the position is start_t + m when an earlier pick of the tag took c, else start_t + c.  The
//    picks of a tag are a uniform k_t-subset of its range, so the law is the one of successive sampling (BiasedChoice).
//  * Output of pick p at out_indptr[i] + p: indices[lo + pos] and data ? data[lo + pos] : lo + pos.
//
// Integer arithmetic, fp64 multiplies that feed compares or the additions of the network, fp64 adds in a fixed order:
// host and device agree bit for bit.
#pragma once
#include <stdint.h>

#include "topk_step.h"   // topk_row, topk_eid, DGLA_RW_HD and the generator of random_walk_step.h

namespace dgla {

constexpr int kBiasedMaxTags = 1024;   // the largest T the sampler accepts (the sort has no bound)
constexpr int kBiasedSlotTag = 0, kBiasedSlotPos = 1;

// flag bits of a call
enum : int { kBiasedBadTag = 1, kBiasedBadEid = 2, kBiasedHub = 4, kBiasedBadSeed = 8 };

// the tag of edge id e, or -1 with *flags updated when e or the tag is out of range
template <typename TagPtr>
DGLA_RW_HD int64_t biased_tag(TagPtr tag, int64_t nnz, int64_t num_tags, int64_t e, int* flags) {
  if (e < 0 || e >= nnz) {
    *flags |= kBiasedBadEid;
    return -1;
  }
  const int64_t t = static_cast<int64_t>(tag[e]);
  if (t < 0 || t >= num_tags) {
    *flags |= kBiasedBadTag;
    return -1;
  }
  return t;
}

// the width of the lane group that owns a seed
DGLA_RW_HD int biased_width(int64_t num_tags) { return num_tags <= 16 ? 16 : 64; }

// start_t and n_t of tag t of a row of `deg` entries (off = the row's T + 1 offsets)
template <typename OffPtr>
DGLA_RW_HD void biased_range(OffPtr off, int64_t t, int64_t deg, int64_t* start, int64_t* n) {
  int64_t a = static_cast<int64_t>(off[t]), b = static_cast<int64_t>(off[t + 1]);
  a = a < 0 ? 0 : (a > deg ? deg : a);
  b = b < a ? a : (b > deg ? deg : b);
  *start = a;
  *n = b - a;
}

// b_t
template <typename B>
DGLA_RW_HD double biased_bias(B raw) {
  const double b = static_cast<double>(raw);
  return (b > 0.0 && b <= 1.7976931348623157e308) ? b : 0.0;
}

// w_t; the product is rounded on its own
DGLA_RW_HD double biased_weight(int64_t remaining, double b) {
#pragma clang fp contract(off)
  return remaining > 0 && b > 0.0 ? static_cast<double>(remaining) * b : 0.0;
}

DGLA_RW_HD double biased_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

DGLA_RW_HD double biased_target(uint64_t r, double total) {
#pragma clang fp contract(off)
  return rw_uniform(r) * total;
}

// the number of picks of a row with P entries in positive-bias ranges
DGLA_RW_HD int64_t biased_picks(int64_t P, int64_t fanout, bool replace) {
  if (fanout < 0) return P;
  if (replace) return P > 0 ? fanout : 0;
  return fanout < P ? fanout : P;
}

// P of seed row u (off = its offsets), a plain loop: the count pass and the host twin
template <typename OffPtr, typename BiasPtr>
DGLA_RW_HD int64_t biased_positive(OffPtr off, BiasPtr bias, int64_t num_tags, int64_t deg) {
  int64_t P = 0;
  for (int64_t t = 0; t < num_tags; ++t) {
    int64_t s, n;
    biased_range(off, t, deg, &s, &n);
    if (biased_bias(bias[t]) > 0.0) P += n;
  }
  return P;
}

// the Hillis-Steele network over x[0 .. W), as the lanes run it
inline void biased_scan_host(double* x, int W) {
  for (int d = 1; d < W; d <<= 1)
    for (int l = W - 1; l >= d; --l) x[l] = biased_add(x[l], x[l - d]);
}

// Floyd's step: the row-relative position of a pick of tag (start, n) that k picks of the row drew, j of them earlier,
// given c = rw_index(r, m + 1) and whether an earlier pick of the tag took c
DGLA_RW_HD int64_t biased_floyd_m(int64_t n, int64_t k, int64_t j) { return n - k + j; }

}  // namespace dgla
