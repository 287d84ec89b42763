// The rule of dgl_amd.sampling.global_uniform_negative_sampling (include/dgl_amd.h, "Negative sampling"): ONE
// definition, compiled for the device (csrc/negative_sampling.hip) and for the host (dgla_negative_sample_host), so
// the two cannot drift.  The generator and the draws are those of csrc/random_walk_step.h, the edge test is n2v_member of
// csrc/node2vec_step.h, both included below and used unchanged.
//
// Setting.  One relation as its out-edge CSR (R = num_rows source nodes, C = num_cols destination nodes, indptr) and
// its membership list member[nnz]: the column ids of every row in ascending order, duplicates kept, over the same
// indptr (dgla_csr_sorted_columns).  Parameters: n_slots >= 0 slots, num_samples >= 0 result entries, num_trials T in
// 1..64, the flags exclude_self_loops and replace, and a 64-bit seed.
//
// The rule:
//  1. Draw.  For slot i in [0, n_slots), trial t = 0 .. T-1:  s = rw_step_key(rw_walk_key(seed, i), t),
//     u = rw_index(rw_draw(s, 0), R), v = rw_index(rw_draw(s, 1), C).  The trial is rejected in either of two cases:
//     exclude_self_loops and u == v; or n2v_member(member, indptr[u], indptr[u+1], v) finds v (u -> v is an edge).
//     The first trial that is not rejected gives the slot its pair (u, v).  A slot with T rejections is empty.
//     R == 0 or C == 0 leaves every slot empty and reads no graph memory.
//  2. Accept.  A is the list of non-empty slots in ascending i.
//  3. Select.  With replace, the result is the first min(|A|, num_samples) pairs of A.  Without replace, first drop
//     from A every slot whose pair equals the pair of an earlier slot of A (first occurrences are kept, in slot order),
//     then take the first num_samples.
//  4. Pad.  out_src and out_dst have num_samples entries of the CSR's id type; the entries beyond the count are -1.
//     The count is one int64.
//
// What follows from the rule.  The result is a pure function of (graph, seed, n_slots, num_samples, T, flags),
// whatever the launch geometry.  The result for num_samples = k is a prefix of the result for k' > k at the same
// n_slots.  A slot's pair is uniform over the cells that are neither edges nor (when excluded) self-loops, slots are
// independent, and first occurrences are kept in slot order, so the truncation to num_samples is an unbiased sample
// without replacement.  How duplicates are found (a hash bucket sort on the device, a set on the host) is no part of
// the rule.
//
// Integer arithmetic and integer compares only: host and device agree bit for bit.
#pragma once
#include "node2vec_step.h"

namespace dgla {

constexpr int kNegMaxTrials = 64;  // T in 1 .. 64

// Rule 1 for slot i: true and (*u, *v) when some trial is not rejected.  EXCL (exclude_self_loops) is a compile-time
// switch and not a flag tested inside the loop that lanes leave at different trials (N2vUniform in node2vec_step.h
// records what a run-time test of that shape compiled to).
template <bool EXCL, typename IdxPtr>
DGLA_RW_HD bool neg_draw(IdxPtr indptr, IdxPtr member, int64_t R, int64_t C, int T, uint64_t seed, int64_t i, int64_t* u,
                         int64_t* v) {
  if (R <= 0 || C <= 0) return false;
  const uint64_t key = rw_walk_key(seed, static_cast<uint64_t>(i));
  for (int t = 0; t < T; ++t) {
    const uint64_t s = rw_step_key(key, static_cast<uint64_t>(t));
    const int64_t uu = static_cast<int64_t>(rw_index(rw_draw(s, 0), static_cast<uint64_t>(R)));
    const int64_t vv = static_cast<int64_t>(rw_index(rw_draw(s, 1), static_cast<uint64_t>(C)));
    if (EXCL && uu == vv) continue;
    if (n2v_member(member, static_cast<int64_t>(indptr[uu]), static_cast<int64_t>(indptr[uu + 1]), vv)) continue;
    *u = uu, *v = vv;
    return true;
  }
  return false;
}

// is u -> v an edge?  An id out of range is no edge and touches no memory.
template <typename IdxPtr>
DGLA_RW_HD bool neg_has_edge(IdxPtr indptr, IdxPtr member, int64_t R, int64_t C, int64_t u, int64_t v) {
  if (u < 0 || u >= R || v < 0 || v >= C) return false;
  return n2v_member(member, static_cast<int64_t>(indptr[u]), static_cast<int64_t>(indptr[u + 1]), v);
}

// The bucket of a pair in the duplicate search: an implementation detail of the device path, not of the rule.
DGLA_RW_HD uint64_t neg_pair_hash(int64_t u, int64_t v) {
  return rw_mix64(rw_mix64(static_cast<uint64_t>(u)) + static_cast<uint64_t>(v));
}

}  // namespace dgla
