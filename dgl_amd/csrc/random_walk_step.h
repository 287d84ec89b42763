// The step rule of dgl_amd.sampling.random_walk (include/dgl_amd.h, "Random walks"): ONE definition, compiled for the
// device (random_walk_kernel, csrc/random_walk.hip) and for the host (dgla_random_walk_host), so the two cannot drift.
//
// Generator.  mix64 is the function of csrc/sampling.hip (the splitmix64 finaliser including its increment).  For walk
// index i (position in `seeds`, not the node id, so a node listed twice gets two independent walks), step t (0-based)
// and draw slot k:
//     r(seed,i,t,k) = mix64( mix64( mix64(seed ^ (i * 0xD1B54A32D192ED03)) + t ) + k )      (all mod 2^64)
//     uniform index in [0,n):  (r * n) >> 64    (multiply-high)
//     uniform double in [0,1): (r >> 11) * 2^-53
// Slot 0 is the neighbour pick and slot 1 is the restart test.
//
// One step of walk i at node curr, step t, relation R = rels[metapath[t]].  R is the out-edge CSR: rows are source
// nodes, `indices` are successors, and `data` is the edge-id map or NULL.
//  1. Restart: if a restart probability p_t is given (scalar, or restart_steps[t] converted to double) and
//     u(seed,i,t,1) < p_t, the walk halts.
//  2. lo = indptr[curr], hi = indptr[curr+1].  If hi == lo, the walk halts.
//  3. Uniform relation (cdf == NULL): pos = lo + index(r(seed,i,t,0), hi - lo).
//  4. Weighted relation: total = cdf[hi-1].  If !(total > 0) or total is not finite, the walk halts.  Otherwise
//     x = u(seed,i,t,0) * total (one fp64 multiply).  pos is the first position in [lo,hi) with cdf[pos] > x.  If there
//     is none (rounding), pos is the first position with cdf[pos] == total.  The search is a bisection, O(log deg).
//  5. trace[i][t+1] = indices[pos], eids[i][t] = data ? data[pos] : pos, curr = indices[pos].
// A halted walk writes -1 into trace[i][t+1 ..] and eids[i][t ..].  trace[i][0] = seeds[i] always.  A seed outside
// [0, num_rows of rels[metapath[0]]) halts at once and touches no memory through that id.
//
// CDF of a relation, as double[nnz] in CSR position order: cdf[pos] = sum_{q = lo..pos} w'(q), with
// w'(q) = max((double)prob[data ? data[q] : q], 0) and NaN -> 0.  `prob` is indexed by EDGE ID.  The order of additions
// is free, but cdf never decreases inside a row, and w'(pos) == 0 implies cdf[pos] == cdf[pos-1], so a zero-weight
// edge is never picked.
//
// Integer arithmetic, one IEEE fp64 multiply and fp64 compares only: host and device agree bit for bit.  The pointer
// types are template parameters so that the kernel can hand in pointers that name the global address space.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DGLA_RW_HD __host__ __device__ inline
#else
#define DGLA_RW_HD inline
#endif

namespace dgla {

DGLA_RW_HD uint64_t rw_mix64(uint64_t z) {  // splitmix64 finaliser (csrc/sampling.hip mix64)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the three levels of r(seed,i,t,k): per walk, per step, per draw slot
DGLA_RW_HD uint64_t rw_walk_key(uint64_t seed, uint64_t i) { return rw_mix64(seed ^ (i * 0xD1B54A32D192ED03ull)); }
DGLA_RW_HD uint64_t rw_step_key(uint64_t walk_key, uint64_t t) { return rw_mix64(walk_key + t); }
DGLA_RW_HD uint64_t rw_draw(uint64_t step_key, uint64_t k) { return rw_mix64(step_key + k); }

DGLA_RW_HD uint64_t rw_index(uint64_t r, uint64_t n) {  // (r * n) >> 64
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, n);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(r) * n) >> 64);
#endif
}

DGLA_RW_HD double rw_uniform(uint64_t r) { return static_cast<double>(r >> 11) * (1.0 / 9007199254740992.0); }

constexpr int kRwSlotPick = 0, kRwSlotRestart = 1;

// w'(q) of the CDF: negative and NaN weights count as 0
template <typename W>
DGLA_RW_HD double rw_weight(W p) {
  const double w = static_cast<double>(p);
  return w > 0.0 ? w : 0.0;
}

// rule 4: the position in [lo, hi) that x = u * total selects, or -1 when the row has no usable weight
template <typename CdfPtr>
DGLA_RW_HD int64_t rw_pick_weighted(CdfPtr cdf, int64_t lo, int64_t hi, uint64_t r) {
  const double total = cdf[hi - 1];
  if (!(total > 0.0) || !(total <= 1.7976931348623157e308)) return -1;
  const double x = rw_uniform(r) * total;
  int64_t a = lo, b = hi;  // first position with cdf > x
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (cdf[m] > x) b = m; else a = m + 1;
  }
  if (a < hi) return a;
  a = lo, b = hi - 1;  // rounding put x at total: first position with cdf == total (cdf[hi-1] is one)
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (cdf[m] >= total) b = m; else a = m + 1;
  }
  return a;
}

// Rules 1-5 for one walk at `curr`.  Returns the CSR position taken, or -1 when the walk halts.  p_t <= 0 (or NaN) never
// restarts, so "no restart" is p_t = 0 and costs no draw.
template <typename IdxPtr, typename CdfPtr>
DGLA_RW_HD int64_t rw_step(IdxPtr indptr, CdfPtr cdf, uint64_t step_key, double p_t, int64_t curr) {
  if (p_t > 0.0 && rw_uniform(rw_draw(step_key, kRwSlotRestart)) < p_t) return -1;
  const int64_t lo = static_cast<int64_t>(indptr[curr]), hi = static_cast<int64_t>(indptr[curr + 1]);
  if (hi == lo) return -1;
  const uint64_t r = rw_draw(step_key, kRwSlotPick);
  if (!cdf) return lo + static_cast<int64_t>(rw_index(r, static_cast<uint64_t>(hi - lo)));
  return rw_pick_weighted(cdf, lo, hi, r);
}

// One whole walk around rw_step: trace[i][0] = seeds[i], the range test of the seed, and the -1 padding after a halt.
// rel_at(t) gives the relation of step t (members indptr, indices, data, cdf, num_rows; any pointer types), p_at(t) the
// restart probability of step t as a double (0 = none).  tr = trace[i], ev = eids[i] or NULL.
template <typename Idx, typename RelAt, typename PAt>
DGLA_RW_HD void rw_walk(RelAt rel_at, PAt p_at, int64_t num_steps, uint64_t rng_seed, int64_t i, Idx seed_node, Idx* tr,
                        Idx* ev) {
  int64_t curr = static_cast<int64_t>(seed_node);
  tr[0] = seed_node;
  const uint64_t key = rw_walk_key(rng_seed, static_cast<uint64_t>(i));
  bool alive = true;
  for (int64_t t = 0; t < num_steps; ++t) {
    const auto R = rel_at(t);
    // (later steps need no range test: the caller checked that the metapath chains, num_cols == next num_rows)
    if (t == 0 && (curr < 0 || curr >= R.num_rows)) alive = false;
    Idx nxt = Idx(-1), e = Idx(-1);
    if (alive) {
      const int64_t pos = rw_step(R.indptr, R.cdf, rw_step_key(key, static_cast<uint64_t>(t)), p_at(t), curr);
      if (pos >= 0) {
        nxt = R.indices[pos];
        e = R.data ? R.data[pos] : static_cast<Idx>(pos);
        curr = static_cast<int64_t>(nxt);
      } else {
        alive = false;
      }
    }
    tr[t + 1] = nxt;
    if (ev) ev[t] = e;
  }
}

}  // namespace dgla
