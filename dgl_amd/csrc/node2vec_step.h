// The step rule of dgl_amd.sampling.node2vec_random_walk (include/dgl_amd.h, "node2vec walks"): ONE definition, compiled
// for the device (node2vec_walk_kernel, csrc/node2vec.hip) and for the host (dgla_node2vec_walk_host), so the two
// cannot drift.  The generator, the draws and the weighted pick are those of csrc/random_walk_step.h, included below.
//
// Setting.  One relation with num_rows == num_cols, as its out-edge CSR (indptr, indices, data = edge-id map or NULL),
// an optional CDF (double[nnz] from dgla_random_walk_cdf, NULL = uniform) and a membership list member[nnz]: the
// column ids of every row in ascending order, duplicates kept, over the same indptr (dgla_csr_sorted_columns).
//
// Parameters.  p and q are finite and > 0.  The host computes, once per call,
//     m = max(1/p, 1, 1/q),   a0 = (1/p)/m,   a1 = 1/m,   a2 = (1/q)/m
// and refuses the call when m is not finite or some a is not > 0; the walk itself divides nothing.
//
// Class of a candidate x when the previous node is prev: class 0 if x == prev (a self-loop or a duplicate edge is
// judged by node id); else class 1 if the edge x -> prev exists, i.e. a bisection of member[indptr[x] .. indptr[x+1])
// finds prev; else class 2.  a_class(x) is a0, a1 or a2.
//
// Step t = 0 of walk i at its seed: rules 2-5 of csrc/random_walk_step.h (no restart), the pick from slot 0.
// Step t >= 1 at curr with row [lo, hi), deg = hi - lo, the node before curr being prev:
//  1. If deg == 0, the walk halts.
//  2. Weighted relation: total = cdf[hi-1]; if !(total > 0) or total is not finite, the walk halts.
//  3. Bounded rejection.  K = min(max(deg, 8), 1024).  For attempt k = 0 .. K-1: the candidate position is
//     pos = lo + index(r(seed,i,t,2k), deg) (uniform) or the weighted pick of rule 4 of csrc/random_walk_step.h with
//     r(seed,i,t,2k) (weighted); x = indices[pos]; the candidate is accepted iff u(seed,i,t,2k+1) < a_class(x).
//     (A class whose a is 1.0 always accepts, because u < 1.)
//  4. After K rejections, an exact scan of the row in position order, in fp64, every operation rounded on its own:
//     d_j = 1 (uniform) or cdf[j] - (j > lo ? cdf[j-1] : 0) (weighted);  g_j = fl(d_j * a_class(indices[j]));
//     S = fl(S + g_j) for j = lo .. hi-1 in that order, from S = 0.  If !(S > 0), the walk halts.
//     x = u(seed,i,t,2K) * S.  A second pass forms the same running sum and takes the first j whose running sum
//     is > x.  If there is none (rounding), it takes the last j with g_j > 0.
//  5. trace[i][t+1] = indices[pos], eids[i][t] = data ? data[pos] : pos, prev = curr, curr = indices[pos].
// A halted walk writes -1 into trace[i][t+1 ..] and eids[i][t ..].  trace[i][0] = seeds[i] always.  A seed outside
// [0, num_rows) halts at once and touches no memory through that id.
//
// What follows from the rule.  Picks are a pure function of (seed, walk index, step, slot).  Rejection and the scan
// draw from the same law, P(j) proportional to d_j * a_class(indices[j]), so falling through after K rejections does
// not bias the walk.  With p == q == 1 every a is 1.0, attempt 0 accepts, and the walk is the one of
// csrc/random_walk_step.h under the same seed, bit for bit.  A step costs at most K attempts and two scans of the row.
//
// K follows the degree because an attempt and one row position of the scan cost about the same (one gather and one
// bisection): K is part of the rule, not a tuned number.
//
// Floating point.  g_j and S are a multiply followed by an add: two roundings.  A device compiler contracts the pair
// into one fused multiply-add (one rounding) unless told otherwise, a host compiler does not, and the two would then
// disagree in the last bit of S: `#pragma clang fp contract(off)` in n2v_scan keeps them apart on every target.
// Everything else is integer arithmetic, single fp64 operations and fp64 compares.
#pragma once
#include "random_walk_step.h"

namespace dgla {

constexpr int64_t kN2vMinAttempts = 8, kN2vMaxAttempts = 1024;  // K = min(max(deg, 8), 1024)

// The CDF argument of the walkers below is one of these two, so that "is the relation weighted" is decided where the
// walker is instantiated and not by a test of a pointer at run time.  The kernel needs it that way: with the test
// inside the attempt loop, the device compiler kept its outcome as a lane mask covering the lanes of the loop's LAST
// iteration, and the scan behind the loop read that mask for lanes that had left the loop earlier (a smaller K): they
// took the weighted path with a null CDF.
struct N2vUniform {  // no CDF
  DGLA_RW_HD explicit operator bool() const { return false; }
  DGLA_RW_HD double operator[](int64_t) const { return 0.0; }
};
template <typename CdfPtr>
struct N2vWeighted {  // a CDF that is there
  CdfPtr p;
  DGLA_RW_HD explicit operator bool() const { return true; }
  DGLA_RW_HD double operator[](int64_t j) const { return p[j]; }
};

struct N2vAccept {  // a0, a1, a2: computed on the host, by value to the kernel
  double a[3];
};

// m and the three acceptance probabilities from p and q; false when the parameters cannot be used
inline bool n2v_accept(double p, double q, N2vAccept* out) {
  if (!(p > 0.0) || !(q > 0.0) || !(p <= 1.7976931348623157e308) || !(q <= 1.7976931348623157e308)) return false;
  const double ip = 1.0 / p, iq = 1.0 / q;
  double m = ip > 1.0 ? ip : 1.0;
  m = iq > m ? iq : m;
  if (!(m <= 1.7976931348623157e308)) return false;
  out->a[0] = ip / m, out->a[1] = 1.0 / m, out->a[2] = iq / m;
  return out->a[0] > 0.0 && out->a[1] > 0.0 && out->a[2] > 0.0;
}

// does the row [xlo, xhi) of the membership list hold `prev`?  (a bisection that stops at the first hit)
template <typename IdxPtr>
DGLA_RW_HD bool n2v_member(IdxPtr member, int64_t xlo, int64_t xhi, int64_t prev) {
  while (xlo < xhi) {
    const int64_t m = xlo + ((xhi - xlo) >> 1);
    const int64_t v = static_cast<int64_t>(member[m]);
    if (v == prev) return true;
    if (v < prev) xlo = m + 1; else xhi = m;
  }
  return false;
}

// a_class(x), through the row of x
template <typename IdxPtr>
DGLA_RW_HD double n2v_accept_of(IdxPtr indptr, IdxPtr member, const N2vAccept& a, int64_t x, int64_t prev) {
  if (x == prev) return a.a[0];
  return n2v_member(member, static_cast<int64_t>(indptr[x]), static_cast<int64_t>(indptr[x + 1]), prev) ? a.a[1] : a.a[2];
}

// rule 4: the position the exact scan takes for the draw r, or -1 when the row carries no mass
template <typename IdxPtr, typename CdfPtr>
DGLA_RW_HD int64_t n2v_scan(IdxPtr indptr, IdxPtr indices, IdxPtr member, CdfPtr cdf, const N2vAccept& a, int64_t prev,
                            int64_t lo, int64_t hi, uint64_t r) {
#pragma clang fp contract(off)
  // g_j; a position without mass needs no class (0 * a is 0 whatever the class)
  auto g_at = [&](int64_t j) {
#pragma clang fp contract(off)
    const double d = cdf ? cdf[j] - (j > lo ? cdf[j - 1] : 0.0) : 1.0;
    if (!(d > 0.0)) return 0.0;
    return d * n2v_accept_of(indptr, member, a, static_cast<int64_t>(indices[j]), prev);
  };
  double S = 0.0;
  for (int64_t j = lo; j < hi; ++j) S = S + g_at(j);
  if (!(S > 0.0)) return -1;
  const double x = rw_uniform(r) * S;
  double run = 0.0;
  int64_t last = -1;
  for (int64_t j = lo; j < hi; ++j) {
    const double g = g_at(j);
    run = run + g;
    if (run > x) return j;
    if (g > 0.0) last = j;
  }
  return last;
}

struct N2vPick {
  int64_t pos;       // CSR position taken, or -1: the walk halts
  int64_t x;         // indices[pos]
  int64_t xlo, xhi;  // the row of x when the step loaded it (has_row), so that the next step does not load it again
  bool has_row;
};

// Rules 1-4 for one walk at a node whose row is [lo, hi).  stats (host only, may be NULL): [1] += candidates drawn,
// [2] += 1 when the step reaches the scan.
template <typename IdxPtr, typename CdfPtr>
DGLA_RW_HD N2vPick n2v_step(IdxPtr indptr, IdxPtr indices, IdxPtr member, CdfPtr cdf, const N2vAccept& a,
                            uint64_t step_key, int64_t prev, int64_t lo, int64_t hi, int64_t* stats) {
  N2vPick out{-1, -1, 0, 0, false};
  const int64_t deg = hi - lo;
  if (deg == 0) return out;
  // what an acceptance draw decides without knowing whether x -> prev exists: below both of a1, a2 it accepts, at or
  // above both it rejects, and the row of x is not read
  const double a_min = a.a[1] < a.a[2] ? a.a[1] : a.a[2], a_max = a.a[1] < a.a[2] ? a.a[2] : a.a[1];
  int64_t K = deg > kN2vMinAttempts ? deg : kN2vMinAttempts;
  K = K < kN2vMaxAttempts ? K : kN2vMaxAttempts;
  for (int64_t k = 0; k < K; ++k) {
    const uint64_t r = rw_draw(step_key, static_cast<uint64_t>(2 * k));
    const int64_t pos = cdf ? rw_pick_weighted(cdf, lo, hi, r) : lo + static_cast<int64_t>(rw_index(r, static_cast<uint64_t>(deg)));
    if (pos < 0) return out;  // rule 2 (the same test at every attempt: it fails at the first or never)
    if (stats) ++stats[1];
    const int64_t x = static_cast<int64_t>(indices[pos]);
    const double u = rw_uniform(rw_draw(step_key, static_cast<uint64_t>(2 * k + 1)));
    bool accept, has_row = false;
    int64_t xlo = 0, xhi = 0;
    if (x == prev) {
      accept = u < a.a[0];
    } else if (u < a_min) {
      accept = true;
    } else if (!(u < a_max)) {
      accept = false;
    } else {
      xlo = static_cast<int64_t>(indptr[x]), xhi = static_cast<int64_t>(indptr[x + 1]);
      has_row = true;
      accept = u < (n2v_member(member, xlo, xhi, prev) ? a.a[1] : a.a[2]);
    }
    if (accept) return N2vPick{pos, x, xlo, xhi, has_row};
  }
  if (stats) ++stats[2];
  const int64_t pos = n2v_scan(indptr, indices, member, cdf, a, prev, lo, hi, rw_draw(step_key, static_cast<uint64_t>(2 * K)));
  if (pos >= 0) out.pos = pos, out.x = static_cast<int64_t>(indices[pos]);
  return out;
}

// One whole walk: trace[i][0] = seeds[i], the range test of the seed, step 0 by rw_step, the later steps by n2v_step and
// the -1 padding after a halt.  tr = trace[i], ev = eids[i] or NULL.  stats (host only, may be NULL): [0] += steps
// t >= 1 that recorded a node, [1] and [2] as in n2v_step.
template <typename Idx, typename IdxPtr, typename CdfPtr>
DGLA_RW_HD void n2v_walk(IdxPtr indptr, IdxPtr indices, IdxPtr data, IdxPtr member, CdfPtr cdf, int64_t num_rows,
                         const N2vAccept& a, int64_t num_steps, uint64_t rng_seed, int64_t i, Idx seed_node, Idx* tr,
                         Idx* ev, int64_t* stats) {
  int64_t curr = static_cast<int64_t>(seed_node), prev = -1, lo = 0, hi = 0;
  tr[0] = seed_node;
  const uint64_t key = rw_walk_key(rng_seed, static_cast<uint64_t>(i));
  bool alive = curr >= 0 && curr < num_rows;
  for (int64_t t = 0; t < num_steps; ++t) {
    Idx nxt = Idx(-1), e = Idx(-1);
    if (alive) {
      const uint64_t step_key = rw_step_key(key, static_cast<uint64_t>(t));
      N2vPick pk{-1, -1, 0, 0, false};
      if (t == 0) {
        pk.pos = rw_step(indptr, cdf, step_key, 0.0, curr);
        if (pk.pos >= 0) pk.x = static_cast<int64_t>(indices[pk.pos]);
      } else {
        pk = n2v_step(indptr, indices, member, cdf, a, step_key, prev, lo, hi, stats);
        if (stats && pk.pos >= 0) ++stats[0];
      }
      if (pk.pos >= 0) {
        nxt = static_cast<Idx>(pk.x);
        e = data ? data[pk.pos] : static_cast<Idx>(pk.pos);
        prev = curr, curr = pk.x;
        if (t + 1 < num_steps) {  // the next step's row: the accepted candidate's when the step read it
          lo = pk.has_row ? pk.xlo : static_cast<int64_t>(indptr[curr]);
          hi = pk.has_row ? pk.xhi : static_cast<int64_t>(indptr[curr + 1]);
        }
      } else {
        alive = false;
      }
    }
    tr[t + 1] = nxt;
    if (ev) ev[t] = e;
  }
}

}  // namespace dgla
