// The rule of dgl_amd.geometry.neighbor_matching (include/dgl_amd.h, "Graph matching"): ONE definition, compiled for the
// device (matching_propose_kernel / matching_respond_kernel, csrc/matching.hip) and for the host
// (dgla_neighbor_matching_host), so the two cannot drift.
//
// Input.  One CSR (indptr[n + 1], indices[nnz], data[nnz] = the edge-id map or NULL; int32 or int64 ids), optional
// non-negative edge weights indexed by EDGE ID (fp32 or fp64) and a 64-bit seed.
//
// State.  label[n] = -1 and prop[n] = -1 (kMatchNone), both in the id type.  Rounds t = 0, 1, ...; a node is ACTIVE in
// round t when its label is negative at the start of the round.
//
// Colour.  Node v in round t is BLUE when rw_draw(rw_step_key(rw_walk_key(seed, v), t), 0) < kMatchBlue, else RED
// (the generator of csrc/random_walk_step.h, unchanged).  kMatchBlue = floor(0.53406 * 2^64), the BLUE_P of the
// reference's edge_coarsening_impl.cu (Fagginger Auer and Bisseling).  A colour is a function of (seed, v, t) only; it
// is never stored, and a neighbour's colour is recomputed in registers.
//
// Key of entry q = (u -> v): the tuple (w', h, v).  w' = rw_weight(weight[data ? data[q] : q]) (negative and NaN count
// as 0, so every active neighbour stays a candidate); without weights w' = 0 and no weight array exists or is read.
// h = match_hash(seed, u, v), a 64-bit mix of (seed, min(u, v), max(u, v)): both directions of an edge agree on it, and
// it breaks weight ties at random.  The larger (w', h) wins; on a full tie the smaller v wins.  Entries with v == u, and
// entries whose v is outside [0, n), are ignored (no memory is touched through such an id).
//
// Propose (reads label, writes only prop[u], for every active u).  No active neighbour: prop[u] = kMatchSingle.  Else
// if u is BLUE: prop[u] = the active RED neighbour with the best key, or kMatchNone if there is none.  Else kMatchNone.
//
// Respond (reads prop, writes label).  An active u with prop[u] == kMatchSingle takes label[u] = u.  An active RED u
// picks the neighbour v with the best key among those that are BLUE and proposed to u in this round, and sets
// label[u] = label[v] = min(u, v).  Nobody else writes label[v], and its only reader in this phase is v itself, a BLUE
// node whose prop is not kMatchSingle, which does nothing whichever value it sees.
//
// "In this round" without a round tag: propose rewrites prop[v] of EVERY active v in every round, and only a BLUE v
// writes a node id, so for an active v the test prop[v] == u is this round's proposal and needs neither label[v] nor
// v's colour.  An inactive v keeps the prop of the round r in which it matched.  If that prop names u, then in round r
// u was active and RED and saw the proposal of v through this very entry u -> v, so u picked a proposer and matched in
// round r: an active u never meets a stale prop[v] == u.
//
// End.  The loop ends when no node is active; `rounds` counts the rounds that started with an active node.  A CSR that
// is not symmetric can cycle for ever (a directed 3-cycle does), so the loop also stops at max_rounds.
//
// Integer arithmetic and fp64 compares only: host and device agree bit for bit.  The pointer types are template
// parameters so that the kernels can hand in pointers that name the global address space.
#pragma once
#include <stdint.h>

#include "random_walk_step.h"

namespace dgla {

constexpr int64_t kMatchNone = -1;    // prop: no proposal
constexpr int64_t kMatchSingle = -2;  // prop: no active neighbour, the node becomes a cluster of its own
constexpr uint64_t kMatchBlue = 0x88b827fa1a0cf000ull;  // floor(0.53406 * 2^64) with 0.53406 the nearest fp64
static_assert(kMatchBlue == static_cast<uint64_t>(0.53406 * 18446744073709551616.0), "kMatchBlue is BLUE_P * 2^64");
constexpr uint64_t kMatchHashSalt = 0x6D61746368696E67ull;  // keeps the edge hashes off the colour stream

DGLA_RW_HD bool match_is_blue(uint64_t seed, int64_t v, int64_t t) {
  return rw_draw(rw_step_key(rw_walk_key(seed, static_cast<uint64_t>(v)), static_cast<uint64_t>(t)), 0) < kMatchBlue;
}

DGLA_RW_HD uint64_t match_hash(uint64_t seed, int64_t u, int64_t v) {
  const int64_t a = u < v ? u : v, b = u < v ? v : u;
  return rw_step_key(rw_walk_key(seed ^ kMatchHashSalt, static_cast<uint64_t>(a)), static_cast<uint64_t>(b));
}

struct MatchKey {  // v < 0: no entry
  double w;
  uint64_t h;
  int64_t v;
};

DGLA_RW_HD MatchKey match_no_key() { return MatchKey{0.0, 0, -1}; }

// does a beat b?  (a total order on the entries of one row up to duplicates of one entry, so any reduction order works)
DGLA_RW_HD bool match_better(const MatchKey& a, const MatchKey& b) {
  if (a.v < 0) return false;
  if (b.v < 0) return true;
  if (a.w != b.w) return a.w > b.w;
  if (a.h != b.h) return a.h > b.h;
  return a.v < b.v;
}

template <bool WEIGHTED, typename IdxPtr, typename WPtr>
DGLA_RW_HD MatchKey match_key(IdxPtr data, WPtr weight, uint64_t seed, int64_t u, int64_t v, int64_t q) {
  double w = 0.0;
  if constexpr (WEIGHTED) w = rw_weight(weight[data ? static_cast<int64_t>(data[q]) : q]);
  return MatchKey{w, match_hash(seed, u, v), v};
}

// Propose, entry q of the active row u: 0 = ignored (v == u or v inactive), 1 = an active neighbour, 2 = an active RED
// neighbour of a BLUE u, *key filled.  A RED u only needs to know whether an active neighbour exists.
template <bool WEIGHTED, typename IdxPtr, typename WPtr, typename LabelPtr>
DGLA_RW_HD int match_propose_entry(IdxPtr indices, IdxPtr data, WPtr weight, LabelPtr label, int64_t n, uint64_t seed,
                                   int64_t t, int64_t u, bool u_blue, int64_t q, MatchKey* key) {
  const int64_t v = static_cast<int64_t>(indices[q]);
  if (v == u || v < 0 || v >= n || label[v] >= 0) return 0;
  if (!u_blue || match_is_blue(seed, v, t)) return 1;
  *key = match_key<WEIGHTED>(data, weight, seed, u, v, q);
  return 2;
}

// the prop of an active u after its row: `any` = it has an active neighbour, `best` = the best key of the 2-entries
DGLA_RW_HD int64_t match_proposal(bool any, bool u_blue, const MatchKey& best) {
  if (!any) return kMatchSingle;
  return u_blue && best.v >= 0 ? best.v : kMatchNone;
}

// Respond, entry q of the active RED row u: whether v proposed to u in this round (see "In this round" above)
template <bool WEIGHTED, typename IdxPtr, typename WPtr, typename PropPtr>
DGLA_RW_HD bool match_respond_entry(IdxPtr indices, IdxPtr data, WPtr weight, PropPtr prop, int64_t n, uint64_t seed,
                                    int64_t u, int64_t q, MatchKey* key) {
  const int64_t v = static_cast<int64_t>(indices[q]);
  if (v == u || v < 0 || v >= n || static_cast<int64_t>(prop[v]) != u) return false;
  *key = match_key<WEIGHTED>(data, weight, seed, u, v, q);
  return true;
}

}  // namespace dgla
