// The rule of top-k neighbour selection (include/dgl_amd.h, "Top-k neighbour selection"): ONE definition, compiled for
// the device (csrc/topk.hip) and for the host twin (dgla_select_topk_host), so the two cannot drift.
//
// Input.  One CSR (indptr[num_rows + 1], indices[nnz], data[nnz] = the edge-id map or NULL; int32 or int64 ids): the
// in-edge CSR for edge_dir = "in", the out-edge CSR for "out".  `weight` holds one value per EDGE ID (fp32, fp64, fp16,
// bf16, int32 or int64), a list of seed rows, k and a direction.
//
// Key of an edge.  An order-preserving map of its weight to an unsigned integer: 32 bits for fp32 / fp16 / bf16 / int32,
// 64 bits for fp64 / int64.  Floats: -0.0 becomes +0.0, then a set sign bit complements the pattern and a clear one sets
// it (the sign-flip map).  fp16 and bf16 widen to the fp32 pattern first (exactly, with integer operations), so values
// that collide after rounding share a key.  Signed integers have their sign bit flipped.  ascending complements the
// key.  NaN loses to every number in both directions: after the direction is applied its key is 0, below the key of
// every float that is a number (those lie in [0x007FFFFF, 0xFF800000], resp. the 64-bit analogue).  An edge id outside
// [0, nnz) reads no weight and gets key 0 as well.
//
// Total order within a row.  Larger key first; among equal keys the smaller EDGE ID first (not the CSR position, so the
// result is a function of (graph, weights) whichever sparse format is read); among equal edge ids, which only a
// malformed edge-id map produces, the smaller position.  The order is strict.
//
// Picks of seed i.  picks = min(k, deg), k = -1: deg, k = 0: none.  The picks are the first `picks` entries of the row
// in that order, emitted in rank order (best first) at out_indptr[i] + rank.  A seed listed twice is selected twice.
//
// Row bounds are clamped into [0, nnz] as in exclude_row, so a malformed indptr reads nothing outside the arrays; a
// seed outside [0, num_rows) is an empty row and touches no memory (and is reported).
//
// Integer comparisons only: host and device agree bit for bit.  The pointer types are template parameters so that the
// kernels can hand in pointers that name the global address space.
#pragma once
#include <stdint.h>

#include "random_walk_step.h"   // DGLA_RW_HD

namespace dgla {

// weight types: the codes of dgla_dtype, then the two integer types (DGLA_TOPK_I32 / DGLA_TOPK_I64 of the header)
enum : int { kTopkF32 = 0, kTopkF64 = 1, kTopkF16 = 2, kTopkBF16 = 3, kTopkI32 = 4, kTopkI64 = 5 };

constexpr int kTopkMaxPicks = 1024;          // the largest number of picks one row may yield
constexpr uint32_t kTopkPad = 0xFFFFFFFFu;   // the position of a padding entry: it loses to every entry of a row

// the key type and the storage word of a weight type
template <int DT>
struct TopkTypes {
  using key = uint32_t;
  using word = uint32_t;
};
template <>
struct TopkTypes<kTopkF64> {
  using key = uint64_t;
  using word = uint64_t;
};
template <>
struct TopkTypes<kTopkI64> {
  using key = uint64_t;
  using word = uint64_t;
};
template <>
struct TopkTypes<kTopkF16> {
  using key = uint32_t;
  using word = uint16_t;
};
template <>
struct TopkTypes<kTopkBF16> {
  using key = uint32_t;
  using word = uint16_t;
};

// the fp32 pattern of an fp16 pattern (exact)
DGLA_RW_HD uint32_t topk_widen_f16(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 31u) return sign | 0x7F800000u | (m << 13);
  if (e == 0u) {
    if (m == 0u) return sign;
    uint32_t s = 0;  // a subnormal: m * 2^-24 = 1.f * 2^(-14 - s)
    while (!(m & 0x400u)) m <<= 1, ++s;
    return sign | ((113u - s) << 23) | ((m & 0x3FFu) << 13);
  }
  return sign | ((e + 112u) << 23) | (m << 13);
}

// the sign-flip map of an fp32 / fp64 pattern; NaN -> 0 after the direction
DGLA_RW_HD uint32_t topk_float_key(uint32_t u, bool ascending) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ascending ? ~key : key;
}
DGLA_RW_HD uint64_t topk_float_key(uint64_t u, bool ascending) {
  if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0u;
  if (u == 0x8000000000000000ull) u = 0u;
  const uint64_t key = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
  return ascending ? ~key : key;
}

// the key of the storage word of a weight
template <int DT>
DGLA_RW_HD typename TopkTypes<DT>::key topk_key(typename TopkTypes<DT>::word w, bool ascending) {
  if constexpr (DT == kTopkF32 || DT == kTopkF64) {
    return topk_float_key(w, ascending);
  } else if constexpr (DT == kTopkF16) {
    return topk_float_key(topk_widen_f16(w), ascending);
  } else if constexpr (DT == kTopkBF16) {
    return topk_float_key(static_cast<uint32_t>(w) << 16, ascending);
  } else if constexpr (DT == kTopkI32) {
    const uint32_t key = w ^ 0x80000000u;
    return ascending ? ~key : key;
  } else {
    const uint64_t key = w ^ 0x8000000000000000ull;
    return ascending ? ~key : key;
  }
}

// the key of edge id e: weight[e] mapped, or 0 for an id outside [0, nnz)
template <int DT, typename WPtr>
DGLA_RW_HD typename TopkTypes<DT>::key topk_edge_key(WPtr weight, int64_t nnz, int64_t e, bool ascending) {
  if (e < 0 || e >= nnz) return 0;
  return topk_key<DT>(weight[e], ascending);
}

// the strict total order: is entry a (key, edge id, position) before entry b?
template <typename K, typename U>
DGLA_RW_HD bool topk_before(K ka, U ea, uint32_t pa, K kb, U eb, uint32_t pb) {
  if (ka != kb) return ka > kb;
  if (ea != eb) return ea < eb;
  return pa < pb;
}

// [lo, hi) of seed i's row, clamped into [0, nnz]; *bad = the seed lies outside [0, num_rows): an empty row
template <typename IndptrPtr, typename SeedPtr>
DGLA_RW_HD void topk_row(IndptrPtr indptr, SeedPtr seeds, int64_t num_rows, int64_t nnz, int64_t i, int64_t* lo, int64_t* hi,
                         bool* bad) {
  const int64_t u = static_cast<int64_t>(seeds[i]);
  *lo = *hi = 0;
  *bad = u < 0 || u >= num_rows;
  if (*bad) return;
  int64_t a = static_cast<int64_t>(indptr[u]), b = static_cast<int64_t>(indptr[u + 1]);
  a = a < 0 ? 0 : (a > nnz ? nnz : a);
  b = b < a ? a : (b > nnz ? nnz : b);
  *lo = a;
  *hi = b;
}

// the number of picks of a row of `deg` entries
DGLA_RW_HD int64_t topk_picks(int64_t deg, int64_t k) { return k < 0 || deg < k ? deg : k; }

// the edge id of entry q
template <typename IdxPtr>
DGLA_RW_HD int64_t topk_eid(IdxPtr data, int64_t q) {
  return data ? static_cast<int64_t>(data[q]) : q;
}

}  // namespace dgla
