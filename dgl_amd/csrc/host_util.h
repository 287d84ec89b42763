// Host-side scaffold of the sampler and sparse units (sampling, random_walk, node2vec, negative_sampling, pinsage,
// csr_mm, coo2csr, labor, knn, matching, subgraph, exclude, traversal, topk): launch geometry, the structural CSR check
// and the typed CSR view, the workspace carver and its two bindings, the read-back, and the id-width and float-type
// dispatches.  fail(msg), align256() and gptr<T> live in common.h, which every unit includes.  Nothing here is device
// code.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/dgl_amd.h"
#include "common.h"

namespace dgla {

// "<who>: <what>" to dgla_last_error(), -1 to the entry point
inline int fail(const char* who, const std::string& what) { return fail(std::string(who) + ": " + what); }

inline bool idbits_ok(int bits) { return bits == 32 || bits == 64; }

// What units differ in when they check a CSR (check_csr below).
enum CsrRule : unsigned {
  kCsrCols = 1u,         // a negative num_cols is refused too
  kCsrEmptyIndptr = 2u,  // a null indptr is accepted when num_rows == 0
  kCsrAnySizes = 4u,     // the sizes are not tested (the unit reads none of them)
  kCsrAnyIndices = 8u,   // a null indices is accepted (the unit does not read it)
};

// The structural check of a dgla_csr, the first thing a unit's own check function calls: nothing is dereferenced but
// the struct, so it refuses before any runtime call.
inline int check_csr(const char* who, const dgla_csr* csr, unsigned rules = 0) {
  if (!csr) return fail(who, "csr is null");
  if (!idbits_ok(csr->idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (!(rules & kCsrAnySizes) && (csr->num_rows < 0 || csr->nnz < 0 || ((rules & kCsrCols) && csr->num_cols < 0)))
    return fail(who, "invalid csr: negative size");
  if (!csr->indptr && !((rules & kCsrEmptyIndptr) && csr->num_rows == 0)) return fail(who, "invalid csr: indptr is null");
  if (!(rules & kCsrAnyIndices) && csr->nnz > 0 && !csr->indices) return fail(who, "invalid csr: indices is null");
  return 0;
}

// The arrays of a checked dgla_csr in the id type of the call, built once per with_idx body.
template <typename Idx>
struct TypedCsr {
  const Idx *indptr, *indices, *data;  // data == nullptr: edge id == position
  int64_t num_rows, num_cols, nnz;
  explicit TypedCsr(const dgla_csr* c)
      : indptr(static_cast<const Idx*>(c->indptr)), indices(static_cast<const Idx*>(c->indices)),
        data(static_cast<const Idx*>(c->data)), num_rows(c->num_rows), num_cols(c->num_cols), nnz(c->nnz) {}
};

// blocks of `per` items over n items, never fewer than one (a launch of zero blocks is an error)
inline unsigned grid1(int64_t n, int per = 256) {
  const int64_t blocks = (n + per - 1) / per;
  return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}

// Lays a workspace out piece by piece, every piece on a 256-byte boundary.  A unit writes ONE layout function around a
// Carver; its *_workspace_bytes query returns that function's bytes() and its run path reads the offsets of the same
// call, so the two cannot disagree.
struct Carver {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += align256(bytes);
    return o;
  }
  size_t bytes() const { return at; }
};

// The one wording of a workspace refusal.
inline int workspace_short(const char* who, size_t need, size_t have) {
  return fail(who, "workspace of " + std::to_string(need) + " bytes required, got " + std::to_string(have));
}

// A REQUIRED workspace: the entry point allocates nothing, so a null or short one is refused.
inline int need_workspace(const char* who, const void* ws, size_t have, size_t need) {
  return !ws || have < need ? workspace_short(who, need, ws ? have : 0) : 0;
}

// An OPTIONAL workspace may be null, and Scratch then serves the call, but not too small.  (The entry points that came
// before this rule, sample_neighbors, to_block, coo_to_csr, csr_mm and csr_sum, never refused a short one: they go
// straight to Scratch::take.)
inline int optional_workspace(const char* who, const void* ws, size_t have, size_t need) {
  return ws && have < need ? workspace_short(who, need, have) : 0;
}

// The caller's workspace when it is large enough, else stream-ordered scratch for the duration of the call.
struct Scratch {
  void* owned = nullptr;
  char* p = nullptr;
  hipStream_t s;
  explicit Scratch(hipStream_t st) : s(st) {}
  int take(void* ws, size_t have, size_t need) {
    if (ws && have >= need) {
      p = static_cast<char*>(ws);
      return 0;
    }
    DGLA_CHECK_HIP(hipMallocAsync(&owned, need, s));
    p = static_cast<char*>(owned);
    return 0;
  }
  ~Scratch() {
    if (owned) (void)hipFreeAsync(owned, s);
  }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
};

// f(Idx{}) with Idx = int32_t or int64_t: the id width of a call, checked by the caller to be 32 or 64
template <typename F>
decltype(auto) with_idx(int bits, F&& f) {
  if (bits == 32) return f(int32_t{});
  return f(int64_t{});
}

// f(T{}) with T = float or double: the float type of a call, checked by the caller to be kF32 or kF64
template <typename F>
decltype(auto) with_float(int dtype, F&& f) {
  if (dtype == kF32) return f(float{});
  return f(double{});
}

// f(W{}, weighted): the type of an optional per-edge weight; a call without one runs the uniform form
template <typename F>
decltype(auto) with_weight(const void* weight, int dtype, F&& f) {
  if (!weight) return f(float{}, std::false_type{});
  if (dtype == kF32) return f(float{}, std::true_type{});
  return f(double{}, std::true_type{});
}

// The device -> host read-back of a call that must know a count before it goes on: the launches so far are checked,
// the bytes copied on the stream, the stream waited for.
inline int read_back(void* dst, const void* src, size_t bytes, hipStream_t s) {
  DGLA_CHECK_HIP(hipGetLastError());
  DGLA_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
  DGLA_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace dgla
