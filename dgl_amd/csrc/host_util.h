// Host-side scaffold of the sampler and sparse units (sampling, random_walk, node2vec, negative_sampling, pinsage,
// csr_mm, coo2csr): launch geometry, the workspace carver and the id-width dispatch.  fail(), align256() and gptr<T>
// live in common.h, which every unit includes.  Nothing here is device code.
#pragma once
#include <stdint.h>

#include "common.h"

namespace dgla {

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

}  // namespace dgla
