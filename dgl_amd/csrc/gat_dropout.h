// The keep rule of attention dropout in the fused GAT operator (include/dgl_amd.h, "Training form"): ONE definition,
// compiled for the host (dgla_gat_dropout_mask_host) and for the device (csrc/gat_attention_train.hip).
//
//   w    = Philox4x32-10(key = seed, counter = (eid low 32, eid high 32, head / 4, 0))[head % 4]
//   keep = (w >> 8) >= threshold,  threshold = (uint32_t)(p * 16777216.0)
//
// Philox4x32-10: Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11 (the counter-based
// generator of Random123, cuRAND / rocRAND and torch).  Integer arithmetic only, so host and device agree bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DGLA_GAT_HD __host__ __device__ inline
#else
#define DGLA_GAT_HD inline
#endif

namespace dgla {

// the four words of the block that holds heads 4 * block .. 4 * block + 3 of edge `eid`
DGLA_GAT_HD void gat_philox4(uint64_t seed, uint64_t eid, uint32_t block, uint32_t (&w)[4]) {
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  uint32_t c0 = static_cast<uint32_t>(eid), c1 = static_cast<uint32_t>(eid >> 32), c2 = block, c3 = 0u;
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

DGLA_GAT_HD bool gat_keep_word(uint32_t word, uint32_t threshold) { return (word >> 8) >= threshold; }

DGLA_GAT_HD bool gat_keep(uint64_t seed, uint64_t eid, int head, uint32_t threshold) {
  uint32_t w[4];
  gat_philox4(seed, eid, static_cast<uint32_t>(head) >> 2, w);
  const int i = head & 3;
  return gat_keep_word(i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3], threshold);
}

// threshold and the scale 1 / (1 - p) of the kept weights, computed ONCE on the host; false when p is not in [0, 1).
// A p below 2^-24 has threshold 0: nothing can be dropped, the kernels skip the generator and the scale is exactly 1.
inline bool gat_dropout_params(float p, uint32_t* threshold, float* scale) {
  if (!(p >= 0.f && p < 1.f)) return false;
  *threshold = static_cast<uint32_t>(static_cast<double>(p) * 16777216.0);
  *scale = *threshold == 0 ? 1.0f : 1.0f / (1.0f - p);
  return true;
}

}  // namespace dgla
