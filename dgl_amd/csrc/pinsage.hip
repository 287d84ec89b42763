// PinSAGE neighbour selection on the device: the visit-count top-k over random-walk traces
// (dgl.sampling.RandomWalkNeighborSampler / PinSAGESampler).
//
// Reference: SelectPinSageNeighbors<kDGLCUDA> (src/graph/sampling/randomwalks/randomwalk_gpu.cu:443 over
// frequency_hashmap.cu: a global hash table filled with atomic inserts, a segmented radix sort, two host
// synchronisations, ties in a run-dependent order) behind python/dgl/sampling/pinsage.py; the rule is the one of its CPU
// form (randomwalk_cpu.cc:41-102).
//
// The rule (quoted in include/dgl_amd.h): segment j = src[j*S .. (j+1)*S) without its -1 entries; its distinct ids are
// ranked by (visit count, id), both descending; the first min(k, distinct) are kept and emitted as (id, dst[j*S], count),
// segments in the order of j.  Ids are compared as UNSIGNED words, so that -1 (all ones) sorts behind every id.
//
// MI355X-first choices:
//  * A segment is small (walks x traversals ids), so one workgroup owns it and the whole selection happens in LDS: no
//    atomics, no global scratch that grows with num_dst * S, the same bits on every run.
//  * ONE key array.  The ids are sorted ascending (a bitonic network on the bare ids: equal keys are indistinguishable,
//    so the result is the same whatever the network does with them).  The heads of the runs of equal ids are then
//    numbered in position order; since the ids ascend, "larger id" is "later head", so ranking the runs by
//    (count, id) descending is sorting the 32-bit words  count << 16 | head position  descending.  An id is never
//    packed into a key, so every bit of an int64 id survives; count and position are below 2^16 by the limit on S.
//  * Size classes over S (dgla_pinsage_size_classes), one launch per call since S is the same for every segment:
//    S <= kWaveMax one wavefront per segment, S <= kBlockMax a 256-thread workgroup, S <= kMaxSamples a 512-thread one.
//    The networks run over the next power of two of S (and of the number of runs), not over the class capacity.
//  * The kernel writes a PADDED result ([num_dst, min(k, S)] with -1 / 0 in the unused slots, and the number kept per
//    segment): a static shape.  The compact form is an exclusive scan of those numbers (csrc/sort.hip.h), one read of
//    the total by the host (the reference synchronises here too) and a compaction kernel.
#include "../../include/dgl_amd.h"

#include <algorithm>
#include <vector>

#include "host_util.h"
#include "sort.hip.h"

namespace dgla {
namespace pinsage {

constexpr int kWaveMax = 64;        // samples of a segment handled by one wavefront
constexpr int kBlockMax = 1024;     // ... by one 256-thread workgroup
constexpr int kMaxSamples = 4096;   // ... by one 512-thread workgroup: the largest accepted S (48 KiB of LDS with int64 ids)

template <typename Idx>
struct Unsigned {
  using type = uint32_t;
};
template <>
struct Unsigned<int64_t> {
  using type = uint64_t;
};

// Bitonic network over the n2 (a power of two) keys of `a` in LDS, ascending or descending; thread t takes the compare
// pairs t, t + NT, ...  Equal keys are never exchanged.  Every stage ends in a barrier.
template <typename K, bool DESC, int NT>
__device__ __forceinline__ void bitonic_sort(K* a, int n2, int tid) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const K x = a[i], y = a[l];
        const bool up = ((i & k) == 0) != DESC;   // this pair's direction in the network
        if (up ? x > y : x < y) {
          a[i] = y;
          a[l] = x;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// One workgroup of NT threads per segment of S <= CAP samples.  kp = min(k, S) slots per segment in out_src / out_cnt.
template <typename Idx, int NT, int CAP>
__global__ __launch_bounds__(NT) void pinsage_select_kernel(const Idx* __restrict__ src, const Idx* __restrict__ dst, int S,
                                                           int kp, Idx* __restrict__ out_src, Idx* __restrict__ out_cnt,
                                                           Idx* __restrict__ out_num, Idx* __restrict__ out_dst) {
  using U = typename Unsigned<Idx>::type;
  static_assert(CAP <= 32768 && CAP % NT == 0, "count and head position share a 32-bit word");
  constexpr U kNone = ~U(0);            // -1, and the padding: behind every id
  __shared__ U key[CAP];                // the segment's ids, then sorted ascending
  __shared__ uint32_t run[CAP + 1];     // head positions of the runs, then count << 16 | head position
  __shared__ int wsum[NT / 64];
  const int64_t j = blockIdx.x;         // 64-bit offsets: num_dst * S may pass 2^31
  const int tid = threadIdx.x;
  const int n2 = pow2_at_least(S);
  const Idx* seg = src + j * S;
  for (int i = tid; i < n2; i += NT) key[i] = i < S ? static_cast<U>(seg[i]) : kNone;
  __syncthreads();
  bitonic_sort<U, false, NT>(key, n2, tid);
  // heads of the runs of equal keys, numbered in position order; thread t owns the consecutive slots [s0, s1).  The run
  // of kNone (if any) is numbered too: it is the last one, and its head is the number of valid samples.
  const int per = (n2 + NT - 1) / NT;
  const int s0 = tid * per, s1 = s0 + per < n2 ? s0 + per : n2;
  int heads = 0;
  for (int s = s0; s < s1; ++s) heads += (s == 0 || key[s] != key[s - 1]) ? 1 : 0;
  int total;
  int at = msd::block_exclusive_scan<NT>(heads, &total, wsum);
  for (int s = s0; s < s1; ++s)
    if (s == 0 || key[s] != key[s - 1]) run[at++] = static_cast<uint32_t>(s);
  if (tid == 0) run[total] = static_cast<uint32_t>(n2);
  __syncthreads();
  const int m = total - (key[n2 - 1] == kNone ? 1 : 0);   // distinct ids
  const int m2 = pow2_at_least(m);
  // run p = [run[p], run[p + 1]): read every pair before any slot is overwritten
  constexpr int PER = CAP / NT;
  uint32_t packed[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = tid + i * NT;
    packed[i] = p < m ? ((run[p + 1] - run[p]) << 16) | run[p] : 0u;   // 0 sorts behind every run (count >= 1)
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = tid + i * NT;
    if (p < m2) run[p] = packed[i];
  }
  __syncthreads();
  bitonic_sort<uint32_t, true, NT>(run, m2, tid);
  const int take = kp < m ? kp : m;
  Idx* o_src = out_src + j * kp;
  Idx* o_cnt = out_cnt + j * kp;
  for (int i = tid; i < kp; i += NT) {
    const uint32_t w = i < take ? run[i] : 0u;
    o_src[i] = i < take ? static_cast<Idx>(key[w & 0xffffu]) : static_cast<Idx>(-1);
    o_cnt[i] = static_cast<Idx>(w >> 16);
  }
  if (tid == 0) {
    out_num[j] = static_cast<Idx>(take);
    if (out_dst) out_dst[j] = dst[j * S];   // the one read of dst for this segment
  }
}

// slot i of segment j goes to off[j] + i when i < num[j]; one thread per slot of the padded result
template <typename Idx>
__global__ __launch_bounds__(256) void pinsage_compact_kernel(const Idx* __restrict__ p_src, const Idx* __restrict__ p_cnt,
                                                             const Idx* __restrict__ p_num, const Idx* __restrict__ p_dst,
                                                             const int64_t* __restrict__ off, int64_t num_dst, int kp,
                                                             Idx* __restrict__ res_src, Idx* __restrict__ res_dst,
                                                             Idx* __restrict__ res_cnt) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= num_dst * kp) return;
  const int64_t j = idx / kp;
  const int i = static_cast<int>(idx - j * kp);
  if (i >= static_cast<int>(p_num[j])) return;
  const int64_t o = off[j] + i;
  res_src[o] = p_src[idx];
  res_dst[o] = p_dst[j];
  res_cnt[o] = p_cnt[idx];
}

// ---- host side ------------------------------------------------------------------------------------------------------
// what every entry point refuses; *kp = min(k, S)
int check_args(const char* who, int idtype_bits, int64_t num_dst, int64_t S, int64_t k, bool device, int64_t* kp) {
  if (!idbits_ok(idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (num_dst < 0) return fail(who, "negative number of segments");
  if (S < 1) return fail(who, "num_samples_per_node must be at least 1, got " + std::to_string(S));
  if (k < 1) return fail(who, "k must be at least 1, got " + std::to_string(k));
  if (device && S > kMaxSamples)
    return fail(who, "num_samples_per_node = " + std::to_string(S) + " is above the largest segment the kernel holds in LDS (" +
                         std::to_string(kMaxSamples) + ", dgla_pinsage_max_samples); there is no CPU fallback");
  if (device && num_dst > 0x7fffffffLL) return fail(who, "more than 2^31 - 1 segments in one call");
  *kp = k < S ? k : S;
  return 0;
}

template <typename Idx>
int launch_select(const void* src, const void* dst, int64_t num_dst, int64_t S, int64_t kp, void* out_src, void* out_cnt,
                  void* out_num, void* out_dst, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(num_dst));
#define DGLA_PINSAGE(NT, CAP)                                                                                          \
  hipLaunchKernelGGL((pinsage_select_kernel<Idx, NT, CAP>), grid, dim3(NT), 0, s, static_cast<const Idx*>(src),          \
                     static_cast<const Idx*>(dst), static_cast<int>(S), static_cast<int>(kp), static_cast<Idx*>(out_src), \
                     static_cast<Idx*>(out_cnt), static_cast<Idx*>(out_num), static_cast<Idx*>(out_dst))
  if (S <= kWaveMax) DGLA_PINSAGE(64, kWaveMax);
  else if (S <= kBlockMax) DGLA_PINSAGE(256, kBlockMax);
  else DGLA_PINSAGE(512, kMaxSamples);
#undef DGLA_PINSAGE
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

// workspace of the compact form: the padded result, the segments' dst, the offsets and the scan's temporary
struct Layout {
  size_t off_src, off_cnt, off_num, off_dst, off_off, off_scan, bytes;
};
Layout make_layout(int idtype_bits, int64_t num_dst, int64_t kp) {
  const size_t i = idtype_bits / 8, n = static_cast<size_t>(num_dst), slots = n * static_cast<size_t>(kp);
  Layout l;
  Carver c;
  l.off_src = c.take(slots * i);
  l.off_cnt = c.take(slots * i);
  l.off_num = c.take(n * i);
  l.off_dst = c.take(n * i);
  l.off_off = c.take(n * sizeof(int64_t));
  l.off_scan = c.take(msd::scan_temp_bytes(num_dst, sizeof(int64_t)));
  l.bytes = c.bytes();
  return l;
}

template <typename Idx>
int count_compact(const void* src, const void* dst, int64_t num_dst, int64_t S, int64_t kp, int64_t* total_out, char* ws,
                  const Layout& l, hipStream_t s) {
  Idx* num = reinterpret_cast<Idx*>(ws + l.off_num);
  int64_t* off = reinterpret_cast<int64_t*>(ws + l.off_off);
  if (launch_select<Idx>(src, dst, num_dst, S, kp, ws + l.off_src, ws + l.off_cnt, num, ws + l.off_dst, s)) return -1;
  if (msd::exclusive_scan<Idx, int64_t>(num, off, num_dst, ws + l.off_scan, s)) return -1;
  int64_t last_off = 0;
  Idx last_num = 0;
  if (read_back(&last_off, off + num_dst - 1, sizeof(int64_t), s) || read_back(&last_num, num + num_dst - 1, sizeof(Idx), s))
    return -1;
  *total_out = last_off + static_cast<int64_t>(last_num);
  return 0;
}

template <typename Idx>
int fill_compact(int64_t num_dst, int64_t kp, void* res_src, void* res_dst, void* res_cnt, const char* ws, const Layout& l,
                 hipStream_t s) {
  const int64_t slots = num_dst * kp;
  hipLaunchKernelGGL(pinsage_compact_kernel<Idx>, dim3(static_cast<unsigned>((slots + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const Idx*>(ws + l.off_src), reinterpret_cast<const Idx*>(ws + l.off_cnt),
                     reinterpret_cast<const Idx*>(ws + l.off_num), reinterpret_cast<const Idx*>(ws + l.off_dst),
                     reinterpret_cast<const int64_t*>(ws + l.off_off), num_dst, static_cast<int>(kp),
                     static_cast<Idx*>(res_src), static_cast<Idx*>(res_dst), static_cast<Idx*>(res_cnt));
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

// the rule on the host: sort the segment's ids, take run lengths, order the (count, id) pairs
template <typename Idx>
int64_t select_host(const Idx* src, const Idx* dst, int64_t num_dst, int64_t S, int64_t kp, Idx* res_src, Idx* res_dst,
                    Idx* res_cnt) {
  using U = typename Unsigned<Idx>::type;
  const U none = ~U(0);
  std::vector<U> ids(static_cast<size_t>(S));
  std::vector<std::pair<int64_t, U>> pairs;   // (count, id)
  int64_t out = 0;
  for (int64_t j = 0; j < num_dst; ++j) {
    for (int64_t i = 0; i < S; ++i) ids[i] = static_cast<U>(src[j * S + i]);
    std::sort(ids.begin(), ids.end());
    pairs.clear();
    for (int64_t i = 0; i < S && ids[i] != none;) {
      int64_t e = i + 1;
      while (e < S && ids[e] == ids[i]) ++e;
      pairs.emplace_back(e - i, ids[i]);
      i = e;
    }
    std::sort(pairs.begin(), pairs.end(), [](const auto& a, const auto& b) { return a > b; });
    const int64_t take = std::min<int64_t>(kp, static_cast<int64_t>(pairs.size()));
    for (int64_t i = 0; i < take; ++i, ++out) {
      res_src[out] = static_cast<Idx>(pairs[i].second);
      res_dst[out] = dst[j * S];
      res_cnt[out] = static_cast<Idx>(pairs[i].first);
    }
  }
  return out;
}

}  // namespace pinsage
}  // namespace dgla

using namespace dgla;
using namespace dgla::pinsage;

extern "C" {

int64_t dgla_pinsage_max_samples(int idtype_bits) {
  return idbits_ok(idtype_bits) ? kMaxSamples : 0;
}

int dgla_pinsage_size_classes(int64_t* bounds, int max) {
  const int64_t b[3] = {kWaveMax, kBlockMax, kMaxSamples};
  for (int i = 0; i < 3 && i < max; ++i) bounds[i] = b[i];
  return 3;
}

int dgla_pinsage_select_padded(int idtype_bits, const void* src, const void* dst, int64_t num_dst,
                               int64_t num_samples_per_node, int64_t k, void* out_src, void* out_cnt, void* out_num,
                               void* out_dst, void* hip_stream) {
  int64_t kp = 0;
  const char* who = "pinsage_select_padded";
  if (check_args(who, idtype_bits, num_dst, num_samples_per_node, k, true, &kp)) return -1;
  if (num_dst == 0) return 0;
  if (!src || !out_src || !out_cnt || !out_num) return fail(who, "src / out_src / out_cnt / out_num are null");
  if (out_dst && !dst) return fail(who, "out_dst asked for without dst");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out_src);
  return with_idx(idtype_bits, [&](auto tag) {
    return launch_select<decltype(tag)>(src, dst, num_dst, num_samples_per_node, kp, out_src, out_cnt, out_num, out_dst, s);
  });
}

size_t dgla_pinsage_select_workspace_bytes(int idtype_bits, int64_t num_dst, int64_t num_samples_per_node, int64_t k) {
  int64_t kp = 0;
  if (check_args("pinsage_select_workspace_bytes", idtype_bits, num_dst, num_samples_per_node, k, true, &kp)) return 0;
  return make_layout(idtype_bits, num_dst, kp).bytes;
}

int dgla_pinsage_select_count(int idtype_bits, const void* src, const void* dst, int64_t num_dst,
                              int64_t num_samples_per_node, int64_t k, int64_t* total_out, void* workspace,
                              size_t workspace_bytes, void* hip_stream) {
  int64_t kp = 0;
  const char* who = "pinsage_select_count";
  if (check_args(who, idtype_bits, num_dst, num_samples_per_node, k, true, &kp)) return -1;
  if (!total_out) return fail(who, "total_out is null");
  *total_out = 0;
  if (num_dst == 0) return 0;
  if (!src || !dst) return fail(who, "src / dst are null");
  const Layout l = make_layout(idtype_bits, num_dst, kp);
  if (need_workspace(who, workspace, workspace_bytes, l.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, workspace);
  char* ws = static_cast<char*>(workspace);
  return with_idx(idtype_bits, [&](auto tag) {
    return count_compact<decltype(tag)>(src, dst, num_dst, num_samples_per_node, kp, total_out, ws, l, s);
  });
}

int dgla_pinsage_select_fill(int idtype_bits, int64_t num_dst, int64_t num_samples_per_node, int64_t k, void* res_src,
                             void* res_dst, void* res_cnt, const void* workspace, size_t workspace_bytes,
                             void* hip_stream) {
  int64_t kp = 0;
  const char* who = "pinsage_select_fill";
  if (check_args(who, idtype_bits, num_dst, num_samples_per_node, k, true, &kp)) return -1;
  if (num_dst == 0) return 0;
  const Layout l = make_layout(idtype_bits, num_dst, kp);
  if (need_workspace(who, workspace, workspace_bytes, l.bytes)) return -1;
  // (a total of 0 leaves the result arrays empty, possibly null: the kernel then stores nothing)
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, workspace);
  const char* ws = static_cast<const char*>(workspace);
  return with_idx(idtype_bits, [&](auto tag) {
    return fill_compact<decltype(tag)>(num_dst, kp, res_src, res_dst, res_cnt, ws, l, s);
  });
}

int dgla_pinsage_select_host(int idtype_bits, const void* src, const void* dst, int64_t num_dst,
                             int64_t num_samples_per_node, int64_t k, void* res_src, void* res_dst, void* res_cnt,
                             int64_t* total_out) {
  int64_t kp = 0;
  const char* who = "pinsage_select_host";
  if (check_args(who, idtype_bits, num_dst, num_samples_per_node, k, false, &kp)) return -1;
  if (!total_out) return fail(who, "total_out is null");
  *total_out = 0;
  if (num_dst == 0) return 0;
  if (!src || !dst || !res_src || !res_dst || !res_cnt) return fail(who, "a null array");
  *total_out = with_idx(idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    return select_host<Idx>(static_cast<const Idx*>(src), static_cast<const Idx*>(dst), num_dst, num_samples_per_node, kp,
                            static_cast<Idx*>(res_src), static_cast<Idx*>(res_dst), static_cast<Idx*>(res_cnt));
  });
  return 0;
}

}  // extern "C"
