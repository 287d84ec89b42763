// Random walks on the device: metapath, weighted and restart forms (dgl.sampling.random_walk).
//
// Reference: RandomWalk<kDGLCUDA> (src/graph/sampling/randomwalks/randomwalk_gpu.cu: one thread per walk, a
// curand state seeded with seed + thread id, a linear scan of the row's probabilities in the weighted step) behind
// python/dgl/sampling/randomwalks.py:31-226.
//
// MI355X-first choices:
//  * The picks are a pure function of (rng_seed, walk index, step, draw slot) — the counter-based generator
//    csrc/sampling.hip draws from too — so a run is reproducible from its seed whatever the launch geometry, and the host walker
//    (dgla_random_walk_host) that shares csrc/random_walk_step.h with the kernel reproduces it bit for bit.
//  * The weighted step is a bisection in a per-relation CDF built once (walk_cdf_kernel): O(log deg) dependent loads per
//    visit of a 17 000-edge hub row instead of 17 000.
//  * A uniform step is two dependent loads (the indptr pair, then indices[pos] together with data[pos]); one lane per
//    walk, no LDS, few registers: occupancy hides the latency.  The relation table and the metapath travel in the
//    kernel arguments (scalar loads, uniform over the wavefront) while they fit, else in `workspace`.
#include "../../include/dgl_amd.h"

#include <cstring>
#include <vector>

#include "host_util.h"
#include "random_walk_step.h"

namespace dgla {
namespace {

// ---- the walk ---------------------------------------------------------------------------------
template <typename Idx>
struct WalkRel {  // one relation of the table: 5 words
  const Idx* indptr;
  const Idx* indices;
  const Idx* data;    // edge-id map or NULL
  const double* cdf;  // NULL = uniform
  int64_t num_rows;
};
static_assert(sizeof(WalkRel<int32_t>) == 40 && sizeof(WalkRel<int64_t>) == 40, "WalkRel is 5 words");

// What travels by value in the kernel arguments: up to kArgRels relations and up to kArgSteps metapath entries (one
// byte each) — 896 bytes.  Anything larger is read from `workspace`.
constexpr int kArgRels = 16;
constexpr int kArgSteps = 256;
template <typename Idx>
struct WalkTable {
  WalkRel<Idx> rel[kArgRels];
  uint32_t path[kArgSteps / 4];  // four entries per word: a scalar load fetches words, not bytes
};

// (one switch for both: a call whose table or metapath does not fit reads both from `workspace`)
bool walk_in_args(int num_rels, int64_t num_steps) { return num_rels <= kArgRels && num_steps <= kArgSteps; }

struct WalkLayout {  // offsets into the workspace of dgla_random_walk; bytes == 0: everything travels in the arguments
  size_t table = 0, path = 0, bytes = 0;
};
WalkLayout walk_layout(int num_rels, int64_t num_steps) {
  WalkLayout L;
  if (walk_in_args(num_rels, num_steps)) return L;
  Carver c;
  L.table = c.take(sizeof(WalkRel<int64_t>) * static_cast<size_t>(num_rels));
  L.path = c.take(sizeof(int32_t) * static_cast<size_t>(num_steps));
  L.bytes = c.bytes();
  return L;
}

// WS: the table and the metapath come from `workspace` (ws_rel / ws_path) instead of the kernel arguments — a
// compile-time switch, so that either form reads them with scalar loads (a run-time choice between the two address
// spaces made the compiler fetch the table through flat vector loads, one more dependent load per step).
template <typename Idx, bool WS>
__global__ __launch_bounds__(256) void random_walk_kernel(const WalkTable<Idx> tab, const WalkRel<Idx>* __restrict__ ws_rel,
                                                          const int32_t* __restrict__ ws_path, int64_t num_steps,
                                                          const Idx* __restrict__ seeds, int64_t num_seeds,
                                                          double restart_prob, const void* __restrict__ restart_steps,
                                                          int restart_f32, uint64_t rng_seed, Idx* __restrict__ traces,
                                                          Idx* __restrict__ eids) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (i >= num_seeds) return;
  // uniform over the wavefront: scalar loads from the kernel arguments, or from the table in `workspace`
  struct GRel {
    gptr<Idx> indptr, indices, data;
    gptr<double> cdf;
    int64_t num_rows;
  };
  auto rel_at = [&](int64_t t) {
    const int m = WS ? ws_path[t] : static_cast<int>((tab.path[t >> 2] >> ((t & 3) * 8)) & 0xffu);
    const WalkRel<Idx> R = WS ? ws_rel[m] : tab.rel[m];
    return GRel{(gptr<Idx>)R.indptr, (gptr<Idx>)R.indices, (gptr<Idx>)R.data, (gptr<double>)R.cdf, R.num_rows};
  };
  auto p_at = [&](int64_t t) {
    if (!restart_steps) return restart_prob;
    return restart_f32 ? static_cast<double>(static_cast<const float*>(restart_steps)[t])
                       : static_cast<const double*>(restart_steps)[t];
  };
  // 64-bit offsets: num_seeds * (num_steps + 1) may pass 2^31
  rw_walk<Idx>(rel_at, p_at, num_steps, rng_seed, i, seeds[i], traces + i * (num_steps + 1),
               eids ? eids + i * num_steps : nullptr);
}

// Writes up to 64 words that arrived in the kernel arguments to `dst`: how the relation table and the metapath
// reach `workspace` without a copy engine, a staging buffer or a synchronisation (and inside a captured stream).
struct UploadWords {
  uint64_t w[64];
};
__global__ __launch_bounds__(64) void walk_upload_kernel(const UploadWords v, uint64_t* __restrict__ dst, int n) {
  const int k = threadIdx.x;
  if (k < n) dst[k] = v.w[k];
}

int upload_words(const uint64_t* words, int64_t n, void* dst, hipStream_t s) {
  for (int64_t done = 0; done < n; done += 64) {
    UploadWords v;
    const int c = static_cast<int>(n - done < 64 ? n - done : 64);
    std::memset(&v, 0, sizeof(v));
    std::memcpy(v.w, words + done, sizeof(uint64_t) * c);
    hipLaunchKernelGGL(walk_upload_kernel, dim3(1), dim3(64), 0, s, v, static_cast<uint64_t*>(dst) + done, c);
  }
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- the CDF ----------------------------------------------------------------------------------
// cdf[pos] = fl(c + l): l is the running sum of the lane's own consecutive positions (added in order), c the LAST
// INCLUSIVE VALUE in front of them.  fl(c + l) never decreases while l does not, a zero weight leaves l — and so the
// value — unchanged, and at a seam the next c IS the previous value; both exact properties of the rule hold whatever
// the weights.  (A carry obtained by a separate reduction would differ from the value in front of it by a rounding.)
//  * rows shorter than kCdfLong: one LANE per row, a plain running sum — a launch over many short rows does not spend a
//    wavefront per row;
//  * longer rows: the WAVEFRONT takes them one after the other (ballot), kCdfK consecutive positions per lane and tile of
//    64 * kCdfK; the carries c of the 64 lanes are chained through lane reads: 64 dependent adds per 512 positions, so a
//    17 000-edge hub row is 34 tiles, not 17 000 dependent iterations.
// No atomics of any kind: the same bits on every run.
constexpr int kCdfLong = 64;
constexpr int kCdfK = 8;

template <typename Idx, typename W>
__global__ __launch_bounds__(256) void walk_cdf_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ data,
                                                       const W* __restrict__ prob, int64_t num_rows,
                                                       double* __restrict__ cdf) {
  const int64_t row = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = 0;
  if (row < num_rows) {
    lo = static_cast<int64_t>(indptr[row]);
    hi = static_cast<int64_t>(indptr[row + 1]);
  }
  auto weight = [&](int64_t q) { return rw_weight(prob[data ? static_cast<int64_t>(data[q]) : q]); };
  const bool is_long = hi - lo >= kCdfLong;
  if (!is_long) {
    double run = 0.0;
    for (int64_t q = lo; q < hi; ++q) {
      run += weight(q);
      cdf[q] = run;
    }
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int src = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1;
    const int64_t rlo = __shfl(lo, src, 64), rhi = __shfl(hi, src, 64);
    double carry = 0.0;  // the last inclusive value so far (the same in every lane)
    for (int64_t base = rlo; base < rhi; base += 64 * kCdfK) {
      const int64_t q0 = base + static_cast<int64_t>(lane) * kCdfK;
      double l[kCdfK];
      // the tile's loads first, all in flight together (positions past the row read its last edge and count as 0)
#pragma unroll
      for (int j = 0; j < kCdfK; ++j) l[j] = weight(q0 + j < rhi ? q0 + j : rhi - 1);
      double run = 0.0;
#pragma unroll
      for (int j = 0; j < kCdfK; ++j) {
        run += q0 + j < rhi ? l[j] : 0.0;
        l[j] = run;
      }
      double c = carry, mine = carry;
#pragma unroll
      for (int k = 0; k < 64; ++k) {
        if (lane == k) mine = c;
        c = c + __shfl(run, k, 64);
      }
      carry = c;
#pragma unroll
      for (int j = 0; j < kCdfK; ++j)
        if (q0 + j < rhi) cdf[q0 + j] = mine + l[j];
    }
  }
}

// ---- host side --------------------------------------------------------------------------------
// everything both entry points refuse; *idbits receives the id width of the table
int check_walk(const char* who, const dgla_walk_relation* rels, int num_rels, const int32_t* metapath, int64_t num_steps,
               const void* seeds, int64_t num_seeds, const void* restart_steps, dgla_dtype restart_dtype,
               const void* traces, int* idbits) {
  if (!rels || num_rels < 1) return fail(who, "the relation table is null or empty");
  if (num_steps < 0 || num_seeds < 0) return fail(who, "negative number of steps / seeds");
  for (int r = 0; r < num_rels; ++r) {
    if (check_csr((std::string(who) + ": relation " + std::to_string(r)).c_str(), rels[r].csr)) return -1;
    if (rels[r].csr->idtype_bits != rels[0].csr->idtype_bits) return fail(who, "the relations have mixed id widths");
  }
  if (num_steps > 0 && !metapath) return fail(who, "metapath is null");
  for (int64_t t = 0; t < num_steps; ++t) {
    if (metapath[t] < 0 || metapath[t] >= num_rels)
      return fail(who, "metapath[" + std::to_string(t) + "] = " + std::to_string(metapath[t]) + " is out of range");
    if (t > 0 && rels[metapath[t - 1]].csr->num_cols != rels[metapath[t]].csr->num_rows)
      return fail(who, "the metapath does not chain at step " + std::to_string(t) + ": relation " +
                           std::to_string(metapath[t - 1]) + " ends in " + std::to_string(rels[metapath[t - 1]].csr->num_cols) +
                           " nodes, relation " + std::to_string(metapath[t]) + " starts from " +
                           std::to_string(rels[metapath[t]].csr->num_rows));
  }
  if (restart_steps && restart_dtype != DGLA_F32 && restart_dtype != DGLA_F64)
    return fail(who, "restart_steps must be float32 or float64");
  if (num_seeds > 0 && (!seeds || !traces)) return fail(who, "seeds / traces are null");
  *idbits = rels[0].csr->idtype_bits;
  return 0;
}

template <typename Idx>
WalkRel<Idx> make_rel(const dgla_walk_relation& r) {
  const TypedCsr<Idx> g(r.csr);
  return WalkRel<Idx>{g.indptr, g.indices, g.data, r.cdf, g.num_rows};
}

template <typename Idx>
int run_walk(const dgla_walk_relation* rels, int num_rels, const int32_t* metapath, int64_t num_steps, const void* seeds,
             int64_t num_seeds, double restart_prob, const void* restart_steps, dgla_dtype restart_dtype, uint64_t rng_seed,
             void* traces, void* eids, char* ws, const WalkLayout& L, hipStream_t s) {
  WalkTable<Idx> tab;
  std::memset(&tab, 0, sizeof(tab));
  const WalkRel<Idx>* ws_rel = nullptr;
  const int32_t* ws_path = nullptr;
  const bool in_args = L.bytes == 0;
  if (in_args) {
    for (int r = 0; r < num_rels; ++r) tab.rel[r] = make_rel<Idx>(rels[r]);
    for (int64_t t = 0; t < num_steps; ++t) tab.path[t >> 2] |= static_cast<uint32_t>(metapath[t]) << ((t & 3) * 8);
  } else {
    std::vector<uint64_t> words(static_cast<size_t>(num_rels) * 5);
    for (int r = 0; r < num_rels; ++r) {
      const WalkRel<Idx> v = make_rel<Idx>(rels[r]);
      std::memcpy(&words[static_cast<size_t>(r) * 5], &v, sizeof(v));
    }
    if (upload_words(words.data(), static_cast<int64_t>(words.size()), ws + L.table, s)) return -1;
    ws_rel = reinterpret_cast<const WalkRel<Idx>*>(ws + L.table);
    char* dst = ws + L.path;
    words.assign(static_cast<size_t>((num_steps + 1) / 2), 0);
    std::memcpy(words.data(), metapath, sizeof(int32_t) * static_cast<size_t>(num_steps));
    if (upload_words(words.data(), static_cast<int64_t>(words.size()), dst, s)) return -1;
    ws_path = reinterpret_cast<const int32_t*>(dst);
  }
#define DGLA_WALK(WS)                                                                                              \
  hipLaunchKernelGGL((random_walk_kernel<Idx, WS>), dim3(grid1(num_seeds)), dim3(256), 0, s, tab, ws_rel, ws_path, \
                     num_steps, static_cast<const Idx*>(seeds), num_seeds, restart_prob, restart_steps,            \
                     restart_dtype == DGLA_F32 ? 1 : 0, rng_seed, static_cast<Idx*>(traces), static_cast<Idx*>(eids))
  if (in_args) DGLA_WALK(false); else DGLA_WALK(true);
#undef DGLA_WALK
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

// the kernel's walk on the host, through the same rw_walk
template <typename Idx>
void walk_host(const dgla_walk_relation* rels, const int32_t* metapath, int64_t num_steps, const void* seeds_v,
               int64_t num_seeds, double restart_prob, const void* restart_steps, dgla_dtype restart_dtype,
               uint64_t rng_seed, void* traces_v, void* eids_v) {
  const Idx* seeds = static_cast<const Idx*>(seeds_v);
  Idx *traces = static_cast<Idx*>(traces_v), *eids = static_cast<Idx*>(eids_v);
  auto rel_at = [&](int64_t t) { return make_rel<Idx>(rels[metapath[t]]); };
  auto p_at = [&](int64_t t) {
    if (!restart_steps) return restart_prob;
    return restart_dtype == DGLA_F32 ? static_cast<double>(static_cast<const float*>(restart_steps)[t])
                                     : static_cast<const double*>(restart_steps)[t];
  };
  for (int64_t i = 0; i < num_seeds; ++i)
    rw_walk<Idx>(rel_at, p_at, num_steps, rng_seed, i, seeds[i], traces + i * (num_steps + 1),
                 eids ? eids + i * num_steps : nullptr);
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_random_walk_cdf_workspace_bytes(const dgla_csr* csr) {
  (void)csr;
  return 0;  // the scan is one pass with its carries in registers
}

int dgla_random_walk_cdf(const dgla_csr* csr, const void* prob, dgla_dtype prob_dtype, double* cdf, void* workspace,
                         size_t workspace_bytes, void* hip_stream) {
  (void)workspace;
  const char* who = "random_walk_cdf";
  if (check_csr(who, csr, kCsrAnyIndices)) return -1;  // (the scan reads indptr and data, never indices)
  if (prob_dtype != DGLA_F32 && prob_dtype != DGLA_F64) return fail(who, "prob must be float32 or float64");
  if (csr->nnz > 0 && (!prob || !cdf)) return fail(who, "prob / cdf are null");
  if (workspace_bytes < dgla_random_walk_cdf_workspace_bytes(csr)) return fail(who, "workspace too small");
  if (csr->nnz == 0 || csr->num_rows == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, cdf);
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    with_float(prob_dtype, [&](auto w) {
      using W = decltype(w);
      hipLaunchKernelGGL((walk_cdf_kernel<Idx, W>), dim3(grid1(g.num_rows)), dim3(256), 0, s, g.indptr, g.data,
                         static_cast<const W*>(prob), g.num_rows, cdf);
    });
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

size_t dgla_random_walk_workspace_bytes(int num_rels, int64_t num_steps) {
  if (num_rels < 0 || num_steps < 0) return 0;
  return walk_layout(num_rels, num_steps).bytes;
}

int dgla_random_walk(const dgla_walk_relation* rels, int num_rels, const int32_t* metapath, int64_t num_steps,
                     const void* seeds, int64_t num_seeds, double restart_prob, const void* restart_steps,
                     dgla_dtype restart_dtype, uint64_t rng_seed, void* traces, void* eids, void* workspace,
                     size_t workspace_bytes, void* hip_stream) {
  int idbits = 0;
  const char* who = "random_walk";
  if (check_walk(who, rels, num_rels, metapath, num_steps, seeds, num_seeds, restart_steps, restart_dtype, traces, &idbits))
    return -1;
  const WalkLayout L = walk_layout(num_rels, num_steps);
  if (L.bytes > 0 && need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  if (num_seeds == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, traces);
  char* ws = static_cast<char*>(workspace);
  return with_idx(idbits, [&](auto tag) {
    return run_walk<decltype(tag)>(rels, num_rels, metapath, num_steps, seeds, num_seeds, restart_prob, restart_steps,
                                   restart_dtype, rng_seed, traces, eids, ws, L, s);
  });
}

int dgla_random_walk_host(const dgla_walk_relation* rels, int num_rels, const int32_t* metapath, int64_t num_steps,
                          const void* seeds, int64_t num_seeds, double restart_prob, const void* restart_steps,
                          dgla_dtype restart_dtype, uint64_t rng_seed, void* traces, void* eids) {
  int idbits = 0;
  if (check_walk("random_walk_host", rels, num_rels, metapath, num_steps, seeds, num_seeds, restart_steps,
                 restart_dtype, traces, &idbits))
    return -1;
  with_idx(idbits, [&](auto tag) {
    walk_host<decltype(tag)>(rels, metapath, num_steps, seeds, num_seeds, restart_prob, restart_steps, restart_dtype,
                             rng_seed, traces, eids);
  });
  return 0;
}

}  // extern "C"
