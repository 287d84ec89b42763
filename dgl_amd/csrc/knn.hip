// Point-cloud graphs on the device: k nearest neighbours per segment (dgl.knn_graph, dgl.segmented_knn_graph,
// dgl.functional.knn) and farthest point sampling (dgl.geometry.farthest_point_sampler).
//
// Reference: BruteforceKnnKernel / BruteforceKnnShareKernel (src/graph/transform/cuda/knn.cu): one thread per query,
// a max-heap per thread in global or shared memory, every data row read from global memory by every query; the
// "bruteforce-blas" path composes cdist + topk through an N x N matrix.  fps_kernel
// (src/geometry/cuda/geometry_op_impl.cu): one block per cloud, a shared-memory arg-max per sample.
//
// MI355X-first choices:
//  * The rule is the one of csrc/knn_step.h, compiled here for the kernels and for dgla_knn_host / dgla_fps_host: one
//    fma chain per pair in ascending column order, keys (d, id), NaN as +inf.  Device == host bit for bit.
//  * k-NN: a workgroup is ONE wavefront that owns a tile of 64 queries of one segment, a query per lane.  The
//    segment's data rows stream through LDS in steps of kKnnDataTile rows x C columns (C = 4 for D <= 4, else 16),
//    kKnnStageBytes of them between two barriers, so a data row comes from HBM / L2 once per 64 queries; every lane
//    reads the SAME LDS address (a broadcast, no bank conflict), the query's columns sit in registers.  A wide row goes
//    chunk by chunk: the kKnnDataTile running sums of a lane stay in registers between chunks, which is the header's
//    chain.  Columns past D are staged as zeros on both sides: fma(0, 0, acc) == acc exactly, so the padding changes no
//    bit.  Nothing of size N x N exists.
//  * The k best keys of a lane live in LDS as list[slot * 64 + lane]: consecutive lanes on consecutive banks, so the
//    lanes never collide whatever slot each of them is at.  The list is UNORDERED; its largest key (the k-th key) and
//    that key's slot are mirrored in registers, so a losing candidate, nearly all of them, costs one compare and no
//    LDS access.  A winner overwrites the k-th key's slot and rescans the k slots for the new largest: k independent
//    reads, where a sorted insertion is a chain of dependent LDS round trips.  A rescan stalls the whole wavefront,
//    so for k <= kKnnBufferedK a tile's winners are first appended to a per-lane LDS buffer (one write each) and
//    inserted afterwards in a loop that ends with the lane that has most: rescans per tile = max over lanes of the
//    winners, not the tile's rows (measured, with the forms before it: DESIGN.md 3.16).  The store ranks every slot by
//    counting the smaller keys (k^2 reads, no LDS write) and writes it to its rank: sorted output without a sort
//    pass.  Unfilled slots hold distinct sentinel positions behind every row, so keys stay unique.  Lists in LDS for
//    every k: no dynamically indexed registers, no scratch.  LDS per workgroup: 8 KiB of stage plus (8 or 12) * 64
//    bytes per list slot and buffer slot, 34 KiB at k = 20 fp32, 56 KiB at k = 32 or 64 fp64.
//  * No atomics; the same bytes on every run.  The tile table (segment offsets and the first tile of every segment)
//    is three small host arrays copied to the workspace in stream order; nothing is read back.
//  * Farthest points: one workgroup of 256 threads per cloud, the whole sample loop inside one launch.  mind lives in
//    LDS up to kFpsLdsRows rows, else in the workspace; thread t owns rows t, t + 256, ... (consecutive banks), so mind
//    needs no barrier; an iteration is one sweep (distance to the last sample, lower mind, local arg-max), a
//    wavefront butterfly and a four-entry LDS exchange.
#include "../../include/dgl_amd.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "host_util.h"
#include "knn_step.h"

namespace dgla {
namespace {

constexpr int kKnnQueryTile = 64;  // queries per workgroup: one per lane of ONE wavefront
constexpr int kKnnDataTile = 32;   // data rows per LDS tile (running sums per lane)
constexpr int kKnnStageBytes = 8192;  // data staged in LDS between two barriers: 16 / 4 steps of fp32 (C = 4 / 16), 8 / 2 of fp64
constexpr int kKnnBufferedK = 32;  // k up to here buffers a tile's winners (the buffer's 24 KiB of fp64 fit beside the lists)
constexpr int kKnnEmpty = 0x7fffffff - kKnnMaxK;  // unfilled slot j holds position kKnnEmpty + j: behind every row

constexpr int kFpsBlock = 256;
constexpr int64_t kFpsLdsRows = 4096;  // mind of a cloud in LDS up to here (32 KiB of fp64)

int knn_chunk(int64_t dim) { return dim <= 4 ? 4 : 16; }

// ---- k-NN -------------------------------------------------------------------------------------------
// The k best keys of one lane, in LDS as list[slot * 64 + lane] (ld / lp point at this lane's column): UNORDERED, with
// the largest key (the k-th key) and its slot mirrored in wd / wp / wslot.  Unfilled slot j holds (+inf, kKnnEmpty + j),
// so keys are unique.
template <typename T>
struct KnnList {
  T* ld;
  int* lp;
  T wd;
  int wp, wslot, k;

  __device__ __forceinline__ void init(int k_, T* ld_, int* lp_) {
    k = k_, ld = ld_, lp = lp_;
    for (int j = 0; j < k; ++j) ld[j * kKnnQueryTile] = knn_inf<T>(), lp[j * kKnnQueryTile] = kKnnEmpty + j;
    wd = knn_inf<T>(), wp = kKnnEmpty + k - 1, wslot = k - 1;
  }
  __device__ __forceinline__ bool wins(T d, int pos) const { return knn_key_less(d, pos, wd, wp); }
  // (d, pos) wins: it takes the slot of the k-th key, and the largest of the list becomes the k-th (k independent
  // reads that pipeline; a sorted insertion would be a chain of dependent LDS round trips)
  __device__ __forceinline__ void insert(T d, int pos) {
    ld[wslot * kKnnQueryTile] = d, lp[wslot * kKnnQueryTile] = pos;
    wd = d, wp = pos;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
      const T e = ld[j * kKnnQueryTile];
      const int ep = lp[j * kKnnQueryTile];
      if (knn_key_less(wd, wp, e, ep)) wd = e, wp = ep, wslot = j;
    }
  }
  // every slot to its rank (keys are unique: the rank is the number of smaller keys): ascending key order, no sort pass
  template <typename Idx>
  __device__ __forceinline__ void store(int64_t q, int64_t xs, Idx* __restrict__ out_ids, T* __restrict__ out_dist,
                                        int64_t total) const {
    for (int j = 0; j < k; ++j) {
      const T d = ld[j * kKnnQueryTile];
      const int p = lp[j * kKnnQueryTile];
      int rank = 0;
#pragma unroll 4
      for (int i = 0; i < k; ++i) rank += knn_key_less(ld[i * kKnnQueryTile], lp[i * kKnnQueryTile], d, p) ? 1 : 0;
      const int64_t slot = q * k + rank;
      out_ids[slot] = static_cast<Idx>(q);
      out_ids[total + slot] = p >= kKnnEmpty ? static_cast<Idx>(-1) : static_cast<Idx>(xs + p);
      if (out_dist) out_dist[slot] = d;
    }
  }
};

// LDS bytes of a workgroup: the stage, the lists and (BUF) the winners of one tile
template <typename T>
size_t knn_lds_bytes(int k, int BUF) {
  const int entries = k + (BUF ? kKnnDataTile : 0);
  return kKnnStageBytes + sizeof(T) * entries * kKnnQueryTile + sizeof(int) * entries * kKnnQueryTile;
}

// tab = x_offsets[S + 1], y_offsets[S + 1], tile_start[S + 1] (tile_start[s] = the first workgroup of segment s).
// out_ids[0][slot] = query row, out_ids[1][slot] = data row (global) or -1, out_dist[slot] (may be NULL).
template <typename T, typename Idx, int C, int BUF>
__global__ __launch_bounds__(kKnnQueryTile) void knn_kernel(const T* __restrict__ x, const T* __restrict__ y, int64_t D,
                                                            const int64_t* __restrict__ tab, int64_t S, int k,
                                                            Idx* __restrict__ out_ids, T* __restrict__ out_dist,
                                                            int64_t total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
  const int lane = threadIdx.x;
  const int entries = k + (BUF ? kKnnDataTile : 0);
  constexpr int kStage = kKnnStageBytes / static_cast<int>(sizeof(T));       // elements of a stage
  T* tile = reinterpret_cast<T*>(knn_lds);                                  // [G][kKnnDataTile][C]
  T* ld = tile + kStage + lane;                                   // [entries][64], this lane's column:
  int* lp = reinterpret_cast<int*>(tile + kStage + entries * kKnnQueryTile) + lane;  // k list slots, then
  T* bd = ld + k * kKnnQueryTile;                                           // the winners of one tile (BUF)
  int* bp = lp + k * kKnnQueryTile;
  const int64_t *xo = tab, *yo = tab + (S + 1), *ts = tab + 2 * (S + 1);
  const int64_t b = blockIdx.x;
  int64_t lo = 0, hi = S;  // the last segment whose first tile is <= b (empty query segments own no tile)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ts[mid] <= b) lo = mid; else hi = mid;
  }
  const int64_t q = yo[lo] + (b - ts[lo]) * kKnnQueryTile + lane;
  const bool valid = q < yo[lo + 1];
  const int64_t xs = xo[lo], n = xo[lo + 1] - xs;

  KnnList<T> list;
  list.init(k, ld, lp);

  // The segment's data goes through LDS in STAGES of G steps, a step being (data tile of kKnnDataTile rows, column
  // chunk of C columns) in the order tile-major, chunk-minor: one pair of barriers and one exposed load latency per
  // stage, G * kKnnDataTile * C = kKnnStageBytes / sizeof(T) elements.  Rows past the segment and columns past D are
  // staged as zeros.
  constexpr int G = kKnnStageBytes / static_cast<int>(sizeof(T)) / (kKnnDataTile * C);
  constexpr int E = kKnnDataTile * C / kKnnQueryTile;  // elements of one step per lane
  const int64_t nchunks = (D + C - 1) / C;
  const int64_t nsteps = (n + kKnnDataTile - 1) / kKnnDataTile * nchunks;
  T qr[C], acc[kKnnDataTile];
#pragma unroll
  for (int j = 0; j < C; ++j) qr[j] = T(0);
#pragma unroll
  for (int r = 0; r < kKnnDataTile; ++r) acc[r] = T(0);
  int64_t r0 = 0, c = 0;    // the step being computed
  int64_t lr0 = 0, lc = 0;  // the step being staged
  for (int64_t s0 = 0; s0 < nsteps; s0 += G) {
    const int steps = static_cast<int>(nsteps - s0 < G ? nsteps - s0 : G);
    __syncthreads();  // the stage before has been consumed
    // every load is unconditional (the address is clamped into the segment, the value replaced by zero afterwards), so
    // the G * E loads of a lane are in flight together; steps past the segment's end stage zeros that nobody reads
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const int e = lane + i * kKnnQueryTile, r = e / C, j = e % C;
        const int64_t row = lr0 + r, col = lc * C + j;
        const T v = x[(xs + (row < n ? row : n - 1)) * D + (col < D ? col : D - 1)];
        tile[g * kKnnDataTile * C + e] = (row < n && col < D) ? v : T(0);
      }
      if (++lc == nchunks) lc = 0, lr0 += kKnnDataTile;
    }
    __syncthreads();
    for (int g = 0; g < steps; ++g) {
      const T* tg = tile + g * kKnnDataTile * C;
      if (valid && (nchunks > 1 || (s0 == 0 && g == 0))) {  // (a single chunk stays in registers over the whole segment)
#pragma unroll
        for (int j = 0; j < C; ++j) qr[j] = c * C + j < D ? y[q * D + c * C + j] : T(0);
      }
#pragma unroll
      for (int r = 0; r < kKnnDataTile; ++r) {
#pragma unroll
        for (int j = 0; j < C; ++j) acc[r] = knn_step(acc[r], qr[j], tg[r * C + j]);
      }
      if (++c < nchunks) continue;
      // the tile's distances are complete: offer them in ascending row order
      const int rows = static_cast<int>(n - r0 < kKnnDataTile ? n - r0 : kKnnDataTile);
      if constexpr (BUF) {
        // winners against the k-th key of the tile's start (never smaller than the current one) go to this lane's
        // buffer column at one LDS write each; they are then re-tested and inserted in a loop the wavefront leaves as
        // soon as no lane has a winner left, so the rescans of a tile number max-over-lanes(winners), not its rows
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < kKnnDataTile; ++r) {
          const T d = knn_canonical(acc[r]);
          if (valid && r < rows && list.wins(d, static_cast<int>(r0) + r)) {
            bd[cnt * kKnnQueryTile] = d, bp[cnt * kKnnQueryTile] = static_cast<int>(r0) + r;
            ++cnt;
          }
          acc[r] = T(0);
        }
        for (int i = 0; __any(i < cnt); ++i) {
          if (i < cnt) {
            const T d = bd[i * kKnnQueryTile];
            const int pos = bp[i * kKnnQueryTile];
            if (list.wins(d, pos)) list.insert(d, pos);
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < kKnnDataTile; ++r) {
          const T d = knn_canonical(acc[r]);
          if (valid && r < rows && list.wins(d, static_cast<int>(r0) + r)) list.insert(d, static_cast<int>(r0) + r);
          acc[r] = T(0);
        }
      }
      c = 0, r0 += kKnnDataTile;
    }
  }
  if (valid) list.store(q, xs, out_ids, out_dist, total);
}

// ---- farthest points --------------------------------------------------------------------------------
// a start row outside [0, N) counts as row 0 (the Python surface refuses it before the call)
__host__ __device__ inline int64_t fps_start(int64_t s, int64_t N) { return s >= 0 && s < N ? s : 0; }

template <typename T, bool LDS>
__global__ __launch_bounds__(kFpsBlock) void fps_kernel(const T* __restrict__ pos, int64_t N, int64_t D, int64_t npoints,
                                                        const int64_t* __restrict__ start, int64_t* __restrict__ out,
                                                        T* __restrict__ ws_mind) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fps_lds[];
  __shared__ T red_m[kFpsBlock / 64];
  __shared__ int red_i[kFpsBlock / 64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const T* p = pos + b * N * D;
  T* mind = LDS ? reinterpret_cast<T*>(fps_lds) : ws_mind + b * N;
  for (int64_t i = tid; i < N; i += kFpsBlock) mind[i] = knn_inf<T>();  // (row i belongs to thread i mod 256 throughout)
  int cur = static_cast<int>(fps_start(start[b], N));
  if (tid == 0) out[b * npoints] = cur;
  for (int64_t t = 1; t < npoints; ++t) {
    T best = static_cast<T>(-2);  // below the mark of a chosen row: any row beats it
    int bi = 0x7fffffff;
    const T* pc = p + static_cast<int64_t>(cur) * D;
    for (int64_t i = tid; i < N; i += kFpsBlock) {
      T acc = T(0);
      for (int64_t j = 0; j < D; ++j) acc = knn_step(acc, p[i * D + j], pc[j]);
      const T m = i == cur ? fps_chosen<T>() : fps_lower(mind[i], acc);
      mind[i] = m;
      if (fps_better(m, i, best, static_cast<int64_t>(bi))) best = m, bi = static_cast<int>(i);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const T om = __shfl_xor(best, s, 64);
      const int oi = __shfl_xor(bi, s, 64);
      if (fps_better(om, static_cast<int64_t>(oi), best, static_cast<int64_t>(bi))) best = om, bi = oi;
    }
    if ((tid & 63) == 0) red_m[tid >> 6] = best, red_i[tid >> 6] = bi;
    __syncthreads();
    best = red_m[0], bi = red_i[0];
#pragma unroll
    for (int w = 1; w < kFpsBlock / 64; ++w)
      if (fps_better(red_m[w], static_cast<int64_t>(red_i[w]), best, static_cast<int64_t>(bi))) best = red_m[w], bi = red_i[w];
    __syncthreads();  // (the four entries are rewritten by the next sample)
    cur = bi;
    if (tid == 0) out[b * npoints + t] = cur;
  }
}

// ---- host side --------------------------------------------------------------------------------------
struct KnnLayout {  // the tile table in the workspace
  size_t tab, bytes;
};

KnnLayout knn_layout(int64_t num_segs) {
  KnnLayout L{};
  Carver c;
  L.tab = c.take(sizeof(int64_t) * 3 * static_cast<size_t>(num_segs + 1));
  L.bytes = c.bytes();
  return L;
}

struct FpsLayout {  // mind of every cloud, when it does not fit LDS
  size_t mind, bytes;
};

FpsLayout fps_layout(int dtype, int64_t batch, int64_t n) {
  FpsLayout L{};
  Carver c;
  if (n > kFpsLdsRows) L.mind = c.take((dtype == kF64 ? 8 : 4) * static_cast<size_t>(batch) * static_cast<size_t>(n));
  L.bytes = c.bytes();
  return L;
}

int check_float(const char* who, int dtype) {
  if (dtype == kF16 || dtype == kBF16)
    return fail(who, "float16 / bfloat16 operands are not supported; use float32 or float64");
  if (dtype != kF32 && dtype != kF64) return fail(who, "unknown dtype " + std::to_string(dtype));
  return 0;
}

int check_offsets(const char* who, const std::string& name, const int64_t* off, int64_t num_segs, int64_t rows) {
  if (!off) return fail(who, name + "_offsets is null");
  if (off[0] != 0) return fail(who, name + "_offsets do not match: they must start at 0");
  for (int64_t s = 0; s < num_segs; ++s)
    if (off[s + 1] < off[s]) return fail(who, name + "_offsets do not match: they descend at segment " + std::to_string(s));
  if (off[num_segs] != rows)
    return fail(who, name + "_offsets do not match: they end at " + std::to_string(off[num_segs]) + ", " + name + " has " +
                         std::to_string(rows) + " rows");
  return 0;
}

// everything dgla_knn and dgla_knn_host refuse
int check_knn(const char* who, const void* x, int64_t num_x, const void* y, int64_t num_y, int dtype, int64_t dim,
              const int64_t* xo, const int64_t* yo, int64_t num_segs, int64_t k, int idbits, const void* out_ids) {
  if (check_float(who, dtype)) return -1;
  if (!idbits_ok(idbits)) return fail(who, "idtype must be int32 or int64");
  if (num_x < 0 || num_y < 0 || num_segs < 0) return fail(who, "negative size");
  if (dim < 1) return fail(who, "dim must be at least 1, got " + std::to_string(dim));
  if (k < 1) return fail(who, "k must be at least 1, got " + std::to_string(k));
  if (k > kKnnMaxK) return fail(who, "k = " + std::to_string(k) + " is above the limit kKnnMaxK = " + std::to_string(kKnnMaxK));
  if (num_x > 0 && !x) return fail(who, "x is null");
  if (!y && num_y != num_x) return fail(who, "y is null (a self-query has num_y == num_x)");
  if (num_x >= (int64_t(1) << 31) - kKnnMaxK || num_y >= (int64_t(1) << 31) - kKnnMaxK)
    return fail(who, "num_x and num_y must be below 2^31 - " + std::to_string(kKnnMaxK));
  if (idbits == 32 && num_y * k >= (int64_t(1) << 31)) return fail(who, "k * num_y does not fit int32 ids; use int64 ids");
  if (check_offsets(who, "x", xo, num_segs, num_x) || check_offsets(who, "y", yo, num_segs, num_y)) return -1;
  if (num_y > 0 && !out_ids) return fail(who, "out_ids is null");
  return 0;
}

int check_fps(const char* who, const void* pos, int dtype, int64_t batch, int64_t n, int64_t dim, int64_t npoints,
              const int64_t* start, const int64_t* out) {
  if (check_float(who, dtype)) return -1;
  if (batch < 0 || n < 0) return fail(who, "negative size");
  if (dim < 1) return fail(who, "dim must be at least 1, got " + std::to_string(dim));
  if (npoints < 1 || npoints > n)
    return fail(who, "npoints must be in [1, num_rows = " + std::to_string(n) + "], got " + std::to_string(npoints));
  if (n >= (int64_t(1) << 31) - 1) return fail(who, "num_rows must be below 2^31 - 1");
  if (batch >= (int64_t(1) << 31)) return fail(who, "batch must be below 2^31");
  if (batch > 0 && (!pos || !start || !out)) return fail(who, "pos / start / out are null");
  return 0;
}

// ---- the rule run by the CPU ------------------------------------------------------------------------
template <typename T, typename Idx>
void knn_host(const T* x, const T* y, int64_t D, const int64_t* xo, const int64_t* yo, int64_t S, int64_t k, Idx* out_ids,
              T* out_dist, int64_t total) {
  std::vector<std::pair<T, int64_t>> keys;
  const auto less = [](const std::pair<T, int64_t>& a, const std::pair<T, int64_t>& b) {
    return knn_key_less(a.first, a.second, b.first, b.second);
  };
  for (int64_t s = 0; s < S; ++s) {
    const int64_t xs = xo[s], n = xo[s + 1] - xs;
    const int64_t kept = n < k ? n : k;
    for (int64_t q = yo[s]; q < yo[s + 1]; ++q) {
      keys.resize(n);
      for (int64_t i = 0; i < n; ++i)
        keys[i] = {knn_canonical(knn_accumulate(T(0), y + q * D, x + (xs + i) * D, D)), xs + i};
      std::partial_sort(keys.begin(), keys.begin() + kept, keys.end(), less);
      for (int64_t j = 0; j < k; ++j) {
        const int64_t slot = q * k + j;
        out_ids[slot] = static_cast<Idx>(q);
        out_ids[total + slot] = static_cast<Idx>(j < kept ? keys[j].second : -1);
        if (out_dist) out_dist[slot] = j < kept ? keys[j].first : knn_inf<T>();
      }
    }
  }
}

template <typename T>
void fps_host(const T* pos, int64_t batch, int64_t N, int64_t D, int64_t npoints, const int64_t* start, int64_t* out) {
  std::vector<T> mind(N);
  for (int64_t b = 0; b < batch; ++b) {
    const T* p = pos + b * N * D;
    std::fill(mind.begin(), mind.end(), knn_inf<T>());
    int64_t cur = fps_start(start[b], N);
    out[b * npoints] = cur;
    for (int64_t t = 1; t < npoints; ++t) {
      T best = static_cast<T>(-2);
      int64_t bi = N;
      for (int64_t i = 0; i < N; ++i) {
        mind[i] = i == cur ? fps_chosen<T>() : fps_lower(mind[i], knn_accumulate(T(0), p + i * D, p + cur * D, D));
        if (fps_better(mind[i], i, best, bi)) best = mind[i], bi = i;
      }
      cur = bi;
      out[b * npoints + t] = cur;
    }
  }
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

int dgla_knn_max_k(void) { return kKnnMaxK; }

int dgla_knn_tile_sizes(int* query_tile, int* data_tile) {
  if (query_tile) *query_tile = kKnnQueryTile;
  if (data_tile) *data_tile = kKnnDataTile;
  return 0;
}

size_t dgla_knn_workspace_bytes(int64_t num_segs) {
  if (num_segs <= 0) return 0;
  return knn_layout(num_segs).bytes;
}

int dgla_knn(const void* x, int64_t num_x, const void* y, int64_t num_y, int dtype, int64_t dim, const int64_t* x_offsets,
             const int64_t* y_offsets, int64_t num_segs, int64_t k, int idtype_bits, void* out_ids, void* out_dist,
             void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "knn";
  if (check_knn(who, x, num_x, y, num_y, dtype, dim, x_offsets, y_offsets, num_segs, k, idtype_bits, out_ids)) return -1;
  if (num_y == 0) return 0;
  const int64_t S = num_segs;
  const KnnLayout L = knn_layout(S);
  if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  std::vector<int64_t> tab(3 * (S + 1));
  int64_t tiles = 0;
  for (int64_t s = 0; s <= S; ++s) {
    tab[s] = x_offsets[s];
    tab[S + 1 + s] = y_offsets[s];
    tab[2 * (S + 1) + s] = tiles;
    if (s < S) tiles += (y_offsets[s + 1] - y_offsets[s] + kKnnQueryTile - 1) / kKnnQueryTile;
  }
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(st, out_ids);
  int64_t* d_tab = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + L.tab);
  // (the host vector lives until the call returns; a pageable source has been staged by then)
  DGLA_CHECK_HIP(hipMemcpyAsync(d_tab, tab.data(), sizeof(int64_t) * tab.size(), hipMemcpyHostToDevice, st));
  const int C = knn_chunk(dim);
  const int BUF = k <= kKnnBufferedK ? 1 : 0;
  with_float(dtype, [&](auto ttag) {
    using T = decltype(ttag);
    const size_t lds = knn_lds_bytes<T>(static_cast<int>(k), BUF);
    const T* xx = static_cast<const T*>(x);
    const T* yy = y ? static_cast<const T*>(y) : xx;
    with_idx(idtype_bits, [&](auto tag) {
      using Idx = decltype(tag);
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles)), dim3(kKnnQueryTile), lds, st, xx, yy, dim, d_tab, S,
                           static_cast<int>(k), static_cast<Idx*>(out_ids), static_cast<T*>(out_dist), num_y * k);
      };
      if (C == 4 && BUF) launch(knn_kernel<T, Idx, 4, 1>);
      else if (C == 4) launch(knn_kernel<T, Idx, 4, 0>);
      else if (BUF) launch(knn_kernel<T, Idx, 16, 1>);
      else launch(knn_kernel<T, Idx, 16, 0>);
    });
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_knn_host(const void* x, int64_t num_x, const void* y, int64_t num_y, int dtype, int64_t dim, const int64_t* x_offsets,
                  const int64_t* y_offsets, int64_t num_segs, int64_t k, int idtype_bits, void* out_ids, void* out_dist) {
  if (check_knn("knn_host", x, num_x, y, num_y, dtype, dim, x_offsets, y_offsets, num_segs, k, idtype_bits, out_ids)) return -1;
  with_float(dtype, [&](auto ttag) {
    using T = decltype(ttag);
    with_idx(idtype_bits, [&](auto tag) {
      using Idx = decltype(tag);
      knn_host<T, Idx>(static_cast<const T*>(x), static_cast<const T*>(y ? y : x), dim, x_offsets, y_offsets, num_segs, k,
                       static_cast<Idx*>(out_ids), static_cast<T*>(out_dist), num_y * k);
    });
  });
  return 0;
}

size_t dgla_fps_workspace_bytes(int dtype, int64_t batch, int64_t num_rows) {
  if ((dtype != kF32 && dtype != kF64) || batch <= 0 || num_rows <= 0) return 0;
  return fps_layout(dtype, batch, num_rows).bytes;
}

int dgla_fps(const void* pos, int dtype, int64_t batch, int64_t num_rows, int64_t dim, int64_t npoints, const int64_t* start,
             int64_t* out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "fps";
  if (check_fps(who, pos, dtype, batch, num_rows, dim, npoints, start, out)) return -1;
  if (batch == 0) return 0;
  const FpsLayout L = fps_layout(dtype, batch, num_rows);
  if (L.bytes && need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(st, out);
  with_float(dtype, [&](auto ttag) {
    using T = decltype(ttag);
    const T* p = static_cast<const T*>(pos);
    if (L.bytes == 0) {
      hipLaunchKernelGGL((fps_kernel<T, true>), dim3(static_cast<unsigned>(batch)), dim3(kFpsBlock), sizeof(T) * num_rows, st, p,
                         num_rows, dim, npoints, start, out, static_cast<T*>(nullptr));
    } else {
      hipLaunchKernelGGL((fps_kernel<T, false>), dim3(static_cast<unsigned>(batch)), dim3(kFpsBlock), 0, st, p, num_rows, dim,
                         npoints, start, out, reinterpret_cast<T*>(static_cast<char*>(workspace) + L.mind));
    }
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_fps_host(const void* pos, int dtype, int64_t batch, int64_t num_rows, int64_t dim, int64_t npoints,
                  const int64_t* start, int64_t* out) {
  if (check_fps("fps_host", pos, dtype, batch, num_rows, dim, npoints, start, out)) return -1;
  with_float(dtype, [&](auto ttag) {
    using T = decltype(ttag);
    fps_host<T>(static_cast<const T*>(pos), batch, num_rows, dim, npoints, start, out);
  });
  return 0;
}

}  // extern "C"
