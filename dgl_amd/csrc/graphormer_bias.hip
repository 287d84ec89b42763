// Graphormer attention bias on the device: the SpatialEncoder and the PathEncoder of a graph transformer fused into one
// gather over what dgla_shortest_dist emits (dist and paths), forward and backward.
//
// Reference: python/dgl/nn/pytorch/gt/path_encoder.py and spatial_encoder.py compose torch operators: they index the
// edge features with the paths into a (pairs, L, d) tensor, contract it with the path table (einsum), divide by the
// clamped distance and add an embedding lookup of the clamped distance.  There is no kernel, and the indexed tensor is
// L * d times the size of the bias it makes.
//
// Here the contraction is hoisted out of the pairs: T = edge_feat . path_table^T is one small GEMM over the E edges
// (the library's segment_mm), and the bias of a pair is a sum of at most max_len rows of T.  The rule: include/dgl_amd.h
// "Graphormer attention bias".
//
// MI355X-first choices:
//  * Forward, ONE pass over the pairs.  A group of G = next_pow2(ceil(H * itemsize / 16)) lanes owns a pair and a lane
//    owns a 16-byte piece of the head row, so a wavefront takes 64 / G consecutive pairs and its output is one
//    contiguous span stored as 16-byte pieces.  The wave's ids are a contiguous span of `paths` too (Lc = Lp) or runs of
//    Lc ids (Lc < Lp): the wave loads them lane by lane, coalesced, into its own slice of LDS, from where the owning
//    lanes pick them up.  All Lc row gathers of a pair are issued before the first add (the kernel is instantiated
//    for Lc <= 8 and Lc <= 32 gathers held in registers), then added in the order of l with fp32 accumulation, divided,
//    the spatial row (the table sits in LDS, loaded once per workgroup) added, and the result rounded once at the store.
//    A head count whose rows are not whole 16-byte pieces takes the same kernel with element-wise, masked accesses.
//    Nothing is read back, nothing is cleared: the call can be captured.
//  * Backward to T, deterministic: the path index is inverted with the library's stable COO -> CSR sort (sort.hip.h;
//    key e * Lc + l, value the pair), so that every (e, l) row lists its pairs in ascending order.  A lane group per row
//    sums them: 16 lanes for rows of up to 16 pairs, the wavefront up to 256, the 256-lane workgroup above; heads sit
//    across the lanes, the entries across the rest of the group, the partial sums meet in a butterfly of fixed shape
//    (and, between the four waves of a workgroup row, in LDS in wave order).  No floating-point atomics; a row without
//    an entry stores zeros, so dT needs no fill.
//  * Backward to S, deterministic: a workgroup owns a fixed contiguous range of pairs, stages (bin, g row) tiles in LDS,
//    and lane (r, h) walks the tile in order adding the rows whose bin is r (the LDS reads are broadcasts).  A second
//    small launch folds the workgroups' partial tables in workgroup order and zeroes the padding row.
#include "../../include/dgl_amd.h"

#include <string>

#include "host_util.h"
#include "sort.hip.h"

namespace dgla {
namespace {

constexpr int kGbBlock = 256;          // threads per workgroup, 4 wavefronts
constexpr int kGbMaxHeads = 256;
constexpr int kGbMaxLen = 32;
constexpr int kGbLdsBytes = 65536;     // what a workgroup may take without asking the runtime for more
constexpr int kGbRows = 16;            // (e, l) rows per workgroup of the backward to T: one per 16-lane group
constexpr int kGbShortRow = 16;        // rows of up to this many pairs: 16 lanes
constexpr int kGbWaveRow = 256;        // up to this many: the wavefront; above: the workgroup
constexpr int kGbSlotsPerLane = 4;     // (bin, head) slots a lane of the backward to S owns
constexpr int kGbSlotChunk = kGbBlock * kGbSlotsPerLane;
constexpr int kGbTileFloats = 4096;    // g values per LDS tile of the backward to S
constexpr int kGbMaxPartials = 1024;   // workgroups (pair ranges) of the backward to S

template <typename T>
__device__ __forceinline__ T gb_zero() {
  return T{};
}

template <typename Idx>
__device__ __forceinline__ int64_t gb_divisor(Idx d, int64_t max_len) {
  const int64_t x = static_cast<int64_t>(d);
  return x < 1 ? 1 : (x > max_len ? max_len : x);
}

__device__ __forceinline__ void gb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// LDS: [spatial table, srows * H elements of T, rounded up to 16 bytes][waves x (64 >> lg) x Lc ids].
template <typename T, typename Idx, int LMAX>
__global__ __launch_bounds__(kGbBlock) void gb_forward_kernel(const Idx* __restrict__ dist, const Idx* __restrict__ paths,
                                                              int64_t P, int64_t Lp, int Lc, const T* __restrict__ table,
                                                              int64_t E, int64_t max_len, int H, const T* __restrict__ spatial,
                                                              int srows, T* __restrict__ out, int lg, int spatial_bytes,
                                                              int vec_ok) {
  constexpr int VEC = 16 / sizeof(T);
  using V = VecT<T, VEC>;
  extern __shared__ __attribute__((aligned(16))) unsigned char gb_lds[];
  T* lds_s = reinterpret_cast<T*>(gb_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int ppw = 64 >> lg;  // pairs per wavefront
  Idx* ids = reinterpret_cast<Idx*>(gb_lds + spatial_bytes) + static_cast<size_t>(wave) * ppw * Lc;

  for (int i = tid; i < srows * H; i += blockDim.x) lds_s[i] = spatial[i];
  __syncthreads();  // (the only workgroup barrier: every wave reaches it)

  const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * waves + wave) * ppw;
  const int np = static_cast<int>(P - p0 < ppw ? (P - p0 < 0 ? 0 : P - p0) : ppw);
  for (int i = lane; i < np * Lc; i += 64) {  // Lc == Lp: one contiguous span
    const int r = i / Lc, l = i - r * Lc;
    ids[i] = paths[(p0 + r) * Lp + l];
  }
  gb_wave_sync();

  const int r = lane >> lg, piece = lane & ((1 << lg) - 1);
  const int h0 = piece * VEC;
  if (r >= np || h0 >= H) return;
  const int64_t p = p0 + r;
  const Idx d = dist[p];

  V raw[LMAX];
#pragma unroll
  for (int l = 0; l < LMAX; ++l) {  // every gather of the pair in flight before the first add
    const int64_t e = l < Lc ? static_cast<int64_t>(ids[r * Lc + l]) : -1;
    const bool hit = e >= 0 && e < E;  // (-1: the zero row; an id >= E is the caller's error and reads nothing)
    const T* row = table + ((hit ? e : 0) * max_len + l) * H + h0;
    if (hit && vec_ok) {
      raw[l] = *reinterpret_cast<const V*>(row);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) raw[l].v[k] = hit && h0 + k < H ? row[k] : gb_zero<T>();
    }
  }
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
#pragma unroll
  for (int l = 0; l < LMAX; ++l)
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] += to_acc<T>(raw[l].v[k]);

  const float div = static_cast<float>(gb_divisor<Idx>(d, max_len));
  int64_t bin = static_cast<int64_t>(d);
  bin = (bin < -1 ? -1 : (bin > srows - 2 ? srows - 2 : bin)) + 1;
  V res;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    float x = acc[k] / div;
    if (spatial && h0 + k < H) x += to_acc<T>(lds_s[bin * H + h0 + k]);
    res.v[k] = from_acc<T>(x);
  }
  T* o = out + p * H + h0;
  if (vec_ok) {
    *reinterpret_cast<V*>(o) = res;
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (h0 + k < H) o[k] = res.v[k];
  }
}

// ---- backward: the inverted path index ---------------------------------------------------------------------------------
// entry i = (p, l), l < Lc: key e * Lc + l, value p.  A -1 and an id >= E go to row E * Lc, which nobody reads; an
// id >= E also raises the flag.
template <typename Idx, typename SI>
__global__ __launch_bounds__(kGbBlock) void gb_keys_kernel(const Idx* __restrict__ paths, int64_t n, int64_t Lp, int64_t Lc,
                                                           int64_t E, SI* __restrict__ keys, SI* __restrict__ cols,
                                                           int* __restrict__ flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGbBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t p = i / Lc, l = i - p * Lc;
  const int64_t e = static_cast<int64_t>(paths[p * Lp + l]);
  if (e >= E) atomicOr(flag, 1);
  keys[i] = static_cast<SI>(e >= 0 && e < E ? e * Lc + l : E * Lc);
  cols[i] = static_cast<SI>(p);
}

// The lane's share of one row for head h, then the butterfly over the lanes that share the head: every lane of the
// group returns the sum.  `li` is the lane inside the group of GS, `hlg` = log2 of the lanes the heads lie across;
// entries part * ES + es, then every parts * ES (ES = GS >> hlg entry slots).  Called by whole groups.
template <int GS, typename T, typename Idx, typename SI>
__device__ __forceinline__ float gb_row_sum(int li, int hlg, int64_t h, bool h_ok, int64_t lo, int64_t n, int part, int parts,
                                            const SI* __restrict__ pairs, const Idx* __restrict__ dist,
                                            const T* __restrict__ g, int64_t H, int64_t max_len) {
  const int es = li >> hlg, slots = GS >> hlg;
  float acc = 0.f;
  for (int64_t j = static_cast<int64_t>(part) * slots + es; j < n; j += static_cast<int64_t>(parts) * slots) {
    const int64_t p = static_cast<int64_t>(pairs[lo + j]);
    const float div = static_cast<float>(gb_divisor<Idx>(dist[p], max_len));
    if (h_ok) acc += to_acc<T>(g[p * H + h]) / div;
  }
  for (int off = 1 << hlg; off < GS; off <<= 1) acc += __shfl_xor(acc, off);
  return acc;
}

// dT[rr][h], rr = e * max_len + l: a workgroup takes kGbRows rows.
template <typename T, typename Idx, typename SI>
__global__ __launch_bounds__(kGbBlock) void gb_grad_table_kernel(const SI* __restrict__ indptr, const SI* __restrict__ pairs,
                                                                 int64_t nnz, const Idx* __restrict__ dist,
                                                                 const T* __restrict__ g, int64_t rows, int64_t Lc,
                                                                 int64_t max_len, int H, int hlg16, int hlg64,
                                                                 T* __restrict__ grad) {
  __shared__ int64_t s_lo[kGbRows], s_n[kGbRows];
  __shared__ float s_part[kGbBlock / 64][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, group = tid >> 4, gl = tid & 15;
  const int64_t rr = static_cast<int64_t>(blockIdx.x) * kGbRows + group;
  int64_t lo = 0, n = 0;
  if (rr < rows) {
    const int64_t e = rr / max_len, l = rr - e * max_len;
    if (l < Lc) {  // (a position the paths do not reach has no entry)
      lo = static_cast<int64_t>(indptr[e * Lc + l]);
      int64_t hi = static_cast<int64_t>(indptr[e * Lc + l + 1]);
      lo = lo < 0 ? 0 : lo;
      hi = hi > nnz ? nnz : hi;
      n = hi > lo ? hi - lo : 0;
    }
  }
  if (gl == 0) s_lo[group] = lo, s_n[group] = rr < rows ? n : -1;
  __syncthreads();

  // 16 lanes per row: the short rows, the empty ones included
  if (rr < rows && n <= kGbShortRow) {
    const int hl = gl & ((1 << hlg16) - 1);
    for (int h = hl; h - hl < H; h += 1 << hlg16) {
      const float s = gb_row_sum<16, T, Idx, SI>(gl, hlg16, h, h < H, lo, n, 0, 1, pairs, dist, g, H, max_len);
      if (gl >> hlg16 == 0 && h < H) grad[rr * H + h] = from_acc<T>(s);
    }
  }
  // the wavefront per row: its own four rows, one after the other
  const int hl = lane & ((1 << hlg64) - 1);
  for (int k = 0; k < 4; ++k) {
    const int64_t nk = s_n[wave * 4 + k];  // (the same for the whole wave)
    if (nk <= kGbShortRow || nk > kGbWaveRow) continue;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kGbRows + wave * 4 + k;
    for (int h = hl; h - hl < H; h += 1 << hlg64) {
      const float s = gb_row_sum<64, T, Idx, SI>(lane, hlg64, h, h < H, s_lo[wave * 4 + k], nk, 0, 1, pairs, dist, g, H, max_len);
      if (lane >> hlg64 == 0 && h < H) grad[row * H + h] = from_acc<T>(s);
    }
  }
  // the workgroup per row: every wave sums a quarter of the entries, wave 0 folds the four in wave order
  for (int k = 0; k < kGbRows; ++k) {
    const int64_t nk = s_n[k];  // (the same for the whole workgroup: the barriers below are uniform)
    if (nk <= kGbWaveRow) continue;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kGbRows + k;
    for (int h = hl; h - hl < H; h += 1 << hlg64) {
      s_part[wave][lane] = gb_row_sum<64, T, Idx, SI>(lane, hlg64, h, h < H, s_lo[k], nk, wave, kGbBlock / 64, pairs, dist, g, H, max_len);
      __syncthreads();
      if (wave == 0 && lane >> hlg64 == 0 && h < H)
        grad[row * H + h] = from_acc<T>(((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane]);
      __syncthreads();
    }
  }
}

// ---- backward to S -------------------------------------------------------------------------------------------------------
// Workgroup (x, y): pairs [x * span, (x + 1) * span), slots [y * kGbSlotChunk, (y + 1) * kGbSlotChunk) of the (bin, head)
// table.  LDS: [tile_pairs bins][tile_pairs * H g values].
template <typename T, typename Idx>
__global__ __launch_bounds__(kGbBlock) void gb_grad_spatial_kernel(const Idx* __restrict__ dist, const T* __restrict__ g,
                                                                   int64_t P, int H, int srows, int64_t span, int tile_pairs,
                                                                   float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gb_lds[];
  int* bins = reinterpret_cast<int*>(gb_lds);
  float* gt = reinterpret_cast<float*>(gb_lds) + tile_pairs;
  const int tid = threadIdx.x, slots = srows * H;
  int bin_of[kGbSlotsPerLane], head_of[kGbSlotsPerLane];
  float acc[kGbSlotsPerLane];
#pragma unroll
  for (int k = 0; k < kGbSlotsPerLane; ++k) {
    const int s = blockIdx.y * kGbSlotChunk + k * kGbBlock + tid;
    bin_of[k] = s < slots ? s / H : -1;  // (no staged bin is negative)
    head_of[k] = s < slots ? s % H : 0;
    acc[k] = 0.f;
  }
  const int64_t begin = static_cast<int64_t>(blockIdx.x) * span;
  const int64_t end = begin + span < P ? begin + span : P;
  for (int64_t t0 = begin; t0 < end; t0 += tile_pairs) {  // (the same trip count for the whole workgroup)
    const int nt = static_cast<int>(end - t0 < tile_pairs ? end - t0 : tile_pairs);
    for (int i = tid; i < nt; i += kGbBlock) {
      int64_t b = static_cast<int64_t>(dist[t0 + i]);
      b = (b < -1 ? -1 : (b > srows - 2 ? srows - 2 : b)) + 1;
      bins[i] = static_cast<int>(b);
    }
    for (int i = tid; i < nt * H; i += kGbBlock) gt[i] = to_acc<T>(g[t0 * H + i]);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const int b = bins[t];
#pragma unroll
      for (int k = 0; k < kGbSlotsPerLane; ++k)
        if (b == bin_of[k]) acc[k] += gt[t * H + head_of[k]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kGbSlotsPerLane; ++k) {
    const int s = blockIdx.y * kGbSlotChunk + k * kGbBlock + tid;
    if (s < slots) partial[static_cast<int64_t>(blockIdx.x) * slots + s] = acc[k];
  }
}

template <typename T>
__global__ __launch_bounds__(kGbBlock) void gb_fold_spatial_kernel(const float* __restrict__ partial, int64_t parts, int slots,
                                                                   int H, int64_t padding_idx, T* __restrict__ grad) {
  const int s = blockIdx.x * kGbBlock + threadIdx.x;
  if (s >= slots) return;
  float sum = 0.f;
  for (int64_t w = 0; w < parts; ++w) sum += partial[w * slots + s];
  grad[s] = from_acc<T>(s / H == padding_idx ? 0.f : sum);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int gb_next_pow2_log(int64_t x) {  // log2 of the smallest power of two >= x
  int lg = 0;
  while ((int64_t(1) << lg) < x) ++lg;
  return lg;
}

// f(LMAX): the row gathers the forward holds in registers, 8 or kGbMaxLen
template <typename F>
int with_gb_lmax(int64_t Lc, F&& f) {
  if (Lc <= 8) return f(std::integral_constant<int, 8>{});
  return f(std::integral_constant<int, kGbMaxLen>{});
}

struct GbShape {
  int64_t P, Lp, Lc, E, max_len, H, srows;
  int64_t entries() const { return P * Lc; }        // what the inverted index sorts
  int64_t index_rows() const { return E * Lc + 1; }  // its rows: every (e, l) and the row of the dropped entries
  int sort_bits() const { return entries() <= INT32_MAX && index_rows() <= INT32_MAX ? 32 : 64; }
  int tile_pairs() const { return static_cast<int>(kGbTileFloats / H < 64 ? kGbTileFloats / H : 64); }
  int64_t span() const {  // pairs per workgroup of the backward to S: a function of the shape alone
    const int64_t tp = tile_pairs();
    const int64_t even = ((P + kGbMaxPartials - 1) / kGbMaxPartials + tp - 1) / tp * tp;
    return even > 8 * tp ? even : 8 * tp;
  }
  int64_t partials() const { return (P + span() - 1) / span(); }
};

msd::Plan gb_plan(const GbShape& g) {
  return msd::make_plan(g.entries(), msd::bits_for(g.index_rows()), msd::bits_for(g.P), msd::bits_for(g.entries()));
}

struct GbLayout {  // offsets into the workspace of dgla_graphormer_bias_backward
  size_t flag, keys, cols, indptr, pairs, pos, sort, partial, bytes;
};

GbLayout gb_layout(const GbShape& g) {
  GbLayout L{};
  Carver c;
  const size_t b = static_cast<size_t>(g.sort_bits() / 8), n = static_cast<size_t>(g.entries());
  const bool index = g.E > 0 && g.P > 0 && g.Lc > 0;
  L.flag = c.take(sizeof(int));
  L.keys = c.take(index ? b * n : 0);
  L.cols = c.take(index ? b * n : 0);
  L.indptr = c.take(index ? b * static_cast<size_t>(g.index_rows() + 1) : 0);
  L.pairs = c.take(index ? b * n : 0);
  L.pos = c.take(index ? b * n : 0);  // (the sort unpacks the positions too; nobody reads them)
  L.sort = c.take(index ? gb_plan(g).bytes : 0);
  L.partial = c.take(g.srows > 0 && g.P > 0 ? sizeof(float) * static_cast<size_t>(g.partials() * g.srows * g.H) : 0);
  L.bytes = c.bytes();
  return L;
}

// everything the three entry points refuse about the shape
int check_gb_shape(const char* who, int idtype_bits, int dtype, GbShape* g, int64_t path_len) {
  if (!idbits_ok(idtype_bits)) return fail(who, "idtype must be int32 or int64");
  if (check_float16(who, dtype, "operands")) return -1;
  if (g->P < 0 || path_len < 0 || g->E < 0 || g->srows < 0) return fail(who, "negative size");
  if (g->H < 1 || g->H > kGbMaxHeads)
    return fail(who, std::to_string(g->H) + " heads: the kernels take 1 to " + std::to_string(kGbMaxHeads));
  if (g->max_len < 1 || g->max_len > kGbMaxLen)
    return fail(who, "max_len " + std::to_string(g->max_len) + ": the kernels take 1 to " + std::to_string(kGbMaxLen));
  if (g->srows == 1) return fail(who, "a spatial table has at least two rows (max_dist + 2)");
  g->Lp = path_len;
  g->Lc = path_len < g->max_len ? path_len : g->max_len;
  if (g->P > INT64_MAX / 64 / (g->max_len * g->H) || g->E > INT64_MAX / 64 / (g->max_len * g->H))
    return fail(who, "sizes overflow");
  return 0;
}

template <typename T, typename Idx>
int gb_forward(const char* who, const GbShape& g, const Idx* dist, const Idx* paths, const T* table, const T* spatial, T* out,
               hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  const int lg = gb_next_pow2_log((g.H + VEC - 1) / VEC), ppw = 64 >> lg;
  const int spatial_bytes = static_cast<int>((sizeof(T) * static_cast<size_t>(g.srows * g.H) + 15) / 16 * 16);
  const size_t ids_bytes = sizeof(Idx) * static_cast<size_t>(ppw) * static_cast<size_t>(g.Lc > 0 ? g.Lc : 1);
  if (g.srows * g.H * static_cast<int64_t>(sizeof(T)) + 16 + static_cast<int64_t>(ids_bytes) > kGbLdsBytes)
    return fail(who, "a spatial table of " + std::to_string(g.srows) + " x " + std::to_string(g.H) +
                         " values does not fit the workgroup's LDS");
  int waves = static_cast<int>((kGbLdsBytes - spatial_bytes) / ids_bytes);
  waves = waves > kGbBlock / 64 ? kGbBlock / 64 : waves;
  const int64_t blocks = (g.P + static_cast<int64_t>(waves) * ppw - 1) / (static_cast<int64_t>(waves) * ppw);
  if (blocks > INT32_MAX) return fail(who, std::to_string(g.P) + " pairs are more than one launch takes");
  const int vec_ok = g.H % VEC == 0 && aligned_to(table, 16) && aligned_to(out, 16);
  const size_t lds = static_cast<size_t>(spatial_bytes) + ids_bytes * static_cast<size_t>(waves);
  const dim3 grid(static_cast<unsigned>(blocks)), block(static_cast<unsigned>(64 * waves));
  return with_gb_lmax(g.Lc, [&](auto ltag) -> int {
    hipLaunchKernelGGL((gb_forward_kernel<T, Idx, decltype(ltag)::value>), grid, block, lds, s, dist, paths, g.P, g.Lp,
                       static_cast<int>(g.Lc), table, g.E, g.max_len, static_cast<int>(g.H), spatial, static_cast<int>(g.srows), out, lg,
                       spatial_bytes, vec_ok);
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

// the inverted index into the workspace, then dT; the flag is read back before dT is trusted
template <typename T, typename Idx, typename SI>
int gb_backward_table(const char* who, const GbShape& g, const GbLayout& L, char* ws, const Idx* dist, const Idx* paths,
                      const T* grad_out, T* grad_table, hipStream_t s) {
  const int64_t rows = g.E * g.max_len;
  if ((rows + kGbRows - 1) / kGbRows > INT32_MAX || (g.entries() + kGbBlock - 1) / kGbBlock > INT32_MAX)
    return fail(who, "more (edge, position) rows or path entries than one launch takes");
  int* flag = reinterpret_cast<int*>(ws + L.flag);
  SI* indptr = reinterpret_cast<SI*>(ws + L.indptr);
  SI* pairs = reinterpret_cast<SI*>(ws + L.pairs);
  if (g.Lc > 0) {
    DGLA_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    SI* keys = reinterpret_cast<SI*>(ws + L.keys);
    SI* cols = reinterpret_cast<SI*>(ws + L.cols);
    hipLaunchKernelGGL((gb_keys_kernel<Idx, SI>), dim3(grid1(g.entries(), kGbBlock)), dim3(kGbBlock), 0, s, paths, g.entries(),
                       g.Lp, g.Lc, g.E, keys, cols, flag);
    const msd::Plan plan = gb_plan(g);
    msd::LevelArgs<SI> a{};
    a.row = keys;
    a.col = cols;
    a.indices = pairs;
    a.eids_out = reinterpret_cast<SI*>(ws + L.pos);
    a.indptr = indptr;
    a.num_rows = g.index_rows();
    if (plan.wide ? msd::run_levels<true, SI>(plan, a, ws + L.sort, s) : msd::run_levels<false, SI>(plan, a, ws + L.sort, s))
      return -1;
    int raised = 0;
    if (read_back(&raised, flag, sizeof(int), s)) return -1;  // the one read-back: 4 bytes
    if (raised) return fail(who, "paths holds an edge id outside [-1, " + std::to_string(g.E) + ")");
  }
  const int hlg16 = gb_next_pow2_log(g.H < 16 ? g.H : 16), hlg64 = gb_next_pow2_log(g.H < 64 ? g.H : 64);
  hipLaunchKernelGGL((gb_grad_table_kernel<T, Idx, SI>), dim3(grid1(rows, kGbRows)), dim3(kGbBlock), 0, s, indptr, pairs,
                     g.entries(), dist, grad_out, rows, g.Lc, g.max_len, static_cast<int>(g.H), hlg16, hlg64, grad_table);
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T, typename Idx>
int gb_backward_spatial(const GbShape& g, const GbLayout& L, char* ws, const Idx* dist, const T* grad_out, int64_t padding_idx,
                        T* grad_spatial, hipStream_t s) {
  const int slots = static_cast<int>(g.srows * g.H), tp = g.tile_pairs();
  float* partial = reinterpret_cast<float*>(ws + L.partial);
  const dim3 grid(static_cast<unsigned>(g.partials()), static_cast<unsigned>((slots + kGbSlotChunk - 1) / kGbSlotChunk));
  const size_t lds = sizeof(float) * static_cast<size_t>(tp) * static_cast<size_t>(g.H + 1);
  hipLaunchKernelGGL((gb_grad_spatial_kernel<T, Idx>), grid, dim3(kGbBlock), lds, s, dist, grad_out, g.P, static_cast<int>(g.H),
                     static_cast<int>(g.srows), g.span(), tp, partial);
  hipLaunchKernelGGL(gb_fold_spatial_kernel<T>, dim3(grid1(slots, kGbBlock)), dim3(kGbBlock), 0, s, partial, g.partials(), slots,
                     static_cast<int>(g.H), padding_idx, grad_spatial);
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_graphormer_bias_workspace_bytes(int64_t num_pairs, int64_t path_len, int64_t max_len, int64_t num_edges,
                                            int64_t num_heads, int64_t spatial_rows) {
  GbShape g{num_pairs, 0, 0, num_edges, max_len, num_heads, spatial_rows};
  if (check_gb_shape("graphormer_bias", 64, kF32, &g, path_len) || g.srows * g.H > INT32_MAX) return 0;
  return gb_layout(g).bytes;
}

int dgla_graphormer_bias_forward(int idtype_bits, int dtype, const void* dist, const void* paths, int64_t num_pairs,
                                 int64_t path_len, const void* table, int64_t num_edges, int64_t max_len, int64_t num_heads,
                                 const void* spatial, int64_t spatial_rows, void* out, void* hip_stream) {
  const char* who = "graphormer_bias";
  GbShape g{num_pairs, 0, 0, num_edges, max_len, num_heads, spatial ? spatial_rows : 0};
  if (check_gb_shape(who, idtype_bits, dtype, &g, path_len)) return -1;
  if (g.P == 0) return 0;
  if (!dist || !out) return fail(who, "dist or out is null");
  if (g.Lc > 0 && !paths) return fail(who, "paths is null");
  if (g.E > 0 && !table) return fail(who, "the projected table is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  return with_idx(idtype_bits, [&](auto itag) -> int {
    using Idx = decltype(itag);
    return with_float16(dtype, [&](auto ttag) -> int {
      using T = decltype(ttag);
      return gb_forward<T, Idx>(who, g, static_cast<const Idx*>(dist), static_cast<const Idx*>(paths),
                                static_cast<const T*>(table), static_cast<const T*>(spatial), static_cast<T*>(out), s);
    });
  });
}

int dgla_graphormer_bias_backward(int idtype_bits, int dtype, const void* dist, const void* paths, int64_t num_pairs,
                                  int64_t path_len, int64_t num_edges, int64_t max_len, int64_t num_heads,
                                  int64_t spatial_rows, const void* grad_out, void* grad_table, void* grad_spatial,
                                  int64_t padding_idx, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "graphormer_bias";
  GbShape g{num_pairs, 0, 0, num_edges, max_len, num_heads, grad_spatial ? spatial_rows : 0};
  if (check_gb_shape(who, idtype_bits, dtype, &g, path_len)) return -1;
  if (grad_spatial && g.srows < 2) return fail(who, "a spatial table has at least two rows (max_dist + 2)");
  if (g.srows * g.H > INT32_MAX) return fail(who, "the spatial table is larger than one launch takes");
  const bool want_table = grad_table && g.E > 0;
  if (!want_table && !grad_spatial) return 0;
  if (g.P > 0 && (!dist || !grad_out)) return fail(who, "dist or grad_out is null");
  if (g.P > 0 && g.Lc > 0 && want_table && !paths) return fail(who, "paths is null");
  const GbLayout L = gb_layout(g);
  if (optional_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, grad_out);
  const size_t item = float_itemsize(dtype);
  if (g.P == 0) {  // nothing to sum: zeros, without a launch
    if (want_table) DGLA_CHECK_HIP(hipMemsetAsync(grad_table, 0, item * static_cast<size_t>(g.E * g.max_len * g.H), s));
    if (grad_spatial) DGLA_CHECK_HIP(hipMemsetAsync(grad_spatial, 0, item * static_cast<size_t>(g.srows * g.H), s));
    return 0;
  }
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, L.bytes)) return -1;
  return with_idx(idtype_bits, [&](auto itag) -> int {
    using Idx = decltype(itag);
    return with_float16(dtype, [&](auto ttag) -> int {
      using T = decltype(ttag);
      const Idx* d = static_cast<const Idx*>(dist);
      const T* go = static_cast<const T*>(grad_out);
      if (want_table) {
        const int rc = with_idx(g.sort_bits(), [&](auto stag) -> int {
          using SI = decltype(stag);
          return gb_backward_table<T, Idx, SI>(who, g, L, scratch.p, d, static_cast<const Idx*>(paths), go,
                                               static_cast<T*>(grad_table), s);
        });
        if (rc) return rc;
      }
      if (grad_spatial) return gb_backward_spatial<T, Idx>(g, L, scratch.p, d, go, padding_idx, static_cast<T*>(grad_spatial), s);
      return 0;
    });
  });
}

}  // extern "C"
