// Biased multi-head attention on the device: the attention of a Graphormer layer, softmax(scale q k^T + bias) v with a
// shared mask and attention dropout, forward and backward, on the operands this library produces: the bias in
// (B, N, N, H) with the heads innermost (dgla_graphormer_bias_forward), the mask (B, N, N) shared by the heads, q, k, v
// as (B, N, H, D) views of (B, N, H * D) projections.  The rule: include/dgl_amd.h "Biased attention".
//
// Reference: python/dgl/nn/pytorch/gt/biased_mha.py composes bmm, four transposes, an in-place add, a masked fill, a
// softmax, a dropout and a second bmm; the (B H, N, N) scores are written and read several times and the bias is read
// through a transpose.  There is no kernel.
//
// MI355X-first choices:
//  * Work split.  A workgroup owns (batch, tile of 32 queries -- or 32 keys in the key-stationary backward --, group of
//    up to four heads); a wavefront owns ONE head of the group.  The (32 x 32 x heads-of-the-group) bias tile is loaded
//    by the whole workgroup, every lane taking the group's consecutive heads of one (query, key) pair, and scattered into
//    LDS as one [stationary][streamed] tile per head; the mask tile is read once per workgroup and folded into that tile
//    as -inf.  Head groups are the fastest grid axis, so the groups that share the lines of a bias span run together.
//  * One tile engine for the three kernels.  The stationary operand (q; k and v in the key-stationary kernel) is kept
//    in registers for the whole loop as the B operand of the MFMA, the streamed 32-row tiles go through the wave's LDS
//    as the A operand, so the score tile is C[streamed][stationary]: a lane holds ONE stationary row (lane % 32) and 16
//    of the 32 streamed rows, rows 8 (r / 4) + 4 (lane / 32) + r % 4 for register r.  In the forward that is the
//    transposed tile k q^T: a query's scores sit in two lanes' registers, so the row maximum and sum are register work
//    and one exchange with lane ^ 32.
//  * Second product.  P feeds the second MFMA straight from those registers as its B operand, without a lane permute
//    or a trip through LDS: a contraction may take its terms in any order, so the k slots of the instruction are given
//    the streamed rows in the order the accumulator layout holds them, and the A operand (v^T, read from the row-major
//    LDS tile element by element) follows the same order.  P is rounded to the operand type for fp16 / bf16
//    (v_mfma_f32_32x32x16) and stays fp32 for fp32 (v_mfma_f32_32x32x2f32).  The output accumulates transposed,
//    O^T[d][query], so the online-softmax rescale is one multiply per register by the lane's own factor.
//  * D is padded with zeros to 32 * ceil(D / 32) in LDS only; steps of the first product past D are skipped.
//  * Rows without a finite score: the running maximum stays -inf, the weights are set to zero instead of
//    exp(-inf - -inf), the output row is zero and the saved log-sum-exp is -inf, from which the backward makes p = 0.
//  * Backward, deterministic, no atomics: delta = sum_d dout out (one small kernel), a key-stationary kernel holding dK
//    and dV in accumulators while it walks the query tiles and writing dbias once through the same LDS tile in the
//    bias's own layout, and a query-stationary kernel for dQ that recomputes ds.
//  * Dropout: gat_dropout.h as it is, row = (b H + h) N + i, block = j / 4, word j % 4.  In the query-stationary kernels
//    one generator call serves four registers; the key-stationary kernel evaluates the same rule once per element.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>

#include "gat_dropout.h"
#include "host_util.h"
#include "mfma_tile.h"

namespace dgla {
namespace {

constexpr int kBaTile = 32;        // rows of a tile: the M and N of the 32 x 32 MFMA
constexpr int kBaMaxWaves = 4;     // heads per workgroup
constexpr int kBaMaxDim = 128;
constexpr int kBaLdsBytes = 65536;  // what a workgroup may take without asking the runtime for more

// The weight exp(s - m) of a score s = hi + lo against a reference m = m_hi + m_lo.  The 16-bit types, whose results
// carry 8 or 11 bits, take the hardware exponential of the rounded difference.  fp32 operands carry the score in two
// parts: one rounding of a score near 8 would alone be a relative error of 2^-22 in its weight, the largest of the whole
// chain.  The difference is formed without a rounding (two-sum), the accurate exponential takes its high part and the
// low part enters to first order.  A score of -inf gives exactly 0 (its low part is then NaN and is not looked at).
template <typename T>
__device__ __forceinline__ float ba_weight(float hi, float lo, float m_hi, float m_lo) {
  if constexpr (std::is_same<T, float>::value) {
    const float d = hi - m_hi, bb = d - hi, err = (hi - (d - bb)) - (m_hi + bb);
    const float ex = expf(d);
    return ex == 0.f ? 0.f : fmaf(ex, err + (lo - m_lo), ex);
  } else {
    return __expf((hi - m_hi) - m_lo);
  }
}
template <typename T>
__device__ __forceinline__ float ba_exp(float x) {
  return std::is_same<T, float>::value ? expf(x) : __expf(x);
}

// Geometry of a (T, NB) instance: D <= 32 NB, LDS rows of RS elements (16 bytes of padding), bias rows of BS.
template <typename T, int NB>
struct BaGeo {
  static constexpr int VEC = 16 / sizeof(T);
  static constexpr int DP = 32 * NB;
  static constexpr int RS = DP + VEC;
  static constexpr int BS = kBaTile + VEC;
  static constexpr int KK = DP / Mma32<T>::KSTEP;      // steps of a product over d
  static constexpr int STEPS = kBaTile / Mma32<T>::KSTEP;  // steps of a product over the 32 streamed rows
  static constexpr int kTileElems = kBaTile * RS;
  static constexpr int kBiasElems = kBaTile * BS;
  static constexpr size_t kWaveBytes = sizeof(T) * (2 * kTileElems + kBiasElems);
};

struct BaArgs {
  const void *q, *k, *v, *bias, *out, *dout;
  const uint8_t* mask;
  float* lse;          // (2, B, H, N): written by the forward, read by the backward
  float* delta;
  void *o, *dq, *dk, *dv, *dbias;
  int64_t B, N, H, D;
  float scale, keep_scale;
  uint32_t threshold;
  uint64_t seed;
  int hg, tiles, groups;  // heads per workgroup, tiles of 32 rows, head groups
  int vec_ok, bias_vec_ok, out_vec_ok;
};

// A 32 x DP tile of a (B, N, H, D) operand into the wave's LDS, zero past `rows` and past D.  `src` is the tile's first
// row at the wave's head; consecutive rows lie `row_stride` elements apart.
template <typename T, int NB>
__device__ __forceinline__ void ba_load_tile(T* lds, const T* __restrict__ src, int64_t row_stride, int rows, int D, bool vec_ok,
                                             int lane) {
  using G = BaGeo<T, NB>;
  using V = VecT<T, G::VEC>;
  constexpr int ppr = G::DP / G::VEC;
  for (int idx = lane; idx < kBaTile * ppr; idx += 64) {
    const int r = idx / ppr, d0 = (idx - r * ppr) * G::VEC;
    const T* p = src + r * row_stride + d0;
    V val;
    if (r < rows && d0 + G::VEC <= D && vec_ok) {
      val = *reinterpret_cast<const V*>(p);
    } else {
#pragma unroll
      for (int k = 0; k < G::VEC; ++k) val.v[k] = r < rows && d0 + k < D ? p[k] : T{};
    }
    *reinterpret_cast<V*>(lds + r * G::RS + d0) = val;
  }
}

// The stationary operand out of an LDS tile: the B fragments of row lane % 32 for every step over d.
template <typename T, int NB>
__device__ __forceinline__ void ba_read_frags(const T* lds, typename Mma32<T>::Raw (&f)[BaGeo<T, NB>::KK], int lane) {
  using G = BaGeo<T, NB>;
  using M = Mma32<T>;
  const T* row = lds + (lane & 31) * G::RS + (lane >> 5) * M::FE;
#pragma unroll
  for (int kk = 0; kk < G::KK; ++kk) f[kk] = *reinterpret_cast<const typename M::Raw*>(row + kk * M::KSTEP);
}

// C[streamed row][stationary row] = sum_d X[streamed][d] S[stationary][d]: X in LDS, S in fragments.
template <typename T, int NB>
__device__ __forceinline__ f32x16 ba_score(const T* xs, const typename Mma32<T>::Raw (&st)[BaGeo<T, NB>::KK], int D, int lane) {
  using G = BaGeo<T, NB>;
  using M = Mma32<T>;
  f32x16 c = mfma_zero();
  const T* row = xs + (lane & 31) * G::RS + (lane >> 5) * M::FE;
#pragma unroll
  for (int kk = 0; kk < G::KK; ++kk)
    if (kk * M::KSTEP < D) c = M::mma(*reinterpret_cast<const typename M::Raw*>(row + kk * M::KSTEP), st[kk], c);
  return c;
}

// acc^T[d][stationary] += sum over the 32 streamed rows of W[streamed][d] * c[streamed][stationary]: c from the
// registers that hold it (rounded to T for the 16-bit types), W element by element from its row-major LDS tile, in the
// order of the streamed rows the registers have.
template <typename T, int NB>
__device__ __forceinline__ void ba_accumulate(f32x16 (&acc)[NB], const T* ws, const f32x16& c, int lane) {
  using G = BaGeo<T, NB>;
  using M = Mma32<T>;
  const int n = lane & 31, g = lane >> 5;
#pragma unroll
  for (int st = 0; st < G::STEPS; ++st) {
    typename M::Raw b;
#pragma unroll
    for (int e = 0; e < M::FE; ++e) M::put(b, e, from_acc<T>(c[st * M::FE + e]));
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      typename M::Raw a;
#pragma unroll
      for (int e = 0; e < M::FE; ++e) M::put(a, e, ws[mfma_c_row(st * M::FE + e, g) * G::RS + nb * 32 + n]);
      acc[nb] = M::mma(a, b, acc[nb]);
    }
  }
}

// acc^T[d][stationary row] to dst[stationary row][d] of a (B, N, H, D) tensor, times `mul`, divided by `div`
template <typename T, int NB>
__device__ __forceinline__ void ba_store_acc(const f32x16 (&acc)[NB], T* __restrict__ dst_row, bool row_ok, int D, float mul, float div,
                                             bool vec_ok, int lane) {
  const int g = lane >> 5;
  if (!row_ok) return;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int d0 = nb * 32 + 8 * r4 + 4 * g;
      VecT<T, 4> val;
#pragma unroll
      for (int e = 0; e < 4; ++e) val.v[e] = from_acc<T>(acc[nb][4 * r4 + e] * mul / div);
      if (vec_ok && d0 + 4 <= D) {
        *reinterpret_cast<VecT<T, 4>*>(dst_row + d0) = val;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (d0 + e < D) dst_row[d0 + e] = val.v[e];
      }
    }
}

// The workgroup's bias tile into LDS, one [stationary][streamed] tile per head of the group, the mask and the pairs
// past N folded in.  KS: the keys are stationary (the tile is stored transposed).  Pair (qi, kj) of the tile is taken
// by one thread, which reads the group's heads as one piece.
template <typename T, bool KS>
__device__ __forceinline__ void ba_stage_bias(T* sb, const BaArgs& a, int64_t b, int q0, int k0, int h0, int bs) {
  const T* bias = static_cast<const T*>(a.bias);
  const int N = static_cast<int>(a.N), H = static_cast<int>(a.H);
  const T ninf = from_acc<T>(-__builtin_huge_valf());
  for (int idx = threadIdx.x; idx < kBaTile * kBaTile; idx += blockDim.x) {
    const int qi = idx >> 5, kj = idx & 31;
    const bool inb = q0 + qi < N && k0 + kj < N;
    const int64_t pair = (b * N + q0 + qi) * N + k0 + kj;
    const bool masked = inb && a.mask && a.mask[pair];
    const int at = KS ? kj * bs + qi : qi * bs + kj;
    VecT<T, kBaMaxWaves> val;
    if (inb && bias && a.bias_vec_ok && a.hg == kBaMaxWaves) {  // (H is a multiple of the group then: no tail)
      val = *reinterpret_cast<const VecT<T, kBaMaxWaves>*>(bias + pair * H + h0);
    } else {
#pragma unroll
      for (int hh = 0; hh < kBaMaxWaves; ++hh)
        val.v[hh] = inb && bias && hh < a.hg && h0 + hh < H ? bias[pair * H + h0 + hh] : T{};
    }
#pragma unroll
    for (int hh = 0; hh < kBaMaxWaves; ++hh)
      if (hh < a.hg) sb[hh * kBaTile * bs + at] = masked ? ninf : val.v[hh];
  }
}

// dbias out of the same LDS tiles, in the bias's own layout: the mirror of ba_stage_bias
template <typename T>
__device__ __forceinline__ void ba_store_dbias(const T* sb, const BaArgs& a, int64_t b, int q0, int k0, int h0, int bs) {
  T* dbias = static_cast<T*>(a.dbias);
  const int N = static_cast<int>(a.N), H = static_cast<int>(a.H);
  for (int idx = threadIdx.x; idx < kBaTile * kBaTile; idx += blockDim.x) {
    const int qi = idx >> 5, kj = idx & 31;
    if (q0 + qi >= N || k0 + kj >= N) continue;
    const int64_t pair = (b * N + q0 + qi) * N + k0 + kj;
    const int at = kj * bs + qi;
    VecT<T, kBaMaxWaves> val;
#pragma unroll
    for (int hh = 0; hh < kBaMaxWaves; ++hh) val.v[hh] = hh < a.hg ? sb[hh * kBaTile * bs + at] : T{};
    if (a.bias_vec_ok && a.hg == kBaMaxWaves) {
      *reinterpret_cast<VecT<T, kBaMaxWaves>*>(dbias + pair * H + h0) = val;
    } else {
#pragma unroll
      for (int hh = 0; hh < kBaMaxWaves; ++hh)
        if (hh < a.hg && h0 + hh < H) dbias[pair * H + h0 + hh] = val.v[hh];
    }
  }
}

// s = scale c + bias tile (the mask is inside it), all 16 registers of the lane.  The 16-bit types round it once;
// fp32 operands keep what that rounding drops in `lo` (an exact product and a two-sum), for ba_weight.
template <typename T, int NB>
__device__ __forceinline__ void ba_add_bias(f32x16& s, f32x16& lo, const T* sbw, bool staged, float scale, int lane) {
#pragma clang fp contract(off)  // (the two-sum needs prod + b as written, not one fused operation)
  using G = BaGeo<T, NB>;
  const int n = lane & 31, g = lane >> 5;
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    VecT<T, 4> bv;
    if (staged) bv = *reinterpret_cast<const VecT<T, 4>*>(sbw + n * G::BS + 8 * r4 + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * r4 + e;
      const float c = s[r], b = staged ? to_acc<T>(bv.v[e]) : 0.f;
      if constexpr (std::is_same<T, float>::value) {
        const float prod = c * scale, perr = fmaf(c, scale, -prod);
        const float hi = prod + b, bb = hi - prod;
        s[r] = hi;
        lo[r] = ((prod - (hi - bb)) + (b - bb)) + perr;
      } else {
        s[r] = staged ? fmaf(c, scale, b) : c * scale;
        lo[r] = 0.f;
      }
    }
  }
}

// keep / (1 - drop) of the four keys 4 * block .. + 3 of query row `row`, as factors
__device__ __forceinline__ void ba_keep4(uint64_t seed, uint64_t row, uint32_t block, uint32_t threshold, float keep_scale,
                                         float (&f)[4]) {
  uint32_t w[4];
  gat_philox4(seed, row, block, w);
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = gat_keep_word(w[e], threshold) ? keep_scale : 0.f;
}

struct BaBlock {
  int64_t b;
  int t, h0;
};
__device__ __forceinline__ BaBlock ba_block(const BaArgs& a) {
  const int64_t x = blockIdx.x;
  const int grp = static_cast<int>(x % a.groups);
  const int64_t rest = x / a.groups;
  return BaBlock{rest / a.tiles, static_cast<int>(rest % a.tiles), grp * a.hg};
}

// ---- forward, and dQ: the query-stationary kernels -----------------------------------------------------------------
// LDS: [waves x (tile X, tile W)][waves x bias tile].
template <typename T, int NB, bool BWD>
__global__ __launch_bounds__(64 * kBaMaxWaves) void ba_query_kernel(const BaArgs a) {
  using G = BaGeo<T, NB>;
  using M = Mma32<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char ba_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, g = lane >> 5;
  const int N = static_cast<int>(a.N), H = static_cast<int>(a.H), D = static_cast<int>(a.D);
  T* xs = reinterpret_cast<T*>(ba_lds) + wave * 2 * G::kTileElems;
  T* ws = xs + G::kTileElems;
  T* sb = reinterpret_cast<T*>(ba_lds) + a.hg * 2 * G::kTileElems;
  const T* sbw = sb + wave * G::kBiasElems;
  const BaBlock blk = ba_block(a);
  const int i0 = blk.t * kBaTile, h = blk.h0 + wave;
  const bool head_ok = h < H;
  const int hc = head_ok ? h : H - 1;  // (a wave past the last head computes on the last one and stores nothing)
  const int64_t row_stride = static_cast<int64_t>(H) * D;
  const int64_t at0 = ((blk.b * N + i0) * H + hc) * D;
  const int qrows = N - i0 < kBaTile ? N - i0 : kBaTile;
  const bool staged = a.bias || a.mask;
  const bool row_ok = head_ok && i0 + n < N;
  const float ninf = -__builtin_huge_valf();

  typename M::Raw qf[G::KK], dof[BWD ? G::KK : 1];
  ba_load_tile<T, NB>(xs, static_cast<const T*>(a.q) + at0, row_stride, qrows, D, a.vec_ok, lane);
  if (BWD) ba_load_tile<T, NB>(ws, static_cast<const T*>(a.dout) + at0, row_stride, qrows, D, a.vec_ok, lane);
  __syncthreads();
  ba_read_frags<T, NB>(xs, qf, lane);
  if constexpr (BWD) ba_read_frags<T, NB>(ws, dof, lane);
  __syncthreads();

  const int64_t stat_row = (blk.b * H + hc) * N + (i0 + n < N ? i0 + n : N - 1);  // the lane's query in (B, H, N)
  const int64_t plane = a.B * a.H * a.N;  // lse[plane + row]: the low-order part of the row's log-sum-exp
  float m = ninf, l = 0.f, lse = ninf, lse_lo = 0.f, delta = 0.f;
  if (BWD) lse = a.lse[stat_row], lse_lo = a.lse[plane + stat_row], delta = a.delta[stat_row];
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma_zero();

  for (int j0 = 0; j0 < N; j0 += kBaTile) {
    const int krows = N - j0 < kBaTile ? N - j0 : kBaTile;
    const int64_t kat = ((blk.b * N + j0) * H + hc) * D;
    if (staged) ba_stage_bias<T, false>(sb, a, blk.b, i0, j0, blk.h0, G::BS);
    ba_load_tile<T, NB>(xs, static_cast<const T*>(a.k) + kat, row_stride, krows, D, a.vec_ok, lane);
    ba_load_tile<T, NB>(ws, static_cast<const T*>(a.v) + kat, row_stride, krows, D, a.vec_ok, lane);
    __syncthreads();

    f32x16 s = ba_score<T, NB>(xs, qf, D, lane);  // s[r]: key j0 + krow(r), query i0 + n
    f32x16 s_lo;
    ba_add_bias<T, NB>(s, s_lo, sbw, staged, a.scale, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (mfma_c_row(r, g) >= krows) s[r] = ninf;

    float keep[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) keep[r] = 1.f;
    if (a.threshold) {
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        float f[4];
        ba_keep4(a.seed, static_cast<uint64_t>(stat_row), static_cast<uint32_t>((j0 + 8 * r4 + 4 * g) >> 2), a.threshold,
                 a.keep_scale, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) keep[4 * r4 + e] = f[e];
      }
    }

    if constexpr (!BWD) {
      float tmax = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m, tmax);
      const bool dead = m_new == ninf;  // no finite score so far: no exp(-inf - -inf)
      const float alpha = dead ? 1.f : ba_exp<T>(m - m_new);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = dead ? 0.f : ba_weight<T>(s[r], s_lo[r], m_new, 0.f);
        psum += p;
        s[r] = p * keep[r];
      }
      psum += __shfl_xor(psum, 32);
      l = l * alpha + psum;
      m = m_new;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] *= alpha;
      ba_accumulate<T, NB>(acc, ws, s, lane);  // O^T += V^T P^T
    } else {
      const f32x16 dp = ba_score<T, NB>(ws, dof, D, lane);  // dP^T[key][query] = sum_d v dout
      const bool dead = lse == ninf;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = dead ? 0.f : ba_weight<T>(s[r], s_lo[r], lse, lse_lo);
        s[r] = p * (keep[r] * dp[r] - delta);
      }
      ba_accumulate<T, NB>(acc, xs, s, lane);  // dQ^T += K^T dS^T
    }
    __syncthreads();
  }

  T* dst = static_cast<T*>(BWD ? a.dq : a.o) + at0 + static_cast<int64_t>(n) * row_stride;
  if constexpr (BWD) {
    ba_store_acc<T, NB>(acc, dst, row_ok, D, a.scale, 1.f, a.out_vec_ok, lane);
  } else {
    const bool zero = !(l > 0.f);
    ba_store_acc<T, NB>(acc, dst, row_ok, D, zero ? 0.f : 1.f, zero ? 1.f : l, a.out_vec_ok, lane);
    if (row_ok && g == 0) {  // m + log l in two fp32 parts: one rounding of it would be the backward's largest error
      float hi = ninf, lo = 0.f;
      if (!zero) {
        const double e = static_cast<double>(m) + log(static_cast<double>(l));
        hi = static_cast<float>(e);
        lo = static_cast<float>(e - static_cast<double>(hi));
      }
      a.lse[stat_row] = hi;
      a.lse[plane + stat_row] = lo;
    }
  }
}

// ---- dK, dV and dbias: the key-stationary kernel -------------------------------------------------------------------
template <typename T, int NB>
__global__ __launch_bounds__(64 * kBaMaxWaves) void ba_key_kernel(const BaArgs a) {
  using G = BaGeo<T, NB>;
  using M = Mma32<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char ba_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, g = lane >> 5;
  const int N = static_cast<int>(a.N), H = static_cast<int>(a.H), D = static_cast<int>(a.D);
  T* xs = reinterpret_cast<T*>(ba_lds) + wave * 2 * G::kTileElems;
  T* ws = xs + G::kTileElems;
  T* sb = reinterpret_cast<T*>(ba_lds) + a.hg * 2 * G::kTileElems;
  T* sbw = sb + wave * G::kBiasElems;
  const BaBlock blk = ba_block(a);
  const int j0 = blk.t * kBaTile, h = blk.h0 + wave;
  const bool head_ok = h < H;
  const int hc = head_ok ? h : H - 1;
  const int64_t row_stride = static_cast<int64_t>(H) * D;
  const int64_t at0 = ((blk.b * N + j0) * H + hc) * D;
  const int krows = N - j0 < kBaTile ? N - j0 : kBaTile;
  const bool staged = a.bias || a.mask;
  const bool key_ok = j0 + n < N;
  const float ninf = -__builtin_huge_valf();

  typename M::Raw kf[G::KK], vf[G::KK];
  ba_load_tile<T, NB>(xs, static_cast<const T*>(a.k) + at0, row_stride, krows, D, a.vec_ok, lane);
  ba_load_tile<T, NB>(ws, static_cast<const T*>(a.v) + at0, row_stride, krows, D, a.vec_ok, lane);
  __syncthreads();
  ba_read_frags<T, NB>(xs, kf, lane);
  ba_read_frags<T, NB>(ws, vf, lane);
  __syncthreads();

  f32x16 dk[NB], dv[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) dk[nb] = mfma_zero(), dv[nb] = mfma_zero();
  const int64_t head_rows = (blk.b * H + hc) * N;  // the head's rows of lse and delta

  for (int i0 = 0; i0 < N; i0 += kBaTile) {
    const int qrows = N - i0 < kBaTile ? N - i0 : kBaTile;
    const int64_t qat = ((blk.b * N + i0) * H + hc) * D;
    if (staged) ba_stage_bias<T, true>(sb, a, blk.b, i0, j0, blk.h0, G::BS);
    ba_load_tile<T, NB>(xs, static_cast<const T*>(a.q) + qat, row_stride, qrows, D, a.vec_ok, lane);
    ba_load_tile<T, NB>(ws, static_cast<const T*>(a.dout) + qat, row_stride, qrows, D, a.vec_ok, lane);
    // lane n carries the statistics of query i0 + n; the registers pick theirs up with a lane read
    const float lse_n = n < qrows ? a.lse[head_rows + i0 + n] : ninf;
    const float lo_n = n < qrows ? a.lse[a.B * a.H * a.N + head_rows + i0 + n] : 0.f;
    const float delta_n = n < qrows ? a.delta[head_rows + i0 + n] : 0.f;
    __syncthreads();

    f32x16 s = ba_score<T, NB>(xs, kf, D, lane);  // s[r]: query i0 + krow(r), key j0 + n
    f32x16 s_lo;
    ba_add_bias<T, NB>(s, s_lo, sbw, staged, a.scale, lane);
    const f32x16 dp = ba_score<T, NB>(ws, vf, D, lane);  // dP[query][key] = sum_d dout v
    f32x16 pd;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = mfma_c_row(r, g);
      const float lse = __shfl(lse_n, qi), lse_lo = __shfl(lo_n, qi), delta = __shfl(delta_n, qi);
      const float p = lse == ninf || !key_ok ? 0.f : ba_weight<T>(s[r], s_lo[r], lse, lse_lo);
      float keep = 1.f;
      if (a.threshold) {
        uint32_t w[4];
        const int j = j0 + n;
        gat_philox4(a.seed, static_cast<uint64_t>(head_rows + i0 + qi), static_cast<uint32_t>(j >> 2), w);
        const int e = j & 3;
        keep = gat_keep_word(e == 0 ? w[0] : e == 1 ? w[1] : e == 2 ? w[2] : w[3], a.threshold) ? a.keep_scale : 0.f;
      }
      pd[r] = p * keep;
      s[r] = p * (keep * dp[r] - delta);
    }
    ba_accumulate<T, NB>(dv, ws, pd, lane);  // dV^T += dout^T (P keep)
    ba_accumulate<T, NB>(dk, xs, s, lane);   // dK^T += Q^T dS
    if (a.dbias) {  // (uniform: every wave reaches the barrier; a wave's own tile is read before it is overwritten)
#pragma unroll
      for (int r = 0; r < 16; ++r) sbw[n * G::BS + mfma_c_row(r, g)] = from_acc<T>(s[r]);
      __syncthreads();
      ba_store_dbias<T>(sb, a, blk.b, i0, j0, blk.h0, G::BS);
    }
    __syncthreads();
  }
  const bool row_ok = head_ok && key_ok;
  const int64_t off = at0 + static_cast<int64_t>(n) * row_stride;
  ba_store_acc<T, NB>(dk, static_cast<T*>(a.dk) + off, row_ok, D, a.scale, 1.f, a.out_vec_ok, lane);
  ba_store_acc<T, NB>(dv, static_cast<T*>(a.dv) + off, row_ok, D, 1.f, 1.f, a.out_vec_ok, lane);
}

// delta[b][h][i] = sum_d dout[b][i][h][d] out[b][i][h][d]: a thread per row
template <typename T>
__global__ __launch_bounds__(256) void ba_delta_kernel(const T* __restrict__ out, const T* __restrict__ dout, int64_t rows, int N,
                                                       int H, int D, float* __restrict__ delta) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;  // (b N + i) H + h
  if (row >= rows) return;
  double sum = 0.0;  // (exact products, one rounding at the store: delta is subtracted from every dP of its row)
  for (int d = 0; d < D; ++d) sum += static_cast<double>(to_acc<T>(out[row * D + d])) * static_cast<double>(to_acc<T>(dout[row * D + d]));
  const int64_t bi = row / H, h = row - bi * H, b = bi / N, i = bi - b * N;
  delta[(b * H + h) * N + i] = static_cast<float>(sum);
}

// ---- host side -------------------------------------------------------------------------------------------------------
template <typename F>
int with_ba_width(int64_t D, F&& f) {
  if (D <= 32) return f(std::integral_constant<int, 1>{});
  if (D <= 64) return f(std::integral_constant<int, 2>{});
  if (D <= 96) return f(std::integral_constant<int, 3>{});
  return f(std::integral_constant<int, 4>{});
}

// BaGeo<T, NB>::kWaveBytes of the instance that dtype and D select
size_t ba_wave_bytes(int dtype, int64_t D) {
  const size_t item = float_itemsize(dtype), vec = 16 / item, dp = static_cast<size_t>((D + 31) / 32 * 32);
  return item * (2 * kBaTile * (dp + vec) + kBaTile * (kBaTile + vec));
}

// What forward and backward open with: the arguments they share into `a`, everything they refuse about the sizes and
// the rate, the geometry of the launch.
int check_ba(const char* who, int dtype, const void* q, const void* k, const void* v, const void* bias, const void* mask, int64_t B,
             int64_t N, int64_t H, int64_t D, float scale, float drop, uint64_t seed, BaArgs* a) {
  a->q = q, a->k = k, a->v = v, a->bias = bias, a->mask = static_cast<const uint8_t*>(mask);
  a->B = B, a->N = N, a->H = H, a->D = D, a->scale = scale, a->seed = seed;
  if (check_float16(who, dtype, "operands")) return -1;
  if (B < 0 || N < 1 || H < 1) return fail(who, "q, k, v must be (B, N, H, D) with N >= 1 and H >= 1");
  if (D < 1 || D > kBaMaxDim)
    return fail(who, "head width " + std::to_string(D) + ": the kernels take 1 to " + std::to_string(kBaMaxDim));
  if (!gat_dropout_params(drop, &a->threshold, &a->keep_scale)) return fail(who, "the dropout probability must lie in [0, 1)");
  if (N > INT32_MAX / 2 || H > INT32_MAX / 2) return fail(who, "sizes overflow");
  int hg = static_cast<int>(kBaLdsBytes / ba_wave_bytes(dtype, D));
  hg = hg > kBaMaxWaves ? kBaMaxWaves : hg;
  hg = hg > H ? static_cast<int>(H) : hg;
  a->hg = hg;
  a->tiles = static_cast<int>((N + kBaTile - 1) / kBaTile);
  a->groups = static_cast<int>((H + hg - 1) / hg);
  if (B > 0 && B > INT32_MAX / a->tiles / a->groups) return fail(who, "more workgroups than one launch takes");
  return 0;
}

template <typename T>
void ba_vector_flags(BaArgs* a) {
  constexpr int VEC = 16 / sizeof(T);
  a->vec_ok = a->D % VEC == 0 && aligned_to(a->q, 16) && aligned_to(a->k, 16) && aligned_to(a->v, 16) &&
              (!a->dout || aligned_to(a->dout, 16));
  const size_t four = 4 * sizeof(T);
  a->out_vec_ok = a->D % 4 == 0 && (!a->o || aligned_to(a->o, four)) && (!a->dq || aligned_to(a->dq, four)) &&
                  (!a->dk || aligned_to(a->dk, four)) && (!a->dv || aligned_to(a->dv, four));
  a->bias_vec_ok = a->H % kBaMaxWaves == 0 && (!a->bias || aligned_to(a->bias, four)) && (!a->dbias || aligned_to(a->dbias, four));
}

// The launch of the three tile kernels of a (T, NB) instance: a workgroup per (batch, tile, head group), a wavefront
// and kWaveBytes of LDS per head of the group.
struct BaLaunch {
  dim3 grid, block;
  size_t lds;
};
template <typename T, int NB>
BaLaunch ba_launch(const BaArgs& a) {
  return BaLaunch{dim3(static_cast<unsigned>(a.B * a.tiles * a.groups)), dim3(static_cast<unsigned>(64 * a.hg)),
                  BaGeo<T, NB>::kWaveBytes * a.hg};
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_biased_attention_workspace_bytes(int64_t B, int64_t N, int64_t H) {
  if (B < 0 || N < 1 || H < 1 || B > INT64_MAX / 4 / N / H) return 0;
  return align256(sizeof(float) * static_cast<size_t>(B * N * H));
}

int dgla_biased_attention_forward(int dtype, const void* q, const void* k, const void* v, const void* bias, const void* mask,
                                  int64_t B, int64_t N, int64_t H, int64_t D, float scale, float drop, uint64_t seed, void* out,
                                  float* lse, void* hip_stream) {
  const char* who = "biased_attention";
  BaArgs a{};
  a.o = out, a.lse = lse;
  if (check_ba(who, dtype, q, k, v, bias, mask, B, N, H, D, scale, drop, seed, &a)) return -1;
  if (B == 0) return 0;
  if (!q || !k || !v || !out || !lse) return fail(who, "q, k, v, out or lse is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  return with_float16(dtype, [&](auto ttag) -> int {
    using T = decltype(ttag);
    ba_vector_flags<T>(&a);
    return with_ba_width(D, [&](auto ntag) -> int {
      constexpr int NB = decltype(ntag)::value;
      const BaLaunch l = ba_launch<T, NB>(a);
      hipLaunchKernelGGL((ba_query_kernel<T, NB, false>), l.grid, l.block, l.lds, s, a);
      DGLA_CHECK_HIP(hipGetLastError());
      return 0;
    });
  });
}

int dgla_biased_attention_backward(int dtype, const void* q, const void* k, const void* v, const void* bias, const void* mask,
                                   const void* out, const float* lse, const void* dout, int64_t B, int64_t N, int64_t H, int64_t D,
                                   float scale, float drop, uint64_t seed, void* dq, void* dk, void* dv, void* dbias,
                                   void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "biased_attention";
  BaArgs a{};
  a.out = out, a.dout = dout, a.lse = const_cast<float*>(lse), a.dq = dq, a.dk = dk, a.dv = dv, a.dbias = dbias;
  if (check_ba(who, dtype, q, k, v, bias, mask, B, N, H, D, scale, drop, seed, &a)) return -1;
  if (B == 0) return 0;
  if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv) return fail(who, "an operand or a gradient of q, k, v is null");
  const size_t need = dgla_biased_attention_workspace_bytes(B, N, H);
  if (optional_workspace(who, workspace, workspace_bytes, need)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, dq);
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, need)) return -1;
  a.delta = reinterpret_cast<float*>(scratch.p);
  return with_float16(dtype, [&](auto ttag) -> int {
    using T = decltype(ttag);
    ba_vector_flags<T>(&a);
    const int64_t rows = B * N * H;
    hipLaunchKernelGGL(ba_delta_kernel<T>, dim3(grid1(rows, 256)), dim3(256), 0, s, static_cast<const T*>(out),
                       static_cast<const T*>(dout), rows, static_cast<int>(N), static_cast<int>(H), static_cast<int>(D), a.delta);
    return with_ba_width(D, [&](auto ntag) -> int {
      constexpr int NB = decltype(ntag)::value;
      const BaLaunch l = ba_launch<T, NB>(a);
      hipLaunchKernelGGL((ba_key_kernel<T, NB>), l.grid, l.block, l.lds, s, a);
      hipLaunchKernelGGL((ba_query_kernel<T, NB, true>), l.grid, l.block, l.lds, s, a);
      DGLA_CHECK_HIP(hipGetLastError());
      return 0;
    });
  });
}

int dgla_biased_attention_dropout_mask_host(uint64_t seed, float drop, int64_t B, int64_t H, int64_t N, uint8_t* keep) {
  const char* who = "biased_attention";
  uint32_t threshold;
  float keep_scale;
  if (!gat_dropout_params(drop, &threshold, &keep_scale)) return fail(who, "the dropout probability must lie in [0, 1)");
  if (B < 0 || H < 1 || N < 1 || (B > 0 && !keep)) return fail(who, "the mask is (B, H, N, N) with H >= 1 and N >= 1");
  for (int64_t row = 0; row < B * H * N; ++row)
    for (int64_t j0 = 0; j0 < N; j0 += 4) {
      uint32_t w[4] = {~0u, ~0u, ~0u, ~0u};
      if (threshold) gat_philox4(seed, static_cast<uint64_t>(row), static_cast<uint32_t>(j0 >> 2), w);
      for (int e = 0; e < 4 && j0 + e < N; ++e) keep[row * N + j0 + e] = gat_keep_word(w[e], threshold) ? 1 : 0;
    }
  return 0;
}

}  // extern "C"
