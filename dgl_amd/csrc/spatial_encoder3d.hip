// 3D spatial encoding on the device: the attention bias of the 3D (molecular) Graphormer, forward and backward.  For
// every pair of nodes: the Euclidean distance, a node-type-dependent affine map, K Gaussian basis functions,
// Linear(K, K) -> GELU -> Linear(K, H), into the (B, N, N, H) layout dgla_biased_attention_forward consumes.  The
// rule: include/dgl_amd.h "3D spatial encoding".
//
// Reference: python/dgl/nn/pytorch/gt/spatial_encoder.py:136-209 composes cdist, two embedding gathers over (B, N, N, 2)
// ids, the Gaussian, two linears and a GELU: three (B N N, K) tensors are written, read and kept for the backward.
// There is no kernel.
//
// MI355X-first choices:
//  * Work split.  Persistent workgroups of NB = ceil(K / 32) (1, 2 or 4) wavefronts walk tiles of 32 consecutive pairs;
//    a tile's output is one contiguous run of 32 H elements.  Wave w owns the columns [32 w, 32 w + 32) of the hidden
//    layer.  Both weight matrices are stationary: every wave keeps its slice of W1 and of W2 as MFMA A fragments in
//    registers for the whole loop, so nothing but coordinates (and dout) is read per tile.
//  * Features.  Thread t owns ONE basis function k = t % (32 NB) (mean, 1 / sd and the normaliser in registers) and 16
//    of the tile's 32 pairs.  Distance, affine map, exp and the feature are fp32; the feature is rounded to the operand
//    type only as it enters LDS, [pair][k], K zero-padded to 32 NB there and nowhere else.
//  * Layer 1 runs TRANSPOSED, z^T[hidden][pair] = W1 g^T (v_mfma_f32_32x32x16_{bf16,f16}, v_mfma_f32_32x32x2_f32), so
//    a lane holds ONE pair (lane % 32) and 16 hidden units, rows 8 (r / 4) + 4 (lane / 32) + r % 4 of the wave's slice.
//    Bias and GELU are register work.  Layer 2, out^T[head][pair] = W2 h^T, takes h straight from those registers as
//    its B operand, without a trip through LDS: a contraction may take its terms in any order, so the k slots of the
//    instruction get the hidden units in the order the accumulator holds them and the W2 fragments were loaded in
//    that order.  The NB partial products meet in LDS ([wave][head][pair], fp32), are summed in wave order, get b2 and
//    leave in 16-byte pieces.
//  * Backward, deterministic, no atomics.  g, z and h are recomputed per tile.  dh^T = W2^T dout^T and dz^T = dh^T
//    gelu'(z) in the same lane layout; h and dz go to LDS once ([pair][hidden]); dg^T = W1^T dz^T (wave w owns the
//    basis functions [32 w, 32 w + 32)), from which dx of the pair and the terms of dmeans / dstds are register work.
//    dW1 += dz^T g and dW2 += dout^T h contract over the PAIRS: their operands are the same LDS tiles read down the
//    columns, and the sums stay in accumulators across all tiles of the workgroup.  Every workgroup writes one partial
//    of the parameter sums; se_reduce_kernel adds the partials in workgroup order (fp64).  dx goes to the workspace,
//    one fp32 per pair, and se_pair_kernel forms the row and column sums for the four per-node vectors.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>

#include "host_util.h"
#include "mfma_tile.h"

namespace dgla {
namespace {

constexpr int kSeTile = 32;       // pairs of a tile: the N of the 32 x 32 MFMA
constexpr int kSeMaxK = 128;
constexpr int kSeMaxH = 64;
constexpr int kSeFwdGroups = 512;  // persistent workgroups of the forward: two per compute unit of an MI355X
constexpr int kSeBwdGroups = 256;  // of the backward (one per compute unit: its registers leave room for no more)
constexpr int kSePartPad = kSeTile + 1;  // row of the [wave][head][pair] partial tile

// Geometry of a (T, NB, HB) instance: K <= 32 NB, H <= 32 HB, LDS rows padded by 16 bytes.
template <typename T, int NB, int HB>
struct SeGeo {
  using M = Mma32<T>;
  static constexpr int VEC = 16 / sizeof(T);
  static constexpr int KP = 32 * NB, HP = 32 * HB;
  static constexpr int RS = KP + VEC;  // row of a [pair][K] tile
  static constexpr int RO = HP + VEC;  // row of the [pair][H] tile of dout
  static constexpr int KK = KP / M::KSTEP, HK = HP / M::KSTEP, MK = kSeTile / M::KSTEP;  // steps over K, H, the pairs
  static constexpr int THREADS = 64 * NB;
  static constexpr int ROWS_PER_THREAD = kSeTile * KP / THREADS;  // 16: the pairs a thread makes its feature of
};

struct SeArgs {
  const float *coord, *gs, *gt, *bs, *bt, *means, *stds;
  const void *w1, *b1, *w2, *b2, *dout;
  void* out;
  float *dx, *part;  // the backward's workspace: dx per pair, one partial of the parameter sums per workgroup
  int64_t N, pairs, tiles;
  int K, H, out_vec_ok;
};

// A fragment out of an LDS tile whose rows are the operand's rows: elements k0 .. k0 + FE of row `row` (one read)
template <typename T>
__device__ __forceinline__ typename Mma32<T>::Raw se_frag_rows(const T* lds, int row, int k0, int rs) {
  return *reinterpret_cast<const typename Mma32<T>::Raw*>(lds + row * rs + k0);
}

// A fragment of the TRANSPOSED tile: the contraction runs down the LDS rows k0 .. k0 + FE, the operand's row is the LDS
// column `col` (consecutive lanes read consecutive addresses)
template <typename T>
__device__ __forceinline__ typename Mma32<T>::Raw se_frag_cols(const T* lds, int col, int k0, int rs) {
  using M = Mma32<T>;
  typename M::Raw f;
#pragma unroll
  for (int e = 0; e < M::FE; ++e) M::put(f, e, lds[(k0 + e) * rs + col]);
  return f;
}

// A stationary fragment out of global memory, element by element, once per workgroup: row `row` of a (rows x cols)
// operand whose element (row, k) lies at src[row * row_stride + k * k_stride]; zero outside.
template <typename T>
__device__ __forceinline__ typename Mma32<T>::Raw se_frag_global(const T* __restrict__ src, int row, int rows, int k0, int cols,
                                                                 int row_stride, int k_stride) {
  using M = Mma32<T>;
  typename M::Raw f;
#pragma unroll
  for (int e = 0; e < M::FE; ++e) M::put(f, e, row < rows && k0 + e < cols ? src[row * row_stride + (k0 + e) * k_stride] : T{});
  return f;
}

// x = (gs_i + gt_j) d + (bs_i + bt_j) of pair p = (b N + i) N + j, d the distance of the two nodes from exact differences.
// Every operation is rounded as the rule writes it, none fused: a rounding of x is magnified t / sd times in the feature
// and dominates the error of dmeans, so the backward and the torch composition must see the x the forward saw.
__device__ __forceinline__ float se_pair_x(const SeArgs& a, int64_t p) {
#pragma clang fp contract(off)
  const int64_t nn = a.N * a.N, b = p / nn, rem = p - b * nn, i = rem / a.N, j = rem - i * a.N;
  const int64_t ni = b * a.N + i, nj = b * a.N + j;
  const float dx = a.coord[3 * ni] - a.coord[3 * nj], dy = a.coord[3 * ni + 1] - a.coord[3 * nj + 1],
              dz = a.coord[3 * ni + 2] - a.coord[3 * nj + 2];
  const float d = sqrtf((dx * dx + dz * dz) + dy * dy);
  return (a.gs[ni] + a.gt[nj]) * d + (a.bs[ni] + a.bt[nj]);
}

// The constants of basis function k: mean, sd, 1 / sd, the normaliser sqrt(2 * 3.14159) sd (the reference's constant) and
// its reciprocal; a padded k gives the feature 0.  fp32 weights take the rule's two divisions as they are written: the
// rounding of t = (x - mean) / sd is magnified t^2 times in exp(-t^2 / 2), and a reciprocal and a product would round
// it twice more.  The 16-bit types, whose feature is rounded to 8 or 11 bits, multiply by the reciprocals.
struct SeBasis {
  float mean, sd, isd, norm, coef;
};
__device__ __forceinline__ SeBasis se_basis(const SeArgs& a, int k) {
  if (k >= a.K) return SeBasis{0.f, 1.f, 0.f, __builtin_huge_valf(), 0.f};
  const float sd = fabsf(a.stds[k]) + 1e-2f, norm = static_cast<float>(2.5066272160016134) * sd;
  return SeBasis{a.means[k], sd, 1.f / sd, norm, 1.f / norm};
}
template <typename T>
__device__ __forceinline__ float se_gauss(const SeBasis& bf, float x, float* t_out) {
  if constexpr (std::is_same<T, float>::value) {
    const float t = (x - bf.mean) / bf.sd;
    *t_out = t;
    return expf(-0.5f * t * t) / bf.norm;
  } else {
    const float t = (x - bf.mean) * bf.isd;
    *t_out = t;
    return __expf(-0.5f * t * t) * bf.coef;
  }
}

// The tile's features into LDS, [pair][k] in the operand type: the thread's one basis function for its 16 pairs.
template <typename T, int NB, int HB>
__device__ __forceinline__ void se_features(T* gl, const float* xs, const SeBasis& bf) {
  using G = SeGeo<T, NB, HB>;
  const int k = threadIdx.x % G::KP, m0 = threadIdx.x / G::KP;  // (THREADS = 2 KP: m0 is 0 or 1)
#pragma unroll
  for (int i = 0; i < G::ROWS_PER_THREAD; ++i) {
    const int m = m0 + 2 * i;
    float t;
    gl[m * G::RS + k] = from_acc<T>(se_gauss<T>(bf, xs[m], &t));
  }
}

// z^T[hidden][pair] = W1 g^T of the wave's 32 hidden units, plus b1: the lane's pair is lane % 32, register r holds the
// hidden unit 32 wave + mfma_c_row(r, lane / 32).
template <typename T, int NB, int HB>
__device__ __forceinline__ f32x16 se_layer1(const typename Mma32<T>::Raw (&w1f)[SeGeo<T, NB, HB>::KK], const T* gl, const float (&b1r)[16],
                                            int K, int lane) {
  using G = SeGeo<T, NB, HB>;
  using M = Mma32<T>;
  f32x16 c = mfma_zero();
#pragma unroll
  for (int kk = 0; kk < G::KK; ++kk)
    if (kk * M::KSTEP < K) c = M::mma(w1f[kk], se_frag_rows<T>(gl, lane & 31, kk * M::KSTEP + (lane >> 5) * M::FE, G::RS), c);
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] += b1r[r];
  return c;
}

__device__ __forceinline__ float se_gelu(float z, float* slope) {
  const float cdf = 0.5f * (1.f + erff(z * 0.70710678f));
  *slope = cdf + z * 0.39894228f * expf(-0.5f * z * z);  // d gelu / dz: Phi(z) + z phi(z)
  return z * cdf;
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <typename T, int NB, int HB>
__global__ __launch_bounds__(64 * NB) void se_forward_kernel(const SeArgs a) {
  using G = SeGeo<T, NB, HB>;
  using M = Mma32<T>;
  __shared__ __attribute__((aligned(16))) T gl[kSeTile * G::RS];
  __shared__ float part[NB * G::HP * kSePartPad];
  __shared__ float xs[kSeTile], b2s[G::HP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, g = lane >> 5;
  const int K = a.K, H = a.H;
  const T* w1 = static_cast<const T*>(a.w1);
  const T* w2 = static_cast<const T*>(a.w2);

  // the stationary operands: W1 rows of the wave's hidden units; W2 with its hidden units in accumulator order
  typename M::Raw w1f[G::KK], w2f[HB][G::MK];
#pragma unroll
  for (int kk = 0; kk < G::KK; ++kk) w1f[kk] = se_frag_global<T>(w1, 32 * wave + n, K, kk * M::KSTEP + g * M::FE, K, K, 1);
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int st = 0; st < G::MK; ++st)
#pragma unroll
      for (int e = 0; e < M::FE; ++e) {
        const int hh = 32 * hb + n, ko = 32 * wave + mfma_c_row(st * M::FE + e, g);
        M::put(w2f[hb][st], e, hh < H && ko < K ? w2[hh * K + ko] : T{});
      }
  float b1r[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ko = 32 * wave + mfma_c_row(r, g);
    b1r[r] = ko < K ? to_acc<T>(static_cast<const T*>(a.b1)[ko]) : 0.f;
  }
  for (int hh = threadIdx.x; hh < G::HP; hh += G::THREADS) b2s[hh] = hh < H ? to_acc<T>(static_cast<const T*>(a.b2)[hh]) : 0.f;
  const SeBasis bf = se_basis(a, threadIdx.x % G::KP);
  T* out = static_cast<T*>(a.out);

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t p0 = tile * kSeTile;
    if (threadIdx.x < kSeTile) {  // (a pair past the end computes on the last one and is not stored)
      const int64_t p = p0 + threadIdx.x;
      xs[threadIdx.x] = se_pair_x(a, p < a.pairs ? p : a.pairs - 1);
    }
    __syncthreads();
    se_features<T, NB, HB>(gl, xs, bf);
    __syncthreads();

    f32x16 h = se_layer1<T, NB, HB>(w1f, gl, b1r, K, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float slope;
      h[r] = se_gelu(h[r], &slope);
    }
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
      f32x16 o = mfma_zero();
#pragma unroll
      for (int st = 0; st < G::MK; ++st) {
        typename M::Raw b;
#pragma unroll
        for (int e = 0; e < M::FE; ++e) M::put(b, e, from_acc<T>(h[st * M::FE + e]));
        o = M::mma(w2f[hb][st], b, o);  // o[r]: head 32 hb + mfma_c_row(r, g), pair n, the wave's share of the sum
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) part[(wave * G::HP + 32 * hb + mfma_c_row(r, g)) * kSePartPad + n] = o[r];
    }
    __syncthreads();

    // the tile's run of the output: 32 H consecutive elements (fewer in the last tile), VEC of them per thread and turn
    const int64_t left = a.pairs - p0;
    const int total = (left < kSeTile ? static_cast<int>(left) : kSeTile) * H;
    for (int e0 = threadIdx.x * G::VEC; e0 < total; e0 += G::THREADS * G::VEC) {
      VecT<T, G::VEC> val;
#pragma unroll
      for (int e = 0; e < G::VEC; ++e) {
        const int idx = e0 + e < total ? e0 + e : total - 1, m = idx / H, hh = idx - m * H;
        float sum = part[hh * kSePartPad + m];
#pragma unroll
        for (int w = 1; w < NB; ++w) sum += part[(w * G::HP + hh) * kSePartPad + m];
        val.v[e] = from_acc<T>(sum + b2s[hh]);
      }
      T* dst = out + p0 * H + e0;
      if (a.out_vec_ok && e0 + G::VEC <= total) {
        *reinterpret_cast<VecT<T, G::VEC>*>(dst) = val;
      } else {
#pragma unroll
        for (int e = 0; e < G::VEC; ++e)
          if (e0 + e < total) dst[e] = val.v[e];
      }
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// The floats of one workgroup's partial: dW1 (K, K), dW2 (H, K), db1, dmeans, dstds (K each), db2 (H).
__host__ __device__ inline int64_t se_part_floats(int64_t K, int64_t H) { return K * K + H * K + 3 * K + H; }

// sum over the 32 lanes that share lane / 32 (the pairs of a tile), left in every one of them
__device__ __forceinline__ float se_sum_pairs(float v) {
#pragma unroll
  for (int s = 1; s < 32; s <<= 1) v += __shfl_xor(v, s);
  return v;
}

template <typename T, int NB, int HB>
__global__ __launch_bounds__(64 * NB) void se_backward_kernel(const SeArgs a) {
  using G = SeGeo<T, NB, HB>;
  using M = Mma32<T>;
  __shared__ __attribute__((aligned(16))) T gl[kSeTile * G::RS];   // features  [pair][k]
  __shared__ __attribute__((aligned(16))) T hl[kSeTile * G::RS];   // h         [pair][hidden]
  __shared__ __attribute__((aligned(16))) T zl[kSeTile * G::RS];   // dz        [pair][hidden]
  __shared__ __attribute__((aligned(16))) T dol[kSeTile * G::RO];  // dout      [pair][head], zero past H and past the end
  __shared__ float xs[kSeTile], dxp[NB * kSeTile];
  __shared__ SeBasis basis[G::KP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, g = lane >> 5;
  const int K = a.K, H = a.H;
  const T* w1 = static_cast<const T*>(a.w1);
  const T* w2 = static_cast<const T*>(a.w2);
  const T* dout = static_cast<const T*>(a.dout);

  // stationary: W1 by rows (layer 1), W1 by columns (dg = dz W1), W2 by columns (dh = dout W2)
  typename M::Raw w1f[G::KK], w1tf[G::KK], w2tf[G::HK];
#pragma unroll
  for (int kk = 0; kk < G::KK; ++kk) {
    w1f[kk] = se_frag_global<T>(w1, 32 * wave + n, K, kk * M::KSTEP + g * M::FE, K, K, 1);
    w1tf[kk] = se_frag_global<T>(w1, 32 * wave + n, K, kk * M::KSTEP + g * M::FE, K, 1, K);
  }
#pragma unroll
  for (int st = 0; st < G::HK; ++st) w2tf[st] = se_frag_global<T>(w2, 32 * wave + n, K, st * M::KSTEP + g * M::FE, H, 1, K);
  float b1r[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ko = 32 * wave + mfma_c_row(r, g);
    b1r[r] = ko < K ? to_acc<T>(static_cast<const T*>(a.b1)[ko]) : 0.f;
  }
  const SeBasis bf = se_basis(a, threadIdx.x % G::KP);
  if (threadIdx.x < G::KP) basis[threadIdx.x] = bf;

  f32x16 dw1[NB], dw2[HB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) dw1[nb] = mfma_zero();
#pragma unroll
  for (int hb = 0; hb < HB; ++hb) dw2[hb] = mfma_zero();
  float db1a[16], dma[16], dsa[16], db2a = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) db1a[r] = 0.f, dma[r] = 0.f, dsa[r] = 0.f;

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t p0 = tile * kSeTile, left = a.pairs - p0;
    const int rows = left < kSeTile ? static_cast<int>(left) : kSeTile;
    if (threadIdx.x < kSeTile) {
      const int64_t p = p0 + threadIdx.x;
      xs[threadIdx.x] = se_pair_x(a, p < a.pairs ? p : a.pairs - 1);
    }
    for (int idx = threadIdx.x; idx < kSeTile * G::HP; idx += G::THREADS) {
      const int m = idx / G::HP, hh = idx % G::HP;
      dol[m * G::RO + hh] = m < rows && hh < H ? dout[(p0 + m) * H + hh] : T{};
    }
    __syncthreads();
    se_features<T, NB, HB>(gl, xs, bf);
    if (threadIdx.x < H) {  // db2 += the column sums of the tile of dout
      float s = 0.f;
#pragma unroll 8
      for (int m = 0; m < kSeTile; ++m) s += to_acc<T>(dol[m * G::RO + threadIdx.x]);
      db2a += s;
    }
    __syncthreads();

    // the lane's pair n and its 16 hidden units: z, h, gelu'(z); dh = dout W2; dz = dh gelu'(z)
    f32x16 z = se_layer1<T, NB, HB>(w1f, gl, b1r, K, lane);
    f32x16 dh = mfma_zero();
#pragma unroll
    for (int st = 0; st < G::HK; ++st)
      if (st * M::KSTEP < H) dh = M::mma(w2tf[st], se_frag_rows<T>(dol, n, st * M::KSTEP + g * M::FE, G::RO), dh);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      VecT<T, 4> hv, zv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * r4 + e;
        float slope;
        const float h = se_gelu(z[r], &slope), dz = dh[r] * slope;
        db1a[r] += dz;
        hv.v[e] = from_acc<T>(h);
        zv.v[e] = from_acc<T>(dz);
      }
      const int at = n * G::RS + 32 * wave + 8 * r4 + 4 * g;
      *reinterpret_cast<VecT<T, 4>*>(hl + at) = hv;
      *reinterpret_cast<VecT<T, 4>*>(zl + at) = zv;
    }
    __syncthreads();

    // dg^T[k][pair] = W1^T dz^T for the wave's 32 basis functions k; dx of the pair and the terms of dmeans and dstds
    f32x16 dg = mfma_zero();
#pragma unroll
    for (int kk = 0; kk < G::KK; ++kk)
      if (kk * M::KSTEP < K) dg = M::mma(w1tf[kk], se_frag_rows<T>(zl, n, kk * M::KSTEP + g * M::FE, G::RS), dg);
    const float x = xs[n];
    float dxl = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = 32 * wave + mfma_c_row(r, g);
      const SeBasis bk = basis[k];
      float t;
      const float u = dg[r] * se_gauss<T>(bk, x, &t) * bk.isd;  // dg g / sd
      dxl -= u * t;                                               // dg/dx = -g t / sd
      dma[r] += u * t;                                            // dg/dmean = g t / sd
      dsa[r] += u * (t * t - 1.f);                                // dg/dsd = g (t^2 - 1) / sd
    }
    dxl += __shfl_xor(dxl, 32);
    if (g == 0) dxp[wave * kSeTile + n] = dxl;

    // dW1[hidden][k] += sum over the pairs of dz g;  dW2[head][hidden] += sum over the pairs of dout h
#pragma clang loop unroll_count(G::MK < 4 ? G::MK : 2)  //(the 16 fp32 steps stay a loop: unrolled, their LDS reads crowd out the sums)
    for (int st = 0; st < G::MK; ++st) {
      const int m0 = st * M::KSTEP + g * M::FE;
      const typename M::Raw zf = se_frag_cols<T>(zl, 32 * wave + n, m0, G::RS);
      const typename M::Raw hf = se_frag_cols<T>(hl, 32 * wave + n, m0, G::RS);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (32 * nb < K) dw1[nb] = M::mma(zf, se_frag_cols<T>(gl, 32 * nb + n, m0, G::RS), dw1[nb]);
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) dw2[hb] = M::mma(se_frag_cols<T>(dol, 32 * hb + n, m0, G::RO), hf, dw2[hb]);
    }
    __syncthreads();
    if (threadIdx.x < rows) {
      float s = dxp[threadIdx.x];
#pragma unroll
      for (int w = 1; w < NB; ++w) s += dxp[w * kSeTile + threadIdx.x];
      a.dx[p0 + threadIdx.x] = s;
    }
  }

  // the workgroup's partial
  float* part = a.part + static_cast<int64_t>(blockIdx.x) * se_part_floats(K, H);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // dw1[nb][r]: hidden 32 wave + mfma_c_row(r, g), basis function 32 nb + n
      const int ko = 32 * wave + mfma_c_row(r, g), k = 32 * nb + n;
      if (ko < K && k < K) part[ko * K + k] = dw1[nb][r];
    }
  part += K * K;
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // dw2[hb][r]: head 32 hb + mfma_c_row(r, g), hidden 32 wave + n
      const int hh = 32 * hb + mfma_c_row(r, g), ko = 32 * wave + n;
      if (hh < H && ko < K) part[hh * K + ko] = dw2[hb][r];
    }
  part += H * K;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float s1 = se_sum_pairs(db1a[r]), sm = se_sum_pairs(dma[r]), ss = se_sum_pairs(dsa[r]);
    const int k = 32 * wave + mfma_c_row(r, g);
    if (n == 0 && k < K) part[k] = s1, part[K + k] = sm, part[2 * K + k] = ss;
  }
  if (threadIdx.x < H) part[3 * K + threadIdx.x] = db2a;
}

// The partials of `groups` workgroups added in workgroup order, a thread per element; dstds gets the sign of stds.
template <typename T>
__global__ __launch_bounds__(256) void se_reduce_kernel(const float* __restrict__ part, int groups, int K, int H,
                                                        const float* __restrict__ stds, T* __restrict__ dw1, T* __restrict__ db1,
                                                        T* __restrict__ dw2, T* __restrict__ db2, float* __restrict__ dmeans,
                                                        float* __restrict__ dstds) {
  const int64_t len = se_part_floats(K, H);
  const int64_t at = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (at >= len) return;
  double sum = 0.0;
  for (int p = 0; p < groups; ++p) sum += static_cast<double>(part[p * len + at]);
  const float v = static_cast<float>(sum);
  int64_t e = at;
  if (e < K * K) {
    dw1[e] = from_acc<T>(v);
  } else if ((e -= K * K) < H * K) {
    dw2[e] = from_acc<T>(v);
  } else if ((e -= H * K) < K) {
    db1[e] = from_acc<T>(v);
  } else if ((e -= K) < K) {
    dmeans[e] = v;
  } else if ((e -= K) < K) {
    const float s = stds[e];
    dstds[e] = s > 0.f ? v : s < 0.f ? -v : 0.f;
  } else {
    db2[e - K] = from_acc<T>(v);
  }
}

// The per-node gradients from dx: a wavefront per node (b, i) sums row i (dgs, dbs) and column i (dgt, dbt) of batch b,
// lane by lane and then across the lanes, always in the same order; d is recomputed from coord.
__global__ __launch_bounds__(64) void se_pair_kernel(const float* __restrict__ coord, const float* __restrict__ dx, int64_t N,
                                                     float* __restrict__ dgs, float* __restrict__ dgt, float* __restrict__ dbs,
                                                     float* __restrict__ dbt) {
  const int64_t node = blockIdx.x, b = node / N, i = node - b * N;
  const float cx = coord[3 * node], cy = coord[3 * node + 1], cz = coord[3 * node + 2];
  double rg = 0.0, rb = 0.0, cg = 0.0, cb = 0.0;
  for (int64_t j = threadIdx.x; j < N; j += 64) {
    const int64_t other = b * N + j;
    const float ex = cx - coord[3 * other], ey = cy - coord[3 * other + 1], ez = cz - coord[3 * other + 2];
    const double d = static_cast<double>(sqrtf(ex * ex + ey * ey + ez * ez));
    const double row = static_cast<double>(dx[node * N + j]), col = static_cast<double>(dx[other * N + i]);
    rg += row * d, rb += row, cg += col * d, cb += col;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) rg += __shfl_xor(rg, s), rb += __shfl_xor(rb, s), cg += __shfl_xor(cg, s), cb += __shfl_xor(cb, s);
  if (threadIdx.x == 0) {
    dgs[node] = static_cast<float>(rg), dbs[node] = static_cast<float>(rb);
    dgt[node] = static_cast<float>(cg), dbt[node] = static_cast<float>(cb);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
const char* const kSeWho = "spatial_encoder_3d";

// everything the entry points refuse about the sizes; fills the geometry
int check_se(int dtype, int64_t B, int64_t N, int64_t K, int64_t H, SeArgs* a) {
  if (check_float16(kSeWho, dtype, "the weights")) return -1;
  if (B < 0 || N < 0) return fail(kSeWho, "coord must be (B, N, 3) with B >= 0 and N >= 0");
  if (K < 1 || K > kSeMaxK)
    return fail(kSeWho, "num_kernels " + std::to_string(K) + ": the kernels take 1 to " + std::to_string(kSeMaxK));
  if (H < 1 || H > kSeMaxH)
    return fail(kSeWho, "num_heads " + std::to_string(H) + ": the kernels take 1 to " + std::to_string(kSeMaxH));
  if (N > INT32_MAX || (N > 0 && B > INT64_MAX / kSeMaxH / 8 / N / N) || B * N > INT32_MAX)
    return fail(kSeWho, "sizes overflow");
  a->N = N, a->pairs = B * N * N, a->tiles = (a->pairs + kSeTile - 1) / kSeTile;
  a->K = static_cast<int>(K), a->H = static_cast<int>(H);
  return 0;
}

// The eleven operands of forward and backward into `a`, after the one refusal of a null among them and `io`, the
// tensor the direction adds (`io_name`: out or dout).
int bind_se(SeArgs* a, const float* coord, const float* gamma_src, const float* gamma_tgt, const float* beta_src,
            const float* beta_tgt, const float* means, const float* stds, const void* w1, const void* b1, const void* w2,
            const void* b2, const void* io, const char* io_name) {
  if (!coord || !gamma_src || !gamma_tgt || !beta_src || !beta_tgt || !means || !stds || !w1 || !b1 || !w2 || !b2 || !io)
    return fail(kSeWho, std::string("an operand or ") + io_name + " is null");
  a->coord = coord, a->gs = gamma_src, a->gt = gamma_tgt, a->bs = beta_src, a->bt = beta_tgt, a->means = means, a->stds = stds;
  a->w1 = w1, a->b1 = b1, a->w2 = w2, a->b2 = b2;
  return 0;
}

struct SeWorkspace {
  size_t dx, part, bytes;
  int groups;
};
SeWorkspace se_workspace(int64_t pairs, int64_t K, int64_t H) {
  const int64_t tiles = (pairs + kSeTile - 1) / kSeTile;
  SeWorkspace w{};
  w.groups = static_cast<int>(tiles < kSeBwdGroups ? tiles : kSeBwdGroups);
  Carver c;
  w.dx = c.take(sizeof(float) * static_cast<size_t>(pairs));
  w.part = c.take(sizeof(float) * static_cast<size_t>(w.groups) * static_cast<size_t>(se_part_floats(K, H)));
  w.bytes = c.bytes();
  return w;
}

template <typename F>
int with_se_instance(int dtype, int64_t K, int64_t H, F&& f) {
  return with_float16(dtype, [&](auto ttag) -> int {
    auto with_h = [&](auto nbtag) -> int {
      if (H <= 32) return f(ttag, nbtag, std::integral_constant<int, 1>{});
      return f(ttag, nbtag, std::integral_constant<int, 2>{});
    };
    if (K <= 32) return with_h(std::integral_constant<int, 1>{});
    if (K <= 64) return with_h(std::integral_constant<int, 2>{});
    return with_h(std::integral_constant<int, 4>{});
  });
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_spatial_encoder3d_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t H) {
  SeArgs a{};
  if (check_se(kF32, B, N, K, H, &a) || a.pairs == 0) return 0;
  return se_workspace(a.pairs, K, H).bytes;
}

int dgla_spatial_encoder3d_forward(int dtype, const float* coord, const float* gamma_src, const float* gamma_tgt,
                                   const float* beta_src, const float* beta_tgt, const float* means, const float* stds,
                                   const void* w1, const void* b1, const void* w2, const void* b2, int64_t B, int64_t N, int64_t K,
                                   int64_t H, void* out, void* hip_stream) {
  SeArgs a{};
  if (check_se(dtype, B, N, K, H, &a)) return -1;
  if (a.pairs == 0) return 0;
  if (bind_se(&a, coord, gamma_src, gamma_tgt, beta_src, beta_tgt, means, stds, w1, b1, w2, b2, out, "out")) return -1;
  a.out = out, a.out_vec_ok = aligned_to(out, 16);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  return with_se_instance(dtype, K, H, [&](auto ttag, auto nbtag, auto hbtag) -> int {
    using T = decltype(ttag);
    constexpr int NB = decltype(nbtag)::value, HB = decltype(hbtag)::value;
    const unsigned grid = static_cast<unsigned>(a.tiles < kSeFwdGroups ? a.tiles : kSeFwdGroups);
    hipLaunchKernelGGL((se_forward_kernel<T, NB, HB>), dim3(grid), dim3(64 * NB), 0, s, a);
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

int dgla_spatial_encoder3d_backward(int dtype, const float* coord, const float* gamma_src, const float* gamma_tgt,
                                    const float* beta_src, const float* beta_tgt, const float* means, const float* stds,
                                    const void* w1, const void* b1, const void* w2, const void* b2, const void* dout, int64_t B,
                                    int64_t N, int64_t K, int64_t H, void* dw1, void* db1, void* dw2, void* db2, float* dmeans,
                                    float* dstds, float* dgamma_src, float* dgamma_tgt, float* dbeta_src, float* dbeta_tgt,
                                    void* workspace, size_t workspace_bytes, void* hip_stream) {
  SeArgs a{};
  if (check_se(dtype, B, N, K, H, &a)) return -1;
  if (a.pairs == 0) return 0;
  if (bind_se(&a, coord, gamma_src, gamma_tgt, beta_src, beta_tgt, means, stds, w1, b1, w2, b2, dout, "dout")) return -1;
  if (!dw1 || !db1 || !dw2 || !db2 || !dmeans || !dstds || !dgamma_src || !dgamma_tgt || !dbeta_src || !dbeta_tgt)
    return fail(kSeWho, "a gradient is null");
  const SeWorkspace w = se_workspace(a.pairs, K, H);
  if (optional_workspace(kSeWho, workspace, workspace_bytes, w.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, dw1);
  Scratch scratch(s);
  if (scratch.take(workspace, workspace_bytes, w.bytes)) return -1;
  a.dout = dout, a.dx = reinterpret_cast<float*>(scratch.p + w.dx), a.part = reinterpret_cast<float*>(scratch.p + w.part);
  return with_se_instance(dtype, K, H, [&](auto ttag, auto nbtag, auto hbtag) -> int {
    using T = decltype(ttag);
    constexpr int NB = decltype(nbtag)::value, HB = decltype(hbtag)::value;
    hipLaunchKernelGGL((se_backward_kernel<T, NB, HB>), dim3(static_cast<unsigned>(w.groups)), dim3(64 * NB), 0, s, a);
    hipLaunchKernelGGL(se_reduce_kernel<T>, dim3(grid1(se_part_floats(K, H), 256)), dim3(256), 0, s, a.part, w.groups, a.K, a.H, stds,
                       static_cast<T*>(dw1), static_cast<T*>(db1), static_cast<T*>(dw2), static_cast<T*>(db2), dmeans, dstds);
    hipLaunchKernelGGL(se_pair_kernel, dim3(static_cast<unsigned>(B * N)), dim3(64), 0, s, coord, a.dx, N, dgamma_src, dgamma_tgt,
                       dbeta_src, dbeta_tgt);
    DGLA_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

}  // extern "C"
