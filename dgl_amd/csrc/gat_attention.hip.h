// Shared pieces of the one-pass GAT attention kernels: the chunk table, the lane map, slab loads and stores, the
// partial-state merge, the fix-up kernels and the scratch layout.  Included by gat_attention.hip (inference form) and
// gat_attention_train.hip (attention dropout, attention-weight output); see gat_attention.hip for the scheme.
#pragma once
#include "../../include/dgl_amd.h"

#include "common.h"

namespace dgla {
namespace {

constexpr int kGatChunk = 512;  // edges per wavefront

// exp(x) for x <= 0 on v_exp_f32 with the product x * log2(e) carried as hi + lo (same routine as the fused edge
// softmax, csrc/edge_softmax.hip: |relative error| < 3e-7 over [-88, 0]; exp(-inf) = 0)
__device__ __forceinline__ float gat_exp(float x) {
  asm("v_max_f32 %0, %1, %2" : "=v"(x) : "v"(x), "v"(-200.f));
  const float hi = x * 1.44269504088896341f;
  const float lo = __builtin_fmaf(x, 1.44269504088896341f, -hi) + x * 1.92596299112661746e-8f;
  return __builtin_amdgcn_exp2f(hi) * __builtin_fmaf(lo, 0.693147180559945309f, 1.0f);
}

struct alignas(16) F4 {
  float x, y, z, w;
};

template <typename Idx>
__global__ __launch_bounds__(256) void gat_chunk_rows_kernel(const Idx* __restrict__ indptr, int64_t num_rows,
                                                            int64_t nchunks, int64_t* __restrict__ chunk_row,
                                                            int64_t* __restrict__ prow) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= nchunks) return;
  const int64_t p0 = c * kGatChunk;
  int64_t lo = 0, hi = num_rows + 1;  // first k with indptr[k] > p0 (exists: indptr[num_rows] = nnz > p0)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(indptr[mid]) > p0)
      hi = mid;
    else
      lo = mid + 1;
  }
  chunk_row[c] = lo - 1;
  prow[2 * c] = prow[2 * c + 1] = -1;
}

// rows without edges: zero their output rows (two outputs of widths wa / wb; either may be null)
template <typename Idx, typename TA, typename TB>
__global__ __launch_bounds__(256) void gat_zero_rows_kernel(const Idx* __restrict__ indptr, int64_t num_rows,
                                                           TA* __restrict__ a, int wa, TB* __restrict__ b, int wb,
                                                           float fill_b0, float fill_b1) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= num_rows || indptr[r] != indptr[r + 1]) return;
  if (a)
    for (int i = 0; i < wa; ++i) a[r * wa + i] = from_acc<TA>(0.f);
  if (b)
    for (int i = 0; i < wb; ++i) b[r * wb + i] = from_acc<TB>((i & 1) ? fill_b1 : fill_b0);
}

// (an empty side launches nothing: a grid of 0 blocks is an error)
template <typename Idx, typename TA, typename TB>
void zero_rows(hipStream_t s, const Idx* indptr, int64_t n, TA* a, int wa, TB* b, int wb, float fill_b0, float fill_b1) {
  if (n <= 0) return;
  hipLaunchKernelGGL((gat_zero_rows_kernel<Idx, TA, TB>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s,
                     indptr, n, a, wa, b, wb, fill_b0, fill_b1);
}

template <int LOG2_LPR>
struct Geo {
  static constexpr int LPR = 1 << LOG2_LPR;
  static constexpr int G = 64 / LPR;
  static constexpr int U = LOG2_LPR >= 4 ? 4 : (LOG2_LPR == 3 ? 2 : 1);
};

__device__ __forceinline__ float head_sum(float v, int lph_log2) {
  for (int m = 1; m < (1 << lph_log2); m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// A lane owns V consecutive elements of one head (one naturally aligned load of V * sizeof(T) bytes), a head is
// LPH = 1 << lph_log2 lanes of which ceil(D / V) are active, a row LPR = next_pow2(H * LPH) lanes:
//     h = l >> lph_log2,  j = l & (LPH - 1),  col = h * D + j * V,  active = h < H && j * V < D.
// Idle lanes hold zeros, so the xor butterfly over the LPH lanes of a head (head_sum) is the one of the fp32
// power-of-two kernels of gat_attention.hip.  16-bit values are widened on load; m, z, the accumulators, every partial state, mz and aux are fp32, and the
// only roundings to 16 bits are the stores of out, d_ft, d_el and d_er.
template <typename T, typename Idx>
struct WideArgs {
  const Idx* indptr;
  const Idx* indices;
  int64_t num_rows, nnz, nchunks;
  const int64_t* chunk_row;
  int64_t* prow;
  float* pval;
  int ns;                      // floats per partial state
  int H, D, HD, HDp, lph_log2;  // heads, width, H * D, H * D padded to 4, log2(LPH)
  float slope;
  const T* ft;
  const T* el;
  const T* er;
  const T* dout;
  T* out;
  float* mz;
  float* aux;
  T* d_ft;
  T* d_el;
  T* d_er;
};

template <typename T, int V>
__device__ __forceinline__ void load_slab(const T* __restrict__ src, float (&f)[V]) {
  const VecT<T, V> v = *reinterpret_cast<const VecT<T, V>*>(src);
#pragma unroll
  for (int i = 0; i < V; ++i) f[i] = to_acc<T>(v.v[i]);
}

template <typename T, int V>
__device__ __forceinline__ void store_slab(T* __restrict__ dst, const float (&f)[V], float scale) {
  VecT<T, V> v;
#pragma unroll
  for (int i = 0; i < V; ++i) v.v[i] = from_acc<T>(f[i] * scale);
  *reinterpret_cast<VecT<T, V>*>(dst) = v;
}

// V floats of a partial state (16-byte pieces: states start on 16-byte boundaries and col is a multiple of V)
template <int V>
__device__ __forceinline__ void load_part(const float* __restrict__ src, float (&f)[V]) {
  constexpr int W = V < 4 ? V : 4;
#pragma unroll
  for (int c = 0; c < V / W; ++c) {
    const VecT<float, W> v = *reinterpret_cast<const VecT<float, W>*>(src + c * W);
#pragma unroll
    for (int i = 0; i < W; ++i) f[c * W + i] = v.v[i];
  }
}

template <int V>
__device__ __forceinline__ void store_part(float* __restrict__ dst, const float (&f)[V]) {
  constexpr int W = V < 4 ? V : 4;
#pragma unroll
  for (int c = 0; c < V / W; ++c) {
    VecT<float, W> v;
#pragma unroll
    for (int i = 0; i < W; ++i) v.v[i] = f[c * W + i];
    *reinterpret_cast<VecT<float, W>*>(dst + c * W) = v;
  }
}

template <int V>
__device__ __forceinline__ float dotv(const float (&a)[V], const float (&b)[V]) {
  float r = a[0] * b[0];
#pragma unroll
  for (int i = 1; i < V; ++i) r = __builtin_fmaf(a[i], b[i], r);
  return r;
}

template <int V>
__device__ __forceinline__ void wide_merge(float& m, float& z, float (&acc)[V], float m_o, float z_o, const float (&a_o)[V]) {
  const float mn = m > m_o ? m : m_o;
  const float a = m == mn ? 1.f : gat_exp(m - mn);
  const float b = m_o == mn ? 1.f : gat_exp(m_o - mn);
  z = z * a + z_o * b;
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = acc[i] * a + a_o[i] * b;
  m = mn;
}

// the lane map of one row group (see the comment on WideArgs)
struct WideLane {
  int h, col;
  bool active, head_lane;
};

template <typename A>
__device__ __forceinline__ WideLane wide_lane(const A& p, int l, int V) {
  WideLane w;
  const int h = l >> p.lph_log2, j = l & ((1 << p.lph_log2) - 1);
  w.active = h < p.H && j * V < p.D;
  w.h = w.active ? h : 0;
  w.col = w.active ? h * p.D + j * V : 0;
  w.head_lane = j == 0;
  return w;
}

template <typename T, int V, typename Idx>
__global__ __launch_bounds__(64) void gat_fwd_wide_fixup_kernel(const WideArgs<T, Idx> p) {
  const int64_t c = blockIdx.x;
  const int64_t r = p.prow[2 * c + 1];
  if (r < 0) return;
  const WideLane w = wide_lane(p, static_cast<int>(threadIdx.x), V);
  if (!w.active) return;  // no cross-lane operation below
  const int h = w.h, col = w.col;
  const float* pv = p.pval + (2 * c + 1) * p.ns;
  float acc[V];
  load_part<V>(pv + col, acc);
  float m = pv[p.HDp + 2 * h], z = pv[p.HDp + 2 * h + 1];
  for (int64_t cc = c + 1; cc < p.nchunks && p.prow[2 * cc] == r; ++cc) {
    const float* qv = p.pval + (2 * cc) * p.ns;
    float a_o[V];
    load_part<V>(qv + col, a_o);
    wide_merge<V>(m, z, acc, qv[p.HDp + 2 * h], qv[p.HDp + 2 * h + 1], a_o);
  }
  store_slab<T, V>(p.out + r * p.HD + col, acc, 1.f / z);
  if (w.head_lane) {
    p.mz[(r * p.H + h) * 2] = m;
    p.mz[(r * p.H + h) * 2 + 1] = z;
  }
}

template <typename T, typename Idx>
__global__ __launch_bounds__(64) void gat_bwd_dst_wide_fixup_kernel(const WideArgs<T, Idx> p) {
  const int64_t c = blockIdx.x;
  const int64_t r = p.prow[2 * c + 1];
  if (r < 0) return;
  const int H = p.H;
  for (int h = threadIdx.x; h < H; h += 64) {
    const float* pv = p.pval + (2 * c + 1) * static_cast<int64_t>(p.ns);
    float s1 = pv[h], s2 = pv[H + h], s3 = pv[2 * H + h];
    for (int64_t cc = c + 1; cc < p.nchunks && p.prow[2 * cc] == r; ++cc) {
      const float* qv = p.pval + (2 * cc) * static_cast<int64_t>(p.ns);
      s1 += qv[h];
      s2 += qv[H + h];
      s3 += qv[2 * H + h];
    }
    p.d_er[r * H + h] = from_acc<T>(s2 - s1 * s3);
    *reinterpret_cast<F4*>(p.aux + (r * H + h) * 4) =
        F4{to_acc<T>(p.er[r * H + h]), p.mz[(r * H + h) * 2], 1.f / p.mz[(r * H + h) * 2 + 1], s1};
  }
}

// fix-up of pass 2, wide: elements [0, wa) of a state go to a[row, :], elements [off_b, off_b + wb) to b[row, :]
template <typename T>
__global__ __launch_bounds__(64) void gat_sum_wide_fixup_kernel(const int64_t* __restrict__ prow, const float* __restrict__ pval,
                                                               int ns, int64_t nchunks, T* __restrict__ a, int wa, int off_b,
                                                               T* __restrict__ b, int wb) {
  const int64_t c = blockIdx.x;
  const int64_t r = prow[2 * c + 1];
  if (r < 0) return;
  for (int i = threadIdx.x; i < wa + wb; i += 64) {
    const int e = i < wa ? i : off_b + (i - wa);
    float v = pval[(2 * c + 1) * static_cast<int64_t>(ns) + e];
    for (int64_t cc = c + 1; cc < nchunks && prow[2 * cc] == r; ++cc) v += pval[(2 * cc) * static_cast<int64_t>(ns) + e];
    if (i < wa)
      a[r * wa + i] = from_acc<T>(v);
    else
      b[r * wb + (i - wa)] = from_acc<T>(v);
  }
}

int pad4(int x) { return (x + 3) & ~3; }  // partial states start on 16-byte boundaries

int64_t num_chunks(int64_t nnz) { return (nnz + kGatChunk - 1) / kGatChunk; }

struct Shape {
  int H, D, HD, lph_log2, log2_lpr;
  int V;        // elements per lane
  bool legacy;  // fp32 with D a power of two >= 4: the 16-byte-slab kernels of gat_attention.hip
};

int next_pow2_log2(int64_t x) {
  int lg = 0;
  while ((int64_t{1} << lg) < x) ++lg;
  return lg;
}

// The accepted set, stated once (include/dgl_amd.h): V = min(16 / s, largest power of two dividing D) elements per lane,
// LPH = next_pow2(ceil(D / V)) lanes per head, and a row must fit one wavefront: H * LPH <= 64.
bool accepted(dgla_dtype dtype, int64_t H, int64_t D, int* v_out, int* lph_log2_out) {
  const int s = dtype == DGLA_F32 ? 4 : (dtype == DGLA_F16 || dtype == DGLA_BF16) ? 2 : 0;
  if (s == 0 || H < 1 || D < 1 || H > 64 || D > 64 * 8) return false;
  int V = 16 / s;
  while (D % V) V >>= 1;
  const int lg = next_pow2_log2((D + V - 1) / V);
  if ((H << lg) > 64) return false;
  if (v_out) *v_out = V;
  if (lph_log2_out) *lph_log2_out = lg;
  return true;
}

// a tensor argument that was given: empty tensors (a side without nodes) carry no data pointer
bool present(const dgla_tensor* t) {
  if (!t || t->ndim <= 0) return false;
  if (t->data) return true;
  for (int i = 0; i < t->ndim; ++i)
    if (t->shape[i] == 0) return true;
  return false;
}

int shape_of(dgla_dtype dtype, const dgla_tensor* ft, const dgla_tensor* el, const dgla_tensor* er, Shape* s) {
  if (!present(ft) || !present(el) || !present(er)) return fail("gat_attention: ft / el / er are required");
  if (ft->ndim != 3 || el->ndim != 3 || er->ndim != 3 || el->shape[2] != 1 || er->shape[2] != 1)
    return fail("gat_attention: ft must be (N_src, H, D), el (N_src, H, 1), er (N_dst, H, 1)");
  const int64_t H = ft->shape[1], D = ft->shape[2];
  if (el->shape[1] != H || er->shape[1] != H || el->shape[0] != ft->shape[0])
    return fail("gat_attention: head counts / node counts of ft, el, er differ");
  if (!accepted(dtype, H, D, &s->V, &s->lph_log2))
    return fail("gat_attention: needs fp32 / fp16 / bf16 operands with H * next_pow2(ceil(D / V)) <= 64, V = min(16 / "
                 "sizeof(element), largest power of two dividing D) (dgla_gat_attention_supported; use the composed "
                 "operators otherwise)");
  s->H = static_cast<int>(H);
  s->D = static_cast<int>(D);
  s->HD = static_cast<int>(H * D);
  s->log2_lpr = next_pow2_log2(H << s->lph_log2);
  if (s->log2_lpr < 2) s->log2_lpr = 2;  // narrowest instantiation: 4 lanes per row (lanes past the last head idle)
  s->legacy = dtype == DGLA_F32 && D >= 4 && (D & (D - 1)) == 0;
  return 0;
}

template <typename Idx>
struct Scratch {
  int64_t* chunk_row;
  int64_t* prow;
  float* pval;
  float* aux;
};

size_t scratch_bytes(int64_t nnz, int64_t num_dst, int H, int HD) {
  const int64_t nc = num_chunks(nnz);
  return align256(8 * nc) + align256(16 * nc) + align256(sizeof(float) * 2 * nc * (pad4(HD) + pad4(2 * H))) +
         align256(sizeof(float) * 4 * num_dst * H);
}

template <typename Idx>
Scratch<Idx> carve(char* ws, int64_t nnz, int H, int HD) {
  const int64_t nc = num_chunks(nnz);
  Scratch<Idx> s;
  s.chunk_row = reinterpret_cast<int64_t*>(ws);
  ws += align256(8 * nc);
  s.prow = reinterpret_cast<int64_t*>(ws);
  ws += align256(16 * nc);
  s.pval = reinterpret_cast<float*>(ws);
  ws += align256(sizeof(float) * 2 * nc * (pad4(HD) + pad4(2 * H)));
  s.aux = reinterpret_cast<float*>(ws);
  return s;
}

unsigned grid1(int64_t n, int per = 256) { return static_cast<unsigned>((n + per - 1) / per); }

struct WidePtrs {
  const void *ft, *el, *er, *dout;
  void *out, *d_ft, *d_el, *d_er;
  float* mz;
};

template <typename T, typename Idx>
WideArgs<T, Idx> wide_args(const Shape& sh, const WidePtrs& q, int64_t nnz, const Scratch<Idx>& sc, float slope) {
  WideArgs<T, Idx> a{};
  a.nnz = nnz;
  a.nchunks = num_chunks(nnz);
  a.chunk_row = sc.chunk_row;
  a.prow = sc.prow;
  a.pval = sc.pval;
  a.H = sh.H;
  a.D = sh.D;
  a.HD = sh.HD;
  a.HDp = pad4(sh.HD);
  a.lph_log2 = sh.lph_log2;
  a.slope = slope;
  a.ft = static_cast<const T*>(q.ft);
  a.el = static_cast<const T*>(q.el);
  a.er = static_cast<const T*>(q.er);
  a.dout = static_cast<const T*>(q.dout);
  a.out = static_cast<T*>(q.out);
  a.mz = q.mz;
  a.aux = sc.aux;
  a.d_ft = static_cast<T*>(q.d_ft);
  a.d_el = static_cast<T*>(q.d_el);
  a.d_er = static_cast<T*>(q.d_er);
  return a;
}

}  // namespace
}  // namespace dgla
