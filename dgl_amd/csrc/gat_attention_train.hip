// Training form of the one-pass GAT attention block for gfx950 (MI355X): dropout on the attention weights and the
// attention weights as an output (include/dgl_amd.h, "Training form"; the reference line is
// graph.edata["a"] = self.attn_drop(edge_softmax(graph, e)), python/dgl/nn/pytorch/conv/gatconv.py:337-347).
//
//   out[v, h, :] = sum_{u -> v} a_e,h c_e,h ft[u, h, :],   a = softmax_v(leaky_relu(el[u, h] + er[v, h])),
//   c_e,h = gat_keep(seed, eid, h) / (1 - p)                                                    (csrc/gat_dropout.h)
//
// No mask is stored.  The keep bit is a pure function of (seed, edge id, head): the forward evaluates it in registers
// and the two backward passes evaluate it again, each from the edge-id map of the CSR it walks (data ? data[pos] : pos),
// so the only extra traffic is the streamed read of that map, E * i bytes per pass.  The softmax state (m, z) is the one
// WITHOUT dropout — mz means what it means in gat_attention.hip — and the weights kernel recomputes a c from it on
// request, in edge-id order.
//
// Same decomposition as the wide kernels of gat_attention.hip (one wavefront per chunk of kGatChunk edges, a lane owns V
// elements of one head, fp32 state, one rounding at the final store, partial rows merged by the same fix-up kernels in
// chunk order; no atomics), for EVERY accepted shape: fp32 with D a power of two runs here too, with V = 4.  With
// x_e = <dout_v, ft_u>_h and l'_e = leaky_relu'(el_u + er_v):
//   forward   z += pk;  acc += (pk c) f
//   B1        S1 = sum a c x (= t),  S2 = sum l' a c x,  S3 = sum l' a;   d_er = S2 - S1 S3;  aux = (er, m, 1/z, t)
//   B2        d_ft[u] = sum a c dout_v;   d_el[u] = sum l' a (c x - t_v)
// p = 0 (threshold 0) evaluates no Philox round, and a multiplication by c = 1 is exact: the results are those of the
// wide kernels, bit for bit.
#include "../../include/dgl_amd.h"

#include "common.h"
#include "gat_attention.hip.h"
#include "gat_dropout.h"

namespace dgla {
namespace {

template <typename T, typename Idx>
struct TrainArgs : WideArgs<T, Idx> {
  const Idx* data;  // edge-id map of the CSR this pass walks, null: edge id == position
  uint64_t seed;
  uint32_t threshold;  // keep iff (word >> 8) >= threshold; 0: nothing is dropped
  float scale;         // 1 / (1 - p)
};

// c_e,h of the edge at position `pos` (read only where `ok`: positions past the row's end may lie past the array)
template <typename A>
__device__ __forceinline__ float drop_factor(const A& p, int64_t pos, bool ok, int h) {
  if (!ok) return 0.f;
  const uint64_t eid = p.data ? static_cast<uint64_t>(p.data[pos]) : static_cast<uint64_t>(pos);
  return gat_keep(p.seed, eid, h, p.threshold) ? p.scale : 0.f;
}

template <typename T, int V, typename Idx, int LOG2_LPR>
__global__ __launch_bounds__(256) void gat_fwd_train_kernel(const TrainArgs<T, Idx> p) {
  using GE = Geo<LOG2_LPR>;
  constexpr int LPR = GE::LPR, G = GE::G, U = GE::U;
  const int lane = threadIdx.x & 63;
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (c >= p.nchunks) return;
  const int l = lane & (LPR - 1), g = lane >> LOG2_LPR;
  const WideLane w = wide_lane(p, l, V);
  const bool active = w.active;
  const int h = w.h, col = w.col;
  const int H = p.H, HD = p.HD;
  const bool drop = p.threshold != 0;  // wave-uniform
  const float ninf = -__builtin_huge_valf();
  const int64_t p0 = c * kGatChunk;
  const int64_t p1 = p0 + kGatChunk < p.nnz ? p0 + kGatChunk : p.nnz;
  int64_t row = p.chunk_row[c];
  int64_t rs = static_cast<int64_t>(p.indptr[row]), re = static_cast<int64_t>(p.indptr[row + 1]);
  int64_t pos = p0;
  while (pos < p1) {
    while (re <= pos) {
      ++row;
      rs = re;
      re = static_cast<int64_t>(p.indptr[row + 1]);
    }
    const int64_t b = re < p1 ? re : p1;
    const float er_h = active ? to_acc<T>(p.er[row * H + h]) : 0.f;
    float m = ninf, z = 0.f, acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int64_t base = pos; base < b; base += G * U) {
      int64_t src[U];
      bool ok[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t j = base + k * G + g;
        ok[k] = j < b && active;
        src[k] = ok[k] ? static_cast<int64_t>(p.indices[j]) : 0;
      }
      float sv[U], f[U][V], cf[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        sv[k] = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) f[k][i] = 0.f;
        if (ok[k]) {
          sv[k] = to_acc<T>(p.el[src[k] * H + h]);
          load_slab<T, V>(p.ft + src[k] * HD + col, f[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) cf[k] = drop ? drop_factor(p, base + k * G + g, ok[k], h) : 1.f;
      float bm = ninf;
#pragma unroll
      for (int k = 0; k < U; ++k) {
        float s = sv[k] + er_h;
        s = s > 0.f ? s : s * p.slope;
        sv[k] = ok[k] ? s : ninf;
        bm = bm > sv[k] ? bm : sv[k];
      }
      const float mn = m > bm ? m : bm;
      const float sc = m == mn ? 1.f : gat_exp(m - mn);
      z *= sc;
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] *= sc;
      m = mn;
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const float pk = ok[k] ? gat_exp(sv[k] - mn) : 0.f;
        const float pc = pk * cf[k];
        z += pk;
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = __builtin_fmaf(pc, f[k][i], acc[i]);
      }
    }
#pragma unroll
    for (int mk = LPR; mk < 64; mk <<= 1) {
      const float m_o = __shfl_xor(m, mk, 64), z_o = __shfl_xor(z, mk, 64);
      float a_o[V];
#pragma unroll
      for (int i = 0; i < V; ++i) a_o[i] = __shfl_xor(acc[i], mk, 64);
      wide_merge<V>(m, z, acc, m_o, z_o, a_o);
    }
    const bool head_partial = pos > rs, tail_partial = re > p1;
    if (head_partial || tail_partial) {
      const int64_t slot = 2 * c + (head_partial ? 0 : 1);
      float* pv = p.pval + slot * p.ns;
      if (g == 0 && active) {
        store_part<V>(pv + col, acc);
        if (w.head_lane) {
          pv[p.HDp + 2 * h] = m;
          pv[p.HDp + 2 * h + 1] = z;
        }
      }
      if (lane == 0) p.prow[slot] = row;
    } else if (g == 0 && active) {
      store_slab<T, V>(p.out + row * HD + col, acc, 1.f / z);
      if (w.head_lane) {
        p.mz[(row * H + h) * 2] = m;
        p.mz[(row * H + h) * 2 + 1] = z;
      }
    }
    pos = b;
  }
}

// backward pass 1 (rows = destination nodes): the three sums of gat_bwd_dst_wide_kernel with the dropout factor on the
// terms that carry x; S3 — the derivative of the normaliser — sees every edge
template <typename T, int V, typename Idx, int LOG2_LPR>
__global__ __launch_bounds__(256) void gat_bwd_dst_train_kernel(const TrainArgs<T, Idx> p) {
  using GE = Geo<LOG2_LPR>;
  constexpr int LPR = GE::LPR, G = GE::G, U = GE::U;
  const int lane = threadIdx.x & 63;
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (c >= p.nchunks) return;
  const int l = lane & (LPR - 1), g = lane >> LOG2_LPR;
  const WideLane w = wide_lane(p, l, V);
  const bool active = w.active;
  const int h = w.h, col = w.col;
  const int H = p.H, HD = p.HD;
  const bool drop = p.threshold != 0;
  const int64_t p0 = c * kGatChunk;
  const int64_t p1 = p0 + kGatChunk < p.nnz ? p0 + kGatChunk : p.nnz;
  int64_t row = p.chunk_row[c];
  int64_t rs = static_cast<int64_t>(p.indptr[row]), re = static_cast<int64_t>(p.indptr[row + 1]);
  int64_t pos = p0;
  while (pos < p1) {
    while (re <= pos) {
      ++row;
      rs = re;
      re = static_cast<int64_t>(p.indptr[row + 1]);
    }
    const int64_t b = re < p1 ? re : p1;
    float er_h = 0.f, m_h = 0.f, rz = 0.f, dO[V];
#pragma unroll
    for (int i = 0; i < V; ++i) dO[i] = 0.f;
    if (active) {
      er_h = to_acc<T>(p.er[row * H + h]);
      m_h = p.mz[(row * H + h) * 2];
      rz = 1.f / p.mz[(row * H + h) * 2 + 1];
      load_slab<T, V>(p.dout + row * HD + col, dO);
    }
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int64_t base = pos; base < b; base += G * U) {
      int64_t src[U];
      bool ok[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t j = base + k * G + g;
        ok[k] = j < b && active;
        src[k] = ok[k] ? static_cast<int64_t>(p.indices[j]) : 0;
      }
      float sv[U], f[U][V], cf[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        sv[k] = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) f[k][i] = 0.f;
        if (ok[k]) {
          sv[k] = to_acc<T>(p.el[src[k] * H + h]);
          load_slab<T, V>(p.ft + src[k] * HD + col, f[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) cf[k] = drop ? drop_factor(p, base + k * G + g, ok[k], h) : 1.f;
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const float x = head_sum(dotv<V>(dO, f[k]), p.lph_log2);
        const float pre = sv[k] + er_h;
        const float s = pre > 0.f ? pre : pre * p.slope;
        const float a = ok[k] ? gat_exp(s - m_h) * rz : 0.f;
        const float la = a * (pre > 0.f ? 1.f : p.slope);
        const float ac = a * cf[k], lac = la * cf[k];
        s1 = __builtin_fmaf(ac, x, s1);
        s2 = __builtin_fmaf(lac, x, s2);
        s3 += la;
      }
    }
#pragma unroll
    for (int mk = LPR; mk < 64; mk <<= 1) {
      s1 += __shfl_xor(s1, mk, 64);
      s2 += __shfl_xor(s2, mk, 64);
      s3 += __shfl_xor(s3, mk, 64);
    }
    const bool head_partial = pos > rs, tail_partial = re > p1;
    if (head_partial || tail_partial) {
      const int64_t slot = 2 * c + (head_partial ? 0 : 1);
      if (g == 0 && active && w.head_lane) {
        float* pv = p.pval + slot * p.ns;
        pv[h] = s1;
        pv[H + h] = s2;
        pv[2 * H + h] = s3;
      }
      if (lane == 0) p.prow[slot] = row;
    } else if (g == 0 && active && w.head_lane) {
      p.d_er[row * H + h] = from_acc<T>(s2 - s1 * s3);
      *reinterpret_cast<F4*>(p.aux + (row * H + h) * 4) = F4{er_h, m_h, rz, s1};
    }
    pos = b;
  }
}

// backward pass 2 (rows = source nodes, out-edge CSR; p.data is THAT CSR's edge-id map)
template <typename T, int V, typename Idx, int LOG2_LPR>
__global__ __launch_bounds__(256) void gat_bwd_src_train_kernel(const TrainArgs<T, Idx> p) {
  using GE = Geo<LOG2_LPR>;
  constexpr int LPR = GE::LPR, G = GE::G, U = GE::U;
  const int lane = threadIdx.x & 63;
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (c >= p.nchunks) return;
  const int l = lane & (LPR - 1), g = lane >> LOG2_LPR;
  const WideLane w = wide_lane(p, l, V);
  const bool active = w.active;
  const int h = w.h, col = w.col;
  const int H = p.H, HD = p.HD;
  const bool drop = p.threshold != 0;
  const int64_t p0 = c * kGatChunk;
  const int64_t p1 = p0 + kGatChunk < p.nnz ? p0 + kGatChunk : p.nnz;
  int64_t row = p.chunk_row[c];
  int64_t rs = static_cast<int64_t>(p.indptr[row]), re = static_cast<int64_t>(p.indptr[row + 1]);
  int64_t pos = p0;
  while (pos < p1) {
    while (re <= pos) {
      ++row;
      rs = re;
      re = static_cast<int64_t>(p.indptr[row + 1]);
    }
    const int64_t b = re < p1 ? re : p1;
    float el_h = 0.f, f[V];
#pragma unroll
    for (int i = 0; i < V; ++i) f[i] = 0.f;
    if (active) {
      el_h = to_acc<T>(p.el[row * H + h]);
      load_slab<T, V>(p.ft + row * HD + col, f);
    }
    float acc_el = 0.f, acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int64_t base = pos; base < b; base += G * U) {
      int64_t dst[U];
      bool ok[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t j = base + k * G + g;
        ok[k] = j < b && active;
        dst[k] = ok[k] ? static_cast<int64_t>(p.indices[j]) : 0;
      }
      F4 ax[U];
      float dO[U][V], cf[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        ax[k] = F4{0.f, 0.f, 1.f, 0.f};
#pragma unroll
        for (int i = 0; i < V; ++i) dO[k][i] = 0.f;
        if (ok[k]) {
          ax[k] = *reinterpret_cast<const F4*>(p.aux + (dst[k] * H + h) * 4);
          load_slab<T, V>(p.dout + dst[k] * HD + col, dO[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) cf[k] = drop ? drop_factor(p, base + k * G + g, ok[k], h) : 1.f;
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const float dA = head_sum(dotv<V>(dO[k], f), p.lph_log2);
        const float pre = el_h + ax[k].x;
        const float s = pre > 0.f ? pre : pre * p.slope;
        const float a = ok[k] ? gat_exp(s - ax[k].y) * ax[k].z : 0.f;
        const float cx = cf[k] * dA, ac = a * cf[k];
        acc_el += a * (cx - ax[k].w) * (pre > 0.f ? 1.f : p.slope);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = __builtin_fmaf(ac, dO[k][i], acc[i]);
      }
    }
#pragma unroll
    for (int mk = LPR; mk < 64; mk <<= 1) {
      acc_el += __shfl_xor(acc_el, mk, 64);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] += __shfl_xor(acc[i], mk, 64);
    }
    const bool head_partial = pos > rs, tail_partial = re > p1;
    if (head_partial || tail_partial) {
      const int64_t slot = 2 * c + (head_partial ? 0 : 1);
      float* pv = p.pval + slot * p.ns;
      if (g == 0 && active) {
        store_part<V>(pv + col, acc);
        if (w.head_lane) pv[p.HDp + h] = acc_el;
      }
      if (lane == 0) p.prow[slot] = row;
    } else if (g == 0 && active) {
      store_slab<T, V>(p.d_ft + row * HD + col, acc, 1.f);
      if (w.head_lane) p.d_el[row * H + h] = from_acc<T>(acc_el);
    }
    pos = b;
  }
}

// attn[eid, h] = a c for every edge, one thread per in-edge CSR position: the thread finds its row by bisection of
// indptr (no workspace: the kernel runs on request, next to a forward that saved mz), walks the heads, evaluates one
// Philox block per four heads and writes the H weights of its edge to row `eid` of attn.
template <typename T, typename Idx>
__global__ __launch_bounds__(256) void gat_weights_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                         const Idx* __restrict__ data, int64_t num_rows, int64_t nnz, int H,
                                                         float slope, uint64_t seed, uint32_t threshold, float scale,
                                                         const T* __restrict__ el, const T* __restrict__ er,
                                                         const float* __restrict__ mz, T* __restrict__ attn) {
  const int64_t pos = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (pos >= nnz) return;
  int64_t lo = 0, hi = num_rows + 1;  // first k with indptr[k] > pos (exists: indptr[num_rows] = nnz > pos)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(indptr[mid]) > pos)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int64_t v = lo - 1, u = static_cast<int64_t>(indices[pos]);
  const int64_t eid = data ? static_cast<int64_t>(data[pos]) : pos;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int h0 = 0; h0 < H; h0 += 4) {
    if (threshold != 0) gat_philox4(seed, static_cast<uint64_t>(eid), static_cast<uint32_t>(h0) >> 2, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int h = h0 + i;
      if (h < H) {
        const float pre = to_acc<T>(el[u * H + h]) + to_acc<T>(er[v * H + h]);
        const float s = pre > 0.f ? pre : pre * slope;
        const float a = gat_exp(s - mz[(v * H + h) * 2]) * (1.f / mz[(v * H + h) * 2 + 1]);
        const float cf = threshold == 0 ? 1.f : (gat_keep_word(w[i], threshold) ? scale : 0.f);
        attn[eid * H + h] = from_acc<T>(a * cf);
      }
    }
  }
}

#define DGLA_GATT_DISPATCH(KERNEL, LG, ...)                                              \
  switch (LG) {                                                                          \
    case 2: hipLaunchKernelGGL((KERNEL<T, V, Idx, 2>), __VA_ARGS__); break;               \
    case 3: hipLaunchKernelGGL((KERNEL<T, V, Idx, 3>), __VA_ARGS__); break;               \
    case 4: hipLaunchKernelGGL((KERNEL<T, V, Idx, 4>), __VA_ARGS__); break;               \
    case 5: hipLaunchKernelGGL((KERNEL<T, V, Idx, 5>), __VA_ARGS__); break;               \
    default: hipLaunchKernelGGL((KERNEL<T, V, Idx, 6>), __VA_ARGS__); break;              \
  }

struct Drop {
  uint64_t seed;
  uint32_t threshold;
  float scale;
};

template <typename T, typename Idx>
TrainArgs<T, Idx> train_args(const Shape& sh, const WidePtrs& q, int64_t nnz, const Scratch<Idx>& sc, float slope,
                             const Drop& dr) {
  TrainArgs<T, Idx> a{};
  static_cast<WideArgs<T, Idx>&>(a) = wide_args<T, Idx>(sh, q, nnz, sc, slope);
  a.seed = dr.seed;
  a.threshold = dr.threshold;
  a.scale = dr.scale;
  return a;
}

template <typename T, int V, typename Idx>
int forward_train_v(const dgla_csr* csc, const Shape& sh, const WidePtrs& q, float slope, const Drop& dr, char* ws,
                    hipStream_t s) {
  const int64_t nnz = csc->nnz, n = csc->num_rows;
  const Idx* indptr = static_cast<const Idx*>(csc->indptr);
  zero_rows(s, indptr, n, static_cast<T*>(q.out), sh.HD, q.mz, 2 * sh.H, 0.f, 1.f);
  if (nnz > 0) {
    const Scratch<Idx> sc = carve<Idx>(ws, nnz, sh.H, sh.HD);
    TrainArgs<T, Idx> a = train_args<T, Idx>(sh, q, nnz, sc, slope, dr);
    a.indptr = indptr;
    a.indices = static_cast<const Idx*>(csc->indices);
    a.data = static_cast<const Idx*>(csc->data);
    a.num_rows = n;
    a.ns = a.HDp + pad4(2 * sh.H);
    hipLaunchKernelGGL(gat_chunk_rows_kernel<Idx>, dim3(grid1(a.nchunks)), dim3(256), 0, s, indptr, n, a.nchunks,
                       sc.chunk_row, sc.prow);
    DGLA_GATT_DISPATCH(gat_fwd_train_kernel, sh.log2_lpr, dim3(grid1(a.nchunks, 4)), dim3(256), 0, s, a);
    const WideArgs<T, Idx>& base = a;
    hipLaunchKernelGGL((gat_fwd_wide_fixup_kernel<T, V, Idx>), dim3(static_cast<unsigned>(a.nchunks)), dim3(64), 0, s, base);
  }
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T, int V, typename Idx>
int backward_train_v(const dgla_csr* csc, const dgla_csr* csr, const Shape& sh, const WidePtrs& q, float slope,
                     const Drop& dr, char* ws, hipStream_t s) {
  const int64_t nnz = csc->nnz, n_dst = csc->num_rows, n_src = csr->num_rows;
  const Idx* ip_in = static_cast<const Idx*>(csc->indptr);
  const Idx* ip_out = static_cast<const Idx*>(csr->indptr);
  zero_rows(s, ip_in, n_dst, static_cast<T*>(q.d_er), sh.H, static_cast<T*>(nullptr), 0, 0.f, 0.f);
  zero_rows(s, ip_out, n_src, static_cast<T*>(q.d_ft), sh.HD, static_cast<T*>(q.d_el), sh.H, 0.f, 0.f);
  if (nnz > 0) {
    const Scratch<Idx> sc = carve<Idx>(ws, nnz, sh.H, sh.HD);
    TrainArgs<T, Idx> a = train_args<T, Idx>(sh, q, nnz, sc, slope, dr);
    const WideArgs<T, Idx>& base = a;
    // pass 1: rows = destination nodes; three sums per (row, head)
    a.indptr = ip_in;
    a.indices = static_cast<const Idx*>(csc->indices);
    a.data = static_cast<const Idx*>(csc->data);
    a.num_rows = n_dst;
    a.ns = pad4(3 * sh.H);
    hipLaunchKernelGGL(gat_chunk_rows_kernel<Idx>, dim3(grid1(a.nchunks)), dim3(256), 0, s, ip_in, n_dst, a.nchunks,
                       sc.chunk_row, sc.prow);
    DGLA_GATT_DISPATCH(gat_bwd_dst_train_kernel, sh.log2_lpr, dim3(grid1(a.nchunks, 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL((gat_bwd_dst_wide_fixup_kernel<T, Idx>), dim3(static_cast<unsigned>(a.nchunks)), dim3(64), 0, s, base);
    // pass 2: rows = source nodes
    a.indptr = ip_out;
    a.indices = static_cast<const Idx*>(csr->indices);
    a.data = static_cast<const Idx*>(csr->data);
    a.num_rows = n_src;
    a.ns = a.HDp + pad4(sh.H);
    hipLaunchKernelGGL(gat_chunk_rows_kernel<Idx>, dim3(grid1(a.nchunks)), dim3(256), 0, s, ip_out, n_src, a.nchunks,
                       sc.chunk_row, sc.prow);
    DGLA_GATT_DISPATCH(gat_bwd_src_train_kernel, sh.log2_lpr, dim3(grid1(a.nchunks, 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(gat_sum_wide_fixup_kernel<T>, dim3(static_cast<unsigned>(a.nchunks)), dim3(64), 0, s, sc.prow, sc.pval,
                       a.ns, a.nchunks, a.d_ft, sh.HD, a.HDp, a.d_el, sh.H);
  }
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

// V = 8 exists only for 16-bit elements (16-byte slabs)
template <typename T, typename Idx>
int train_typed(bool backward, const dgla_csr* csc, const dgla_csr* csr, const Shape& sh, const WidePtrs& q, float slope,
                const Drop& dr, char* ws, hipStream_t s) {
#define DGLA_GATT_V(VV)                                                                   \
  return backward ? backward_train_v<T, VV, Idx>(csc, csr, sh, q, slope, dr, ws, s)       \
                  : forward_train_v<T, VV, Idx>(csc, sh, q, slope, dr, ws, s)
  if constexpr (sizeof(T) == 2) {
    if (sh.V == 8) DGLA_GATT_V(8);
  }
  switch (sh.V) {
    case 4: DGLA_GATT_V(4);
    case 2: DGLA_GATT_V(2);
    default: DGLA_GATT_V(1);
  }
#undef DGLA_GATT_V
}

int train(bool backward, dgla_dtype dtype, const dgla_csr* csc, const dgla_csr* csr, const Shape& sh, const WidePtrs& q,
          float slope, const Drop& dr, char* ws, hipStream_t s) {
  const bool i32 = csc->idtype_bits == 32;
  switch (dtype) {
    case DGLA_F16:
      return i32 ? train_typed<f16_t, int32_t>(backward, csc, csr, sh, q, slope, dr, ws, s)
                 : train_typed<f16_t, int64_t>(backward, csc, csr, sh, q, slope, dr, ws, s);
    case DGLA_BF16:
      return i32 ? train_typed<bf16_t, int32_t>(backward, csc, csr, sh, q, slope, dr, ws, s)
                 : train_typed<bf16_t, int64_t>(backward, csc, csr, sh, q, slope, dr, ws, s);
    default:
      return i32 ? train_typed<float, int32_t>(backward, csc, csr, sh, q, slope, dr, ws, s)
                 : train_typed<float, int64_t>(backward, csc, csr, sh, q, slope, dr, ws, s);
  }
}

template <typename T, typename Idx>
int weights_typed(const dgla_csr* csc, int H, const void* el, const void* er, const float* mz, float slope, const Drop& dr,
                  void* attn, hipStream_t s) {
  hipLaunchKernelGGL((gat_weights_kernel<T, Idx>), dim3(grid1(csc->nnz)), dim3(256), 0, s,
                     static_cast<const Idx*>(csc->indptr), static_cast<const Idx*>(csc->indices),
                     static_cast<const Idx*>(csc->data), csc->num_rows, csc->nnz, H, slope, dr.seed, dr.threshold, dr.scale,
                     static_cast<const T*>(el), static_cast<const T*>(er), mz, static_cast<T*>(attn));
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int drop_of(const char* who, float p, uint64_t seed, Drop* dr) {
  dr->seed = seed;
  if (!gat_dropout_params(p, &dr->threshold, &dr->scale))
    return fail(std::string(who) + ": the dropout probability p must lie in [0, 1)");
  return 0;
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

int dgla_gat_attention_train_forward(const dgla_csr* csc, dgla_dtype dtype, const dgla_tensor* ft, const dgla_tensor* el,
                                     const dgla_tensor* er, float negative_slope, float p, uint64_t seed,
                                     const dgla_tensor* out, void* mz, void* workspace, size_t workspace_bytes,
                                     void* hip_stream) {
  if (!csc || !present(out) || (!mz && csc->num_rows > 0))
    return fail("gat_attention_train_forward: csc / out / mz are required");
  Drop dr;
  if (drop_of("gat_attention_train_forward", p, seed, &dr)) return -1;
  Shape sh;
  if (shape_of(dtype, ft, el, er, &sh)) return -1;
  if (csc->idtype_bits != 32 && csc->idtype_bits != 64) return fail("idtype must be int32 or int64");
  if (ft->shape[0] != csc->num_cols || er->shape[0] != csc->num_rows || out->ndim != 3 ||
      out->shape[0] != csc->num_rows || out->shape[1] != sh.H || out->shape[2] != sh.D)
    return fail("gat_attention_train_forward: tensor shapes do not match the graph");
  if (csc->nnz > 0 && (!workspace || workspace_bytes < dgla_gat_attention_workspace_bytes(csc, sh.H, sh.D)))
    return fail("gat_attention_train_forward: workspace too small (dgla_gat_attention_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out->data);
  WidePtrs q{};
  q.ft = ft->data;
  q.el = el->data;
  q.er = er->data;
  q.out = out->data;
  q.mz = static_cast<float*>(mz);
  return train(false, dtype, csc, nullptr, sh, q, negative_slope, dr, static_cast<char*>(workspace), s);
}

int dgla_gat_attention_train_backward(const dgla_csr* csc, const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* ft,
                                      const dgla_tensor* el, const dgla_tensor* er, const void* mz, const dgla_tensor* dout,
                                      float negative_slope, float p, uint64_t seed, const dgla_tensor* d_ft,
                                      const dgla_tensor* d_el, const dgla_tensor* d_er, void* workspace,
                                      size_t workspace_bytes, void* hip_stream) {
  if (!csc || !csr || !present(dout) || !present(d_ft) || !present(d_el) || !present(d_er) || (!mz && csc->num_rows > 0))
    return fail("gat_attention_train_backward: every tensor is required");
  Drop dr;
  if (drop_of("gat_attention_train_backward", p, seed, &dr)) return -1;
  Shape sh;
  if (shape_of(dtype, ft, el, er, &sh)) return -1;
  if (csc->idtype_bits != csr->idtype_bits || (csc->idtype_bits != 32 && csc->idtype_bits != 64))
    return fail("gat_attention_train_backward: the two CSRs must share one id type (int32 or int64)");
  if (csc->nnz != csr->nnz || csc->num_rows != csr->num_cols || csc->num_cols != csr->num_rows)
    return fail("gat_attention_train_backward: csr is not the out-edge CSR of csc's graph");
  if (ft->shape[0] != csc->num_cols || er->shape[0] != csc->num_rows)
    return fail("gat_attention_train_backward: tensor shapes do not match the graph");
  if (dout->ndim != 3 || dout->shape[0] != csc->num_rows || dout->shape[1] != sh.H || dout->shape[2] != sh.D)
    return fail("gat_attention_train_backward: dout must be (N_dst, H, D)");
  if (d_ft->ndim != 3 || d_ft->shape[0] != ft->shape[0] || d_ft->shape[1] != sh.H || d_ft->shape[2] != sh.D ||
      d_el->ndim != 3 || d_el->shape[0] != el->shape[0] || d_el->shape[1] != sh.H || d_el->shape[2] != 1 ||
      d_er->ndim != 3 || d_er->shape[0] != er->shape[0] || d_er->shape[1] != sh.H || d_er->shape[2] != 1)
    return fail("gat_attention_train_backward: d_ft / d_el / d_er must have the shapes of ft / el / er");
  if (csc->nnz > 0 && (!workspace || workspace_bytes < dgla_gat_attention_workspace_bytes(csc, sh.H, sh.D)))
    return fail("gat_attention_train_backward: workspace too small (dgla_gat_attention_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, d_ft->data);
  WidePtrs q{};
  q.ft = ft->data;
  q.el = el->data;
  q.er = er->data;
  q.dout = dout->data;
  q.mz = const_cast<float*>(static_cast<const float*>(mz));
  q.d_ft = d_ft->data;
  q.d_el = d_el->data;
  q.d_er = d_er->data;
  return train(true, dtype, csc, csr, sh, q, negative_slope, dr, static_cast<char*>(workspace), s);
}

int dgla_gat_attention_weights(const dgla_csr* csc, dgla_dtype dtype, const dgla_tensor* el, const dgla_tensor* er,
                               const void* mz, float negative_slope, float p, uint64_t seed, const dgla_tensor* attn,
                               void* hip_stream) {
  if (!csc || !present(el) || !present(er) || !present(attn) || (!mz && csc->num_rows > 0))
    return fail("gat_attention_weights: csc / el / er / mz / attn are required");
  Drop dr;
  if (drop_of("gat_attention_weights", p, seed, &dr)) return -1;
  if (dtype != DGLA_F32 && dtype != DGLA_F16 && dtype != DGLA_BF16)
    return fail("gat_attention_weights: needs fp32 / fp16 / bf16 operands");
  if (csc->idtype_bits != 32 && csc->idtype_bits != 64) return fail("idtype must be int32 or int64");
  if (el->ndim != 3 || er->ndim != 3 || el->shape[2] != 1 || er->shape[2] != 1 || el->shape[1] != er->shape[1] ||
      el->shape[1] < 1 || el->shape[1] > 64 || el->shape[0] != csc->num_cols || er->shape[0] != csc->num_rows)
    return fail("gat_attention_weights: el must be (N_src, H, 1), er (N_dst, H, 1) with 1 <= H <= 64");
  const int H = static_cast<int>(el->shape[1]);
  if ((attn->ndim != 2 && attn->ndim != 3) || attn->shape[0] != csc->nnz || attn->shape[1] != H ||
      (attn->ndim == 3 && attn->shape[2] != 1))
    return fail("gat_attention_weights: attn must be (E, H, 1)");
  if (csc->nnz <= 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, attn->data);
  const float* mzf = static_cast<const float*>(mz);
  const bool i32 = csc->idtype_bits == 32;
#define DGLA_GATT_W(T) \
  (i32 ? weights_typed<T, int32_t>(csc, H, el->data, er->data, mzf, negative_slope, dr, attn->data, s) \
       : weights_typed<T, int64_t>(csc, H, el->data, er->data, mzf, negative_slope, dr, attn->data, s))
  switch (dtype) {
    case DGLA_F16: return DGLA_GATT_W(f16_t);
    case DGLA_BF16: return DGLA_GATT_W(bf16_t);
    default: return DGLA_GATT_W(float);
  }
#undef DGLA_GATT_W
}

int dgla_gat_dropout_mask_host(uint64_t seed, float p, const int64_t* eids, int64_t n, int heads, uint8_t* keep) {
  uint32_t threshold;
  float scale;
  if (!gat_dropout_params(p, &threshold, &scale))
    return fail("gat_dropout_mask_host: the dropout probability p must lie in [0, 1)");
  if (n < 0 || heads < 1 || (n > 0 && (!eids || !keep))) return fail("gat_dropout_mask_host: eids / keep / heads are required");
  for (int64_t i = 0; i < n; ++i)
    for (int h = 0; h < heads; ++h)
      keep[i * heads + h] = gat_keep(seed, static_cast<uint64_t>(eids[i]), h, threshold) ? 1 : 0;
  return 0;
}

}  // extern "C"
