// Sparse x sparse on the device: CSRMM (C = A . B), CSRSum (C = sum_k A_k) and CSRMask (out[e] = A[row_B[e], col_B[e]]).
//
// Reference: aten::CSRMM / CSRSum / CSRGetData behind _CAPI_DGLCSRMM / _CAPI_DGLCSRSum / _CAPI_DGLCSRMask
// (src/array/kernel.cc:725-800); CPU kernels src/array/cpu/csr_mm.cc:20-130 (two passes over a per-thread hash map, hash
// order inside a row) and csr_sum.cc; GPU kernels src/array/cuda/csr_mm.cu / csr_sum.cu (cusparseSpGEMM / csrgeam2, row
// order whatever the vendor library leaves, a 2^31 limit on the sizes).  Weights are one scalar per edge and are read
// through the edge-id map: w[data ? data[pos] : pos] (csr_mm.cc:67-70).
//
// Contract of this unit:
//   * structure of C = the structural product / union: an entry exists wherever at least one term exists, also when the
//     terms cancel to 0.0; C has no edge-id map; columns ascend strictly inside a row; same structure on every run;
//   * values: fp32 / fp64 in their own arithmetic; fp16 / bf16 widened on load, multiplied and added in fp32 and rounded
//     ONCE at the store; the terms of one entry are added in a fixed order (for the product: position order of A's row,
//     the sum: operand order) — no floating-point atomics anywhere, a second launch gives the same bits;
//   * operands are simple graphs (no duplicate column inside a row), as the reference requires;
//   * sizes: term counts and nnz(C) are int64 inside the unit; with int32 ids an nnz(C) above 2^31 - 1 is an error.
//
// Two calls around one workspace, every output allocated by the caller: `count` writes C's indptr and returns nnz(C) (the
// one host synchronisation, which the reference pays too), `fill` writes indices and weights.  Both run the same
// machinery with and without values:
//   bound    ub[i] = number of terms of row i (product: sum of deg_B over the entries of A's row i), one wavefront per row;
//   classes  by ub (dgla_csr_mm_row_classes):  0 -> empty;  <= kWaveMax -> one wavefront per row;  <= kBlockMax -> one
//            256-thread workgroup per row; both expand the terms into LDS as (column, sequence number, value), order them
//            with a bitonic network on the unique key (column, sequence) and let the head of every run of equal columns add
//            its run front to back;  above kBlockMax -> one wavefront per row walks column windows of kSpaWindow columns with
//            a dense accumulator in LDS: the terms' sources (rows of B / operands) are visited one after the other, the
//            lanes spread over ONE source row, whose columns are distinct — so no two lanes meet in a slot and the order of
//            additions is the order of the sources.  No path needs global scratch beyond ub and the row counts.
#include "../../include/dgl_amd.h"

#include <vector>

#include "host_util.h"
#include "sort.hip.h"

namespace dgla {
namespace spgemm {

constexpr int kWaveMax = 64;       // terms of a row handled by one wavefront
constexpr int kBlockMax = 2048;    // terms of a row handled by one workgroup in LDS (36 KiB with fp64 values: 4 per CU)
constexpr int kSpaWindow = 4096;   // columns per dense-accumulator window (36 KiB with fp64 values)

template <typename Idx>
struct Operand {   // one CSR operand on the device
  const Idx* indptr;
  const Idx* indices;
  const Idx* data;
  const void* w;
};

// ---- where the terms of an output row come from ---------------------------------------------------------------------
// A source = one row of B (product) / row i of one operand (sum); term u of output row i scales source u by `scale`.
template <typename Idx, typename T>
struct MmSrc {
  using A = typename Acc<T>::type;
  Operand<Idx> a, b;
  __device__ __forceinline__ int64_t begin(int64_t row) const { return static_cast<int64_t>(a.indptr[row]); }
  __device__ __forceinline__ int64_t end(int64_t row) const { return static_cast<int64_t>(a.indptr[row + 1]); }
  template <bool VAL>
  __device__ __forceinline__ void source(int64_t, int64_t u, A* scale, int64_t* p0, int64_t* p1) const {
    const int64_t k = static_cast<int64_t>(a.indices[u]);
    *p0 = static_cast<int64_t>(b.indptr[k]);
    *p1 = static_cast<int64_t>(b.indptr[k + 1]);
    if constexpr (VAL) *scale = to_acc(static_cast<const T*>(a.w)[a.data ? static_cast<int64_t>(a.data[u]) : u]);
  }
  __device__ __forceinline__ int64_t col(int64_t, int64_t p) const { return static_cast<int64_t>(b.indices[p]); }
  __device__ __forceinline__ A term(int64_t, int64_t p, A scale) const {
    return scale * to_acc(static_cast<const T*>(b.w)[b.data ? static_cast<int64_t>(b.data[p]) : p]);
  }
};

template <typename Idx, typename T>
struct SumSrc {
  using A = typename Acc<T>::type;
  const Operand<Idx>* ops;   // device table
  int n;
  __device__ __forceinline__ int64_t begin(int64_t) const { return 0; }
  __device__ __forceinline__ int64_t end(int64_t) const { return n; }
  template <bool VAL>
  __device__ __forceinline__ void source(int64_t row, int64_t u, A* scale, int64_t* p0, int64_t* p1) const {
    *p0 = static_cast<int64_t>(ops[u].indptr[row]);
    *p1 = static_cast<int64_t>(ops[u].indptr[row + 1]);
    if constexpr (VAL) *scale = A(1);
  }
  __device__ __forceinline__ int64_t col(int64_t u, int64_t p) const { return static_cast<int64_t>(ops[u].indices[p]); }
  __device__ __forceinline__ A term(int64_t u, int64_t p, A) const {
    const Operand<Idx>& o = ops[u];
    return to_acc(static_cast<const T*>(o.w)[o.data ? static_cast<int64_t>(o.data[p]) : p]);
  }
};

// ---- bound pass: ub[row] = number of terms, one wavefront per row ------------------------------------------------------
template <typename Src>
__global__ __launch_bounds__(256) void bound_kernel(const Src src, int64_t num_rows, int64_t* __restrict__ ub) {
  const int64_t row = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (row >= num_rows) return;   // (whole wavefronts leave together)
  const int lane = threadIdx.x & 63;
  int64_t s = 0;
  for (int64_t u = src.begin(row) + lane; u < src.end(row); u += 64) {
    typename Src::A unused;
    int64_t p0, p1;
    src.template source<false>(row, u, &unused, &p0, &p1);
    s += p1 - p0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) ub[row] = s;
}

// ---- classes 1 and 2: expand -> sort by (column, sequence) -> segmented sum, all in LDS --------------------------------
// One workgroup of NT threads per row whose term count lies in [lo, hi], hi <= CAP.  FILL = false counts the distinct
// columns into cnt[row]; FILL = true writes them and their sums at c_indptr[row].
template <typename Idx, typename T, typename Src, int NT, int CAP, bool FILL>
__global__ __launch_bounds__(NT) void row_sort_kernel(const Src src, const int64_t* __restrict__ ub, int64_t lo, int64_t hi,
                                                     int64_t* __restrict__ cnt, const Idx* __restrict__ c_indptr,
                                                     Idx* __restrict__ c_indices, T* __restrict__ c_w) {
  using A = typename Acc<T>::type;
  __shared__ unsigned long long kc[CAP];   // column of the slot
  __shared__ uint16_t ks[CAP];             // sequence number of the term in the slot (CAP <= 65536)
  __shared__ A val[FILL ? CAP : 1];        // value of term `sequence number` (values do not move)
  __shared__ int wsum[NT / 64];
  const int64_t row = blockIdx.x;
  const int64_t n64 = ub[row];
  if (n64 < lo || n64 > hi) return;
  const int n = static_cast<int>(n64);
  const int tid = threadIdx.x;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  // expand: thread t takes source u0 + t, the sources' term ranges follow each other in source order
  int running = 0;
  const int64_t u_end = src.end(row);
  for (int64_t u0 = src.begin(row); u0 < u_end; u0 += NT) {
    const int64_t u = u0 + tid;
    int64_t p0 = 0, p1 = 0;
    A scale = A(0);
    if (u < u_end) src.template source<FILL>(row, u, &scale, &p0, &p1);
    int total;
    const int off = running + msd::block_exclusive_scan<NT>(static_cast<int>(p1 - p0), &total, wsum);
    for (int64_t p = p0; p < p1; ++p) {
      const int slot = off + static_cast<int>(p - p0);
      if (slot < n) {   // (always, for a consistent indptr)
        kc[slot] = static_cast<unsigned long long>(src.col(u, p));
        ks[slot] = static_cast<uint16_t>(slot);
        if constexpr (FILL) val[slot] = src.term(u, p, scale);
      }
    }
    running += total;
  }
  for (int i = n + tid; i < n2; i += NT) {   // padding sorts behind every column
    kc[i] = ~0ull;
    ks[i] = static_cast<uint16_t>(i);
  }
  __syncthreads();
  // bitonic network over n2 slots; the key (column, sequence) is unique, so the result does not depend on the network
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += NT) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long ci = kc[i], cl = kc[l];
          const uint16_t si = ks[i], sl = ks[l];
          const bool gt = ci > cl || (ci == cl && si > sl);
          if (gt == ((i & k) == 0)) {
            kc[i] = cl;
            kc[l] = ci;
            ks[i] = sl;
            ks[l] = si;
          }
        }
      }
      __syncthreads();
    }
  }
  // heads of the runs of equal columns; thread t owns the consecutive slots [t * per, t * per + per)
  const int per = (n + NT - 1) / NT;
  const int s0 = tid * per, s1 = s0 + per < n ? s0 + per : n;
  int heads = 0;
  for (int s = s0; s < s1; ++s) heads += (s == 0 || kc[s] != kc[s - 1]) ? 1 : 0;
  int total;
  int at = msd::block_exclusive_scan<NT>(heads, &total, wsum);
  if constexpr (!FILL) {
    if (tid == 0) cnt[row] = total;
  } else {
    const int64_t base = static_cast<int64_t>(c_indptr[row]);
    for (int s = s0; s < s1; ++s) {
      const unsigned long long c = kc[s];
      if (s == 0 || c != kc[s - 1]) {
        A sum = val[ks[s]];
        for (int r = s + 1; r < n && kc[r] == c; ++r) sum += val[ks[r]];   // ascending sequence number: a fixed order
        c_indices[base + at] = static_cast<Idx>(c);
        c_w[base + at] = from_acc<T>(sum);
        ++at;
      }
    }
  }
}

// ---- class 3: dense accumulator over column windows, one wavefront per row ---------------------------------------------
template <typename Idx, typename T, typename Src, bool FILL>
__global__ __launch_bounds__(64) void row_spa_kernel(const Src src, const int64_t* __restrict__ ub, int64_t lo,
                                                    int64_t* __restrict__ cnt, const Idx* __restrict__ c_indptr,
                                                    Idx* __restrict__ c_indices, T* __restrict__ c_w) {
  using A = typename Acc<T>::type;
  __shared__ A acc[FILL ? kSpaWindow : 1];
  __shared__ uint8_t flag[kSpaWindow];
  const int64_t row = blockIdx.x;
  if (ub[row] <= lo) return;
  const int lane = threadIdx.x;
  const int64_t u_begin = src.begin(row), u_end = src.end(row);
  // the row's column range, so that only windows that can hold something are walked
  int64_t cmin = INT64_MAX, cmax = -1;
  for (int64_t u = u_begin; u < u_end; ++u) {
    A scale;
    int64_t p0, p1;
    src.template source<false>(row, u, &scale, &p0, &p1);
    for (int64_t p = p0 + lane; p < p1; p += 64) {
      const int64_t c = src.col(u, p);
      cmin = c < cmin ? c : cmin;
      cmax = c > cmax ? c : cmax;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t a = __shfl_xor(cmin, d, 64), b = __shfl_xor(cmax, d, 64);
    cmin = a < cmin ? a : cmin;
    cmax = b > cmax ? b : cmax;
  }
  int64_t written = 0;
  const int64_t base = FILL ? static_cast<int64_t>(c_indptr[row]) : 0;
  for (int64_t c0 = cmin; c0 <= cmax; c0 += kSpaWindow) {
    for (int i = lane; i < kSpaWindow; i += 64) flag[i] = 0;
    __syncthreads();
    for (int64_t u = u_begin; u < u_end; ++u) {   // sources one after the other: the order of additions
      A scale = A(0);
      int64_t p0, p1;
      src.template source<FILL>(row, u, &scale, &p0, &p1);
      for (int64_t p = p0 + lane; p < p1; p += 64) {   // one source row: distinct columns, no two lanes in one slot
        const int64_t c = src.col(u, p) - c0;
        if (c >= 0 && c < kSpaWindow) {
          if constexpr (FILL) {
            const A x = src.term(u, p, scale);
            acc[c] = flag[c] ? acc[c] + x : x;
          }
          flag[c] = 1;
        }
      }
      __syncthreads();
    }
    // emit in column order: lane l owns the slots [64 l, 64 l + 64)
    constexpr int kPer = kSpaWindow / 64;
    int have = 0;
    for (int i = 0; i < kPer; ++i) have += flag[lane * kPer + i];
    int total;
    int at = msd::block_exclusive_scan<64>(have, &total, nullptr);
    if constexpr (FILL) {
      for (int i = 0; i < kPer; ++i) {
        const int sl = lane * kPer + i;
        if (flag[sl]) {
          c_indices[base + written + at] = static_cast<Idx>(c0 + sl);
          c_w[base + written + at] = from_acc<T>(acc[sl]);
          ++at;
        }
      }
    }
    written += total;
    __syncthreads();
  }
  if constexpr (!FILL) {
    if (lane == 0) cnt[row] = written;
  }
}

template <typename Idx>
__global__ __launch_bounds__(256) void indptr_kernel(const int64_t* __restrict__ off, int64_t n, Idx* __restrict__ indptr) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) indptr[i] = static_cast<Idx>(off[i]);
}

// ---- workspace ------------------------------------------------------------------------------------------------------------
struct Layout {
  size_t off_ub = 0, off_cnt = 0, off_scan = 0, off_ops = 0, bytes = 0;
};
inline Layout layout_for(int64_t num_rows, int n_ops, int idbits) {
  Layout l;
  Carver c;
  l.off_ub = c.take(sizeof(int64_t) * static_cast<size_t>(num_rows + 1));
  l.off_cnt = c.take(sizeof(int64_t) * static_cast<size_t>(num_rows + 1));
  l.off_scan = c.take(msd::scan_temp_bytes(num_rows + 1, sizeof(int64_t)));
  l.off_ops = c.take((idbits == 32 ? sizeof(Operand<int32_t>) : sizeof(Operand<int64_t>)) * static_cast<size_t>(n_ops));
  l.bytes = c.bytes();
  return l;
}

// the three class launches over all rows; terms == 0: nothing to do (every row is empty)
template <typename Idx, typename T, typename Src, bool FILL>
int launch_classes(const Src& src, int64_t num_rows, const int64_t* ub, int64_t* cnt, const void* c_indptr, void* c_indices,
                   void* c_w, hipStream_t s) {
  if (num_rows <= 0) return 0;
  const dim3 grid(static_cast<unsigned>(num_rows));
  const Idx* ip = static_cast<const Idx*>(c_indptr);
  Idx* ix = static_cast<Idx*>(c_indices);
  T* w = static_cast<T*>(c_w);
  hipLaunchKernelGGL((row_sort_kernel<Idx, T, Src, 64, kWaveMax, FILL>), grid, dim3(64), 0, s, src, ub, int64_t(1),
                     int64_t(kWaveMax), cnt, ip, ix, w);
  hipLaunchKernelGGL((row_sort_kernel<Idx, T, Src, 256, kBlockMax, FILL>), grid, dim3(256), 0, s, src, ub,
                     int64_t(kWaveMax + 1), int64_t(kBlockMax), cnt, ip, ix, w);
  hipLaunchKernelGGL((row_spa_kernel<Idx, T, Src, FILL>), grid, dim3(64), 0, s, src, ub, int64_t(kBlockMax), cnt, ip, ix, w);
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename Src>
int launch_bound(const Src& src, int64_t num_rows, int64_t* ub, hipStream_t s) {
  if (num_rows <= 0) return 0;
  hipLaunchKernelGGL(bound_kernel<Src>, dim3(static_cast<unsigned>((num_rows + 3) / 4)), dim3(256), 0, s, src, num_rows, ub);
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

// count: bound -> classes -> scan -> indptr -> nnz to the host
template <typename Idx, typename Src>
int count_rows(const Src& src, int64_t num_rows, bool any_terms, void* c_indptr, int64_t* nnz_out, char* ws, const Layout& l,
               hipStream_t s) {
  int64_t* ub = reinterpret_cast<int64_t*>(ws + l.off_ub);
  int64_t* cnt = reinterpret_cast<int64_t*>(ws + l.off_cnt);
  DGLA_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int64_t) * static_cast<size_t>(num_rows + 1), s));
  if (any_terms) {
    if (launch_bound(src, num_rows, ub, s)) return -1;
    if (launch_classes<Idx, float, Src, false>(src, num_rows, ub, cnt, nullptr, nullptr, nullptr, s)) return -1;
    if (msd::exclusive_scan<int64_t, int64_t>(cnt, cnt, num_rows + 1, ws + l.off_scan, s)) return -1;
  }
  hipLaunchKernelGGL(indptr_kernel<Idx>, dim3(static_cast<unsigned>((num_rows + 1 + 255) / 256)), dim3(256), 0, s, cnt,
                     num_rows + 1, static_cast<Idx*>(c_indptr));
  int64_t nnz = 0;
  if (read_back(&nnz, cnt + num_rows, sizeof(int64_t), s)) return -1;  // (0 without terms: cnt was cleared above)
  if (sizeof(Idx) == 4 && nnz > 0x7fffffffLL)
    return fail("csr_mm: the result has " + std::to_string(nnz) + " entries, which int32 ids cannot address; use int64 ids");
  *nnz_out = nnz;
  return 0;
}

template <typename Idx, typename T, typename Src>
int fill_rows(const Src& src, int64_t num_rows, const void* c_indptr, void* c_indices, void* c_w, char* ws, const Layout& l,
              hipStream_t s) {
  int64_t* ub = reinterpret_cast<int64_t*>(ws + l.off_ub);
  if (launch_bound(src, num_rows, ub, s)) return -1;
  return launch_classes<Idx, T, Src, true>(src, num_rows, ub, nullptr, c_indptr, c_indices, c_w, s);
}

template <typename Idx>
Operand<Idx> operand_of(const dgla_csr* c, const void* w) {
  const TypedCsr<Idx> g(c);
  return Operand<Idx>{g.indptr, g.indices, g.data, w};
}

// one operand; `who` names the entry point and the operand
int check_operand(const char* who, const dgla_csr* c) {
  if (check_csr(who, c, kCsrCols | kCsrEmptyIndptr)) return -1;
  if (c->idtype_bits == 32 && (c->num_rows > 0x7fffffffLL || c->num_cols > 0x7fffffffLL || c->nnz > 0x7fffffffLL))
    return fail(who, "int32 ids cannot address this matrix");
  if (c->num_rows > 0x7fffffffLL) return fail(who, "more than 2^31 - 1 rows");   // (one workgroup per row)
  return 0;
}

int check_mm(const dgla_csr* a, const dgla_csr* b) {
  if (check_operand("csr_mm: a", a) || check_operand("csr_mm: b", b)) return -1;
  if (a->idtype_bits != b->idtype_bits) return fail("csr_mm: the operands have different id types");
  if (a->num_cols != b->num_rows)
    return fail("csr_mm: a has " + std::to_string(a->num_cols) + " columns but b has " + std::to_string(b->num_rows) + " rows");
  return 0;
}

int check_sum(const dgla_csr* const* ops, int n) {
  if (!ops || n < 1) return fail("csr_sum: at least one operand is required");
  for (int k = 0; k < n; ++k) {
    if (check_operand("csr_sum: operand", ops[k])) return -1;
    if (ops[k]->idtype_bits != ops[0]->idtype_bits) return fail("csr_sum: the operands have different id types");
    if (ops[k]->num_rows != ops[0]->num_rows || ops[k]->num_cols != ops[0]->num_cols)
      return fail("csr_sum: the operands have different shapes");
  }
  return 0;
}

// the operand table of a sum, copied to the workspace (the host vector lives until the call returns; a pageable source
// has been staged by then)
template <typename Idx>
int upload_ops(const dgla_csr* const* ops, const void* const* w, int n, std::vector<Operand<Idx>>* host, char* dst,
               hipStream_t s) {
  host->resize(n);
  for (int k = 0; k < n; ++k) (*host)[k] = operand_of<Idx>(ops[k], w ? w[k] : nullptr);
  DGLA_CHECK_HIP(hipMemcpyAsync(dst, host->data(), sizeof(Operand<Idx>) * n, hipMemcpyHostToDevice, s));
  return 0;
}

// ---- CSRMask ---------------------------------------------------------------------------------------------------------------
// flag stays 1 iff the columns ascend strictly in every row (one wavefront per row)
template <typename Idx>
__global__ __launch_bounds__(256) void ascending_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                       int64_t num_rows, int* __restrict__ flag) {
  const int64_t row = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (row >= num_rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t e = static_cast<int64_t>(indptr[row + 1]);
  bool bad = false;
  for (int64_t p = static_cast<int64_t>(indptr[row]) + lane; p + 1 < e; p += 64) bad |= indices[p] >= indices[p + 1];
  if (bad) *flag = 0;   // (every writer stores the same value)
}

static __global__ void set_flag_kernel(int* flag) { *flag = 1; }

constexpr int kMaskGroup = 8;   // lanes per query
template <typename Idx, typename T>
__global__ __launch_bounds__(256) void mask_kernel(const Operand<Idx> a, int64_t a_rows, const Idx* __restrict__ b_row,
                                                  const Idx* __restrict__ b_col, const Idx* __restrict__ b_data, int64_t nq,
                                                  const int* __restrict__ ascending, T* __restrict__ out) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t q = g / kMaskGroup;
  const int sub = static_cast<int>(g % kMaskGroup);
  int64_t found = INT64_MAX;
  if (q < nq) {
    const int64_t r = static_cast<int64_t>(b_row[q]);
    const Idx c = b_col[q];
    if (r >= 0 && r < a_rows) {
      int64_t lo = static_cast<int64_t>(a.indptr[r]), hi = static_cast<int64_t>(a.indptr[r + 1]);
      if (*ascending) {
        if (sub == 0) {   // bisection
          while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            const Idx x = a.indices[mid];
            if (x < c) {
              lo = mid + 1;
            } else {
              hi = mid;
              if (x == c) found = mid;
            }
          }
        }
      } else {          // strided scan, the smallest matching position wins
        for (int64_t p = lo + sub; p < hi; p += kMaskGroup)
          if (a.indices[p] == c) {
            found = p;
            break;
          }
      }
    }
  }
#pragma unroll
  for (int d = kMaskGroup / 2; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor(found, d, kMaskGroup);
    found = o < found ? o : found;
  }
  if (q < nq && sub == 0) {
    T v = from_acc<T>(typename Acc<T>::type(0));
    if (found != INT64_MAX) v = static_cast<const T*>(a.w)[a.data ? static_cast<int64_t>(a.data[found]) : found];
    out[b_data ? static_cast<int64_t>(b_data[q]) : q] = v;
  }
}

template <typename Idx, typename T>
int run_mask(const dgla_csr* a, const void* a_w, const dgla_coo* b, void* out, hipStream_t s) {
  if (b->nnz == 0) return 0;
  int* flag = nullptr;
  DGLA_CHECK_HIP(hipMallocAsync(reinterpret_cast<void**>(&flag), sizeof(int), s));
  hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, s, flag);
  const Operand<Idx> op = operand_of<Idx>(a, a_w);
  if (a->num_rows > 0 && a->nnz > 0)
    hipLaunchKernelGGL(ascending_kernel<Idx>, dim3(static_cast<unsigned>((a->num_rows + 3) / 4)), dim3(256), 0, s, op.indptr,
                       op.indices, a->num_rows, flag);
  const int64_t threads = b->nnz * kMaskGroup;
  hipLaunchKernelGGL((mask_kernel<Idx, T>), dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, op,
                     a->nnz > 0 ? a->num_rows : int64_t(0), static_cast<const Idx*>(b->row), static_cast<const Idx*>(b->col),
                     static_cast<const Idx*>(b->data), b->nnz, flag, static_cast<T*>(out));
  const hipError_t e = hipGetLastError();
  (void)hipFreeAsync(flag, s);
  DGLA_CHECK_HIP(e);
  return 0;
}

#define DGLA_SPGEMM_DTYPE(DT, IDX, CALL)                                 \
  switch (DT) {                                                          \
    case DGLA_F32: { using T = float; return CALL; }                     \
    case DGLA_F64: { using T = double; return CALL; }                    \
    case DGLA_F16: { using T = f16_t; return CALL; }                     \
    case DGLA_BF16: { using T = bf16_t; return CALL; }                   \
    default: return fail("csr_mm: unknown dtype");                      \
  }

template <typename Idx>
int mm_fill(const dgla_csr* a, dgla_dtype dt, const void* a_w, const dgla_csr* b, const void* b_w, const void* c_indptr,
            void* c_indices, void* c_w, char* ws, const Layout& l, hipStream_t s) {
  DGLA_SPGEMM_DTYPE(dt, Idx, (fill_rows<Idx, T>(MmSrc<Idx, T>{operand_of<Idx>(a, a_w), operand_of<Idx>(b, b_w)}, a->num_rows,
                                                c_indptr, c_indices, c_w, ws, l, s)))
}

template <typename Idx>
int sum_fill(const Operand<Idx>* table, int n, int64_t num_rows, dgla_dtype dt, const void* c_indptr, void* c_indices, void* c_w,
             char* ws, const Layout& l, hipStream_t s) {
  DGLA_SPGEMM_DTYPE(dt, Idx, (fill_rows<Idx, T>(SumSrc<Idx, T>{table, n}, num_rows, c_indptr, c_indices, c_w, ws, l, s)))
}

template <typename Idx>
int mask_dispatch(const dgla_csr* a, dgla_dtype dt, const void* a_w, const dgla_coo* b, void* out, hipStream_t s) {
  DGLA_SPGEMM_DTYPE(dt, Idx, (run_mask<Idx, T>(a, a_w, b, out, s)))
}

}  // namespace spgemm
}  // namespace dgla

using namespace dgla;
using namespace dgla::spgemm;

extern "C" {

int dgla_csr_mm_row_classes(int64_t* bounds, int max) {
  const int64_t b[2] = {kWaveMax, kBlockMax};
  for (int i = 0; i < 2 && i < max && bounds; ++i) bounds[i] = b[i];
  return 2;
}

size_t dgla_csr_mm_workspace_bytes(const dgla_csr* a, const dgla_csr* b) {
  if (!a || !b || a->num_rows < 0) return 0;
  return layout_for(a->num_rows, 0, a->idtype_bits).bytes;
}

int dgla_csr_mm_count(const dgla_csr* a, const dgla_csr* b, void* c_indptr, int64_t* nnz_out, void* workspace,
                      size_t workspace_bytes, void* hip_stream) {
  if (check_mm(a, b)) return -1;
  if (!c_indptr || !nnz_out) return fail("csr_mm: c_indptr / nnz_out is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, c_indptr);
  const Layout l = layout_for(a->num_rows, 0, a->idtype_bits);
  Scratch ws(s);
  if (ws.take(workspace, workspace_bytes, l.bytes)) return -1;
  const bool any = a->nnz > 0 && b->nnz > 0;
  return with_idx(a->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    return count_rows<Idx>(MmSrc<Idx, float>{operand_of<Idx>(a, nullptr), operand_of<Idx>(b, nullptr)}, a->num_rows, any,
                           c_indptr, nnz_out, ws.p, l, s);
  });
}

int dgla_csr_mm_fill(const dgla_csr* a, dgla_dtype dtype, const void* a_w, const dgla_csr* b, const void* b_w,
                     const void* c_indptr, void* c_indices, void* c_w, void* workspace, size_t workspace_bytes,
                     void* hip_stream) {
  if (check_mm(a, b)) return -1;
  if (!c_indptr) return fail("csr_mm: c_indptr is null");
  if (a->nnz == 0 || b->nnz == 0 || a->num_rows == 0) return 0;   // C has no entries
  if (!a_w || !b_w) return fail("csr_mm: the weights of a / b are null");
  if (!c_indices || !c_w) return fail("csr_mm: c_indices / c_w is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, c_indptr);
  const Layout l = layout_for(a->num_rows, 0, a->idtype_bits);
  Scratch ws(s);
  if (ws.take(workspace, workspace_bytes, l.bytes)) return -1;
  return with_idx(a->idtype_bits, [&](auto tag) {
    return mm_fill<decltype(tag)>(a, dtype, a_w, b, b_w, c_indptr, c_indices, c_w, ws.p, l, s);
  });
}

size_t dgla_csr_sum_workspace_bytes(const dgla_csr* const* ops, int n) {
  if (!ops || n < 1 || !ops[0] || ops[0]->num_rows < 0) return 0;
  return layout_for(ops[0]->num_rows, n, ops[0]->idtype_bits).bytes;
}

int dgla_csr_sum_count(const dgla_csr* const* ops, int n, void* c_indptr, int64_t* nnz_out, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
  if (check_sum(ops, n)) return -1;
  if (!c_indptr || !nnz_out) return fail("csr_sum: c_indptr / nnz_out is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, c_indptr);
  const int64_t rows = ops[0]->num_rows;
  const Layout l = layout_for(rows, n, ops[0]->idtype_bits);
  Scratch ws(s);
  if (ws.take(workspace, workspace_bytes, l.bytes)) return -1;
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || ops[k]->nnz > 0;
  return with_idx(ops[0]->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    std::vector<Operand<Idx>> host;
    if (upload_ops<Idx>(ops, nullptr, n, &host, ws.p + l.off_ops, s)) return -1;
    return count_rows<Idx>(SumSrc<Idx, float>{reinterpret_cast<const Operand<Idx>*>(ws.p + l.off_ops), n}, rows, any,
                           c_indptr, nnz_out, ws.p, l, s);
  });
}

int dgla_csr_sum_fill(const dgla_csr* const* ops, int n, dgla_dtype dtype, const void* const* weights, const void* c_indptr,
                      void* c_indices, void* c_w, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (check_sum(ops, n)) return -1;
  if (!c_indptr) return fail("csr_sum: c_indptr is null");
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || ops[k]->nnz > 0;
  const int64_t rows = ops[0]->num_rows;
  if (!any || rows == 0) return 0;
  if (!weights) return fail("csr_sum: the weights are null");
  for (int k = 0; k < n; ++k)
    if (ops[k]->nnz > 0 && !weights[k]) return fail("csr_sum: the weights of an operand are null");
  if (!c_indices || !c_w) return fail("csr_sum: c_indices / c_w is null");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, c_indptr);
  const Layout l = layout_for(rows, n, ops[0]->idtype_bits);
  Scratch ws(s);
  if (ws.take(workspace, workspace_bytes, l.bytes)) return -1;
  return with_idx(ops[0]->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    std::vector<Operand<Idx>> host;
    if (upload_ops<Idx>(ops, weights, n, &host, ws.p + l.off_ops, s)) return -1;
    return sum_fill<Idx>(reinterpret_cast<const Operand<Idx>*>(ws.p + l.off_ops), n, rows, dtype, c_indptr, c_indices, c_w,
                         ws.p, l, s);
  });
}

int dgla_csr_mask(const dgla_csr* a, dgla_dtype dtype, const void* a_w, const dgla_coo* b, void* out, void* hip_stream) {
  if (check_operand("csr_mask: a", a)) return -1;
  if (!b) return fail("csr_mask: b is null");
  if (b->idtype_bits != a->idtype_bits) return fail("csr_mask: the operands have different id types");
  if (b->num_rows != a->num_rows || b->num_cols != a->num_cols) return fail("csr_mask: the operands have different shapes");
  if (b->nnz < 0) return fail("csr_mask: negative size");
  if (b->nnz == 0) return 0;
  if (!b->row || !b->col) return fail("csr_mask: the coo arrays of b are null");
  if (!out) return fail("csr_mask: out is null");
  if (a->nnz > 0 && !a_w) return fail("csr_mask: the weights of a are null");
  if (static_cast<unsigned>(dtype) > DGLA_BF16) return fail("csr_mask: unknown dtype");
  if (b->nnz > (int64_t(0xffffffffLL) * 256) / kMaskGroup) return fail("csr_mask: too many queries for one launch");
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, out);
  return with_idx(a->idtype_bits, [&](auto tag) { return mask_dispatch<decltype(tag)>(a, dtype, a_w, b, out, s); });
}

}  // extern "C"
