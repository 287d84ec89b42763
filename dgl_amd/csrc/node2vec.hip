// node2vec walks on the device: a bounded second-order step (dgl.sampling.node2vec_random_walk).
//
// Reference: Node2vecRandomWalkStep (src/graph/sampling/randomwalks/node2vec_randomwalk.h:67-147, CPU only; there is no
// GPU form): an UNBOUNDED rejection loop around RandInt / Choice, the class of a candidate from has_edge_between
// (a binary search when the CSR is sorted, else a linear find).  With p = 1000 one walk can spin for thousands of
// draws, which one lane of a wavefront must not do.
//
// MI355X-first choices:
//  * The step is the rule of csrc/node2vec_step.h, compiled here for the kernel and for dgla_node2vec_walk_host: at
//    most K = min(max(deg, 8), 1024) rejection attempts, then an exact scan of the row with the same law.  The picks are a
//    pure function of (rng_seed, walk index, step, draw slot).
//  * "does x -> prev exist" is a bisection in a membership list: every row's column ids in ascending order, built once
//    per relation by two runs of the library's own stable COO -> CSR sort (dgla_csr_sorted_columns) — no vendor sort, no
//    host pass, multigraphs and self-loops included.
//  * One lane per walk, no LDS, no atomics.  p and q arrive as three acceptance probabilities computed by the host (the
//    kernel divides nothing); the graph arrays are reached through pointers that name the global address space; an
//    attempt whose acceptance draw decides without the class reads neither the candidate's row nor the membership list;
//    the accepted candidate's indptr pair is kept as the next step's row.
#include "../../include/dgl_amd.h"

#include <string>
#include <type_traits>

#include "host_util.h"
#include "node2vec_step.h"

namespace dgla {
namespace {

// ---- the walk ---------------------------------------------------------------------------------
// WEIGHTED is a compile-time switch (N2vUniform in csrc/node2vec_step.h says why a run-time test of `cdf` will not do).
template <typename Idx, bool WEIGHTED>
__global__ __launch_bounds__(256) void node2vec_walk_kernel(const Idx* __restrict__ indptr, const Idx* __restrict__ indices,
                                                            const Idx* __restrict__ data, const Idx* __restrict__ member,
                                                            const double* __restrict__ cdf, int64_t num_rows,
                                                            const N2vAccept a, int64_t num_steps,
                                                            const Idx* __restrict__ seeds, int64_t num_seeds,
                                                            uint64_t rng_seed, Idx* __restrict__ traces,
                                                            Idx* __restrict__ eids) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (i >= num_seeds) return;
  // 64-bit offsets: num_seeds * (num_steps + 1) may pass 2^31
  Idx* tr = traces + i * (num_steps + 1);
  Idx* ev = eids ? eids + i * num_steps : nullptr;
  if (WEIGHTED)
    n2v_walk<Idx>((gptr<Idx>)indptr, (gptr<Idx>)indices, (gptr<Idx>)data, (gptr<Idx>)member,
                  N2vWeighted<gptr<double>>{(gptr<double>)cdf}, num_rows, a, num_steps, rng_seed, i, seeds[i], tr, ev,
                  nullptr);
  else
    n2v_walk<Idx>((gptr<Idx>)indptr, (gptr<Idx>)indices, (gptr<Idx>)data, (gptr<Idx>)member, N2vUniform{}, num_rows, a,
                  num_steps, rng_seed, i, seeds[i], tr, ev, nullptr);
}

// ---- the membership list ------------------------------------------------------------------------
// out[pos] = the row that holds CSR position pos: the last r with indptr[r] <= pos (empty rows are stepped over)
template <typename Idx>
__global__ __launch_bounds__(256) void expand_rows_kernel(const Idx* __restrict__ indptr, int64_t num_rows, int64_t nnz,
                                                          Idx* __restrict__ out) {
  const int64_t pos = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
  if (pos >= nnz) return;
  int64_t a = 0, b = num_rows;  // first r in [0, num_rows] with indptr[r] > pos; indptr[num_rows] = nnz > pos
  while (a < b) {
    const int64_t m = a + ((b - a) >> 1);
    if (static_cast<int64_t>(indptr[m]) > pos) b = m; else a = m + 1;
  }
  out[pos] = static_cast<Idx>(a - 1);
}

struct SortedLayout {  // offsets into the workspace of dgla_csr_sorted_columns
  size_t rows, t_indices, junk, cols, t_indptr, indptr2, sort, bytes;
};

SortedLayout sorted_layout(const dgla_csr* c) {
  const size_t w = c->idtype_bits == 32 ? 4 : 8, e = w * static_cast<size_t>(c->nnz);
  const size_t s1 = dgla_coo_to_csr_workspace_bytes(c->idtype_bits, c->num_cols, c->nnz),
               s2 = dgla_coo_to_csr_workspace_bytes(c->idtype_bits, c->num_rows, c->nnz);
  Carver cv;
  SortedLayout L;
  L.rows = cv.take(e);
  L.t_indices = cv.take(e);
  L.junk = cv.take(e);
  L.cols = cv.take(e);
  L.t_indptr = cv.take(w * static_cast<size_t>(c->num_cols + 1));
  L.indptr2 = cv.take(w * static_cast<size_t>(c->num_rows + 1));
  L.sort = cv.take(s1 > s2 ? s1 : s2);
  L.bytes = cv.bytes();
  return L;
}

template <typename Idx>
int run_sorted(const dgla_csr* c, void* member, char* ws, const SortedLayout& L, hipStream_t s) {
  const int bits = c->idtype_bits;
  Idx* rows = reinterpret_cast<Idx*>(ws + L.rows);
  Idx* cols = reinterpret_cast<Idx*>(ws + L.cols);
  Idx* t_indptr = reinterpret_cast<Idx*>(ws + L.t_indptr);
  const size_t sort_bytes = L.bytes - L.sort;
  // 1. the edges in CSC order: a stable sort by column id keeps the rows of a column in CSR order
  hipLaunchKernelGGL(expand_rows_kernel<Idx>, dim3(grid1(c->nnz)), dim3(256), 0, s, TypedCsr<Idx>(c).indptr, c->num_rows,
                     c->nnz, rows);
  DGLA_CHECK_HIP(hipGetLastError());
  if (dgla_coo_to_csr_bounded(bits, c->num_cols, c->num_rows, c->nnz, c->indices, rows, nullptr, t_indptr,
                              ws + L.t_indices, ws + L.junk, ws + L.sort, sort_bytes, s))
    return -1;
  // 2. ... and back by row: stable again, so every row receives its column ids in ascending order
  hipLaunchKernelGGL(expand_rows_kernel<Idx>, dim3(grid1(c->nnz)), dim3(256), 0, s, t_indptr, c->num_cols, c->nnz, cols);
  DGLA_CHECK_HIP(hipGetLastError());
  return dgla_coo_to_csr_bounded(bits, c->num_rows, c->num_cols, c->nnz, ws + L.t_indices, cols, nullptr, ws + L.indptr2,
                                 member, ws + L.junk, ws + L.sort, sort_bytes, s);
}

// ---- host side --------------------------------------------------------------------------------
// everything both walk entry points refuse
int check_n2v(const char* who, const dgla_csr* csr, const void* member, const void* seeds, int64_t num_seeds,
              int64_t num_steps, double p, double q, const void* traces, N2vAccept* a) {
  if (check_csr(who, csr)) return -1;
  if (csr->num_rows != csr->num_cols)
    return fail(who, "the relation must join one node set to itself (num_rows " + std::to_string(csr->num_rows) +
                         " != num_cols " + std::to_string(csr->num_cols) + ")");
  if (csr->nnz > 0 && !member) return fail(who, "member is null");
  if (num_steps < 0 || num_seeds < 0) return fail(who, "negative number of steps / seeds");
  if (num_seeds > 0 && (!seeds || !traces)) return fail(who, "seeds / traces are null");
  if (!n2v_accept(p, q, a))
    return fail(who, "p and q must be finite and > 0 with usable acceptance probabilities (p = " + std::to_string(p) +
                         ", q = " + std::to_string(q) + ")");
  return 0;
}

template <typename Idx>
void n2v_host(const TypedCsr<Idx>& c, const double* cdf, const void* member, const void* seeds, int64_t num_seeds,
              int64_t num_steps, const N2vAccept& a, uint64_t rng_seed, void* traces, void* eids, int64_t* stats) {
  const Idx* sd = static_cast<const Idx*>(seeds);
  Idx* tr = static_cast<Idx*>(traces);
  Idx* ev = static_cast<Idx*>(eids);
  const Idx* mem = static_cast<const Idx*>(member);
  for (int64_t i = 0; i < num_seeds; ++i) {  // the two instantiations of the kernel
    if (cdf)
      n2v_walk<Idx>(c.indptr, c.indices, c.data, mem, N2vWeighted<const double*>{cdf}, c.num_rows, a, num_steps, rng_seed, i, sd[i],
                    tr + i * (num_steps + 1), ev ? ev + i * num_steps : nullptr, stats);
    else
      n2v_walk<Idx>(c.indptr, c.indices, c.data, mem, N2vUniform{}, c.num_rows, a, num_steps, rng_seed, i, sd[i],
                    tr + i * (num_steps + 1), ev ? ev + i * num_steps : nullptr, stats);
  }
}

}  // namespace
}  // namespace dgla

using namespace dgla;

extern "C" {

size_t dgla_csr_sorted_columns_workspace_bytes(const dgla_csr* csr) {
  if (!csr || !idbits_ok(csr->idtype_bits) || csr->nnz <= 0 || csr->num_rows <= 0 ||
      csr->num_cols <= 0)
    return 0;
  return sorted_layout(csr).bytes;
}

int dgla_csr_sorted_columns(const dgla_csr* csr, void* member, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "csr_sorted_columns";
  if (check_csr(who, csr, kCsrCols)) return -1;
  if (csr->nnz == 0) return 0;
  if (csr->num_rows == 0 || csr->num_cols == 0) return fail(who, "edges without rows / columns");
  if (!member) return fail(who, "member is null");
  const SortedLayout L = sorted_layout(csr);
  if (need_workspace(who, workspace, workspace_bytes, L.bytes)) return -1;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, member);
  char* ws = static_cast<char*>(workspace);
  return with_idx(csr->idtype_bits, [&](auto tag) { return run_sorted<decltype(tag)>(csr, member, ws, L, s); });
}

int dgla_node2vec_walk(const dgla_csr* csr, const double* cdf, const void* member, const void* seeds, int64_t num_seeds,
                       int64_t num_steps, double p, double q, uint64_t rng_seed, void* traces, void* eids,
                       void* hip_stream) {
  N2vAccept a;
  if (check_n2v("node2vec_walk", csr, member, seeds, num_seeds, num_steps, p, q, traces, &a)) return -1;
  if (num_seeds == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const DeviceGuard dev(s, traces);
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    const TypedCsr<Idx> g(csr);
    auto launch = [&](auto weighted) {
      hipLaunchKernelGGL((node2vec_walk_kernel<Idx, decltype(weighted)::value>), dim3(grid1(num_seeds)), dim3(256), 0, s,
                         g.indptr, g.indices, g.data, static_cast<const Idx*>(member), cdf, g.num_rows, a, num_steps,
                         static_cast<const Idx*>(seeds), num_seeds, rng_seed, static_cast<Idx*>(traces),
                         static_cast<Idx*>(eids));
    };
    if (cdf) launch(std::true_type{}); else launch(std::false_type{});
  });
  DGLA_CHECK_HIP(hipGetLastError());
  return 0;
}

int dgla_node2vec_walk_host(const dgla_csr* csr, const double* cdf, const void* member, const void* seeds,
                            int64_t num_seeds, int64_t num_steps, double p, double q, uint64_t rng_seed, void* traces,
                            void* eids, int64_t* stats) {
  N2vAccept a;
  if (check_n2v("node2vec_walk_host", csr, member, seeds, num_seeds, num_steps, p, q, traces, &a)) return -1;
  int64_t local[3] = {0, 0, 0};
  with_idx(csr->idtype_bits, [&](auto tag) {
    using Idx = decltype(tag);
    n2v_host<Idx>(TypedCsr<Idx>(csr), cdf, member, seeds, num_seeds, num_steps, a, rng_seed, traces, eids,
                  stats ? local : nullptr);
  });
  if (stats) stats[0] = local[0], stats[1] = local[1], stats[2] = local[2];
  return 0;
}

}  // extern "C"
