/*
 * dgl_amd.h — C ABI of the MI355X-native g-SpMM / g-SDDMM hot path (libdgl_amd.so).
 *
 * Two layers are exported:
 *
 *  (1) the GRAPH-FREE SEAM `dgla_*` — plain pointers and sizes.  It replaces the
 *      reference's aten::CSRSpMM / COOSpMM / CSRSDDMM / COOSDDMM
 *      (src/array/array.cc:1148-1233, declared include/dgl/aten/csr.h:1046-1066 and
 *      include/dgl/aten/coo.h:842-867), i.e. the template seam
 *      SpMMCsr<XPU,IdType,DType> / SDDMMCsr / SDDMMCoo of src/array/kernel_decl.h:23-87
 *      with XPU = the ROCm device.  This is what a libdgl build would link against.
 *
 *  (2) the REGISTRY LAYER `DGL*` — the PackedFunc-style FFI that python/dgl/_ffi binds
 *      (include/dgl/runtime/c_runtime_api.h:205-212,336-338,437-445): functions are found
 *      by name ("sparse._CAPI_DGLKernelSpMM", ...) and called with (DGLValue*, type codes).
 *      See the second half of this header.
 *
 * All device pointers are HIP device pointers on the current device; every call is
 * asynchronous on the given stream (reference: kernels run on the current PyTorch stream,
 * src/runtime/cuda/cuda_device_api.cc:362-367).  Functions return 0 on success and -1 on
 * error with the message available from dgla_last_error() / DGLGetLastError()
 * (reference convention: src/runtime/runtime_base.h:14-45).
 */
#ifndef DGL_AMD_H_
#define DGL_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGLA_ABI_VERSION 2

/* Feature element types (DGLDataType {code,bits}: float32/64, float16, bfloat16 —
 * ATEN_FLOAT_TYPE_SWITCH_16BITS, include/dgl/aten/macro.h:137-166). */
typedef enum { DGLA_F32 = 0, DGLA_F64 = 1, DGLA_F16 = 2, DGLA_BF16 = 3 } dgla_dtype;

/* Flags of dgla_spmm_csr. */
#define DGLA_ACCUMULATE 1u /* out += result: the reference's contract, `out` pre-zeroed by the
                              caller (src/array/cuda/spmm.cuh:528-534, _sparse_ops.py:227).
                              Without it rows are written, not accumulated (no memset, no
                              read of `out`).  Only meaningful for reduce == "sum". */
#define DGLA_PLAN_VALID 2u /* `workspace` still holds the merge plan built by an earlier
                              call on the SAME csr (indptr contents, num_rows, nnz). */
#define DGLA_MEAN 4u       /* reduce == "sum" only: every output row is divided by
                              max(in-degree, 1) before it is stored — the `mean` reducer of
                              dgl.ops.gspmm (python/dgl/ops/spmm.py:109-114: sum, then
                              / clamp(in_degrees, 1)) without the second pass over `out`;
                              same two roundings as the reference's sum-then-divide. */
#define DGLA_SPLIT_KEEP 16u /* the caller promises to hand the SAME, unchanged ufeat to later calls
                              on this csr + workspace (static input features, e.g. layer 0 of
                              full-graph training or inference): the split-row copy
                              (DGLA_TUNE_SPLIT) is made whatever the locality probe says — its
                              cost is paid once — and later calls pass DGLA_SPLIT_VALID. */
#define DGLA_SPLIT_VALID 8u /* `workspace` still holds the split-row copy an earlier call (with
                              DGLA_SPLIT_KEEP) made of THIS ufeat, whose contents have not
                              changed since: the re-layout copy is skipped.  Needs
                              DGLA_PLAN_VALID.  Never set it for a tensor you do not own. */
#define DGLA_ESM_OUT_POSITION 128u /* dgla_edge_softmax_forward: see there */
#define DGLA_ESM_B_IS_GRAD 256u    /* dgla_edge_softmax_backward: see there */
#define DGLA_PREPARE_ONLY 32u /* (with DGLA_SPLIT_KEEP) build the merge plan if needed and make the side copy of
                              ufeat's ragged row ends — nothing else: no output is written.  For the PRODUCER of
                              ufeat (the previous layer's epilogue, a feature loader): it prepares the operand on
                              its own stream when it finishes the tensor, and the g-SpMM that consumes it passes
                              DGLA_SPLIT_VALID and launches the merge kernel alone (0.10 ms of the headline
                              step moved out of the consumer's critical path). */

/* CSRMatrix (include/dgl/aten/csr.h:40-49).  For SpMM the rows are DESTINATION nodes
 * (the in-edge CSR / "CSC", src/array/kernel.cc:20-44); for SDDMM rows are SOURCE nodes. */
typedef struct {
  int64_t num_rows, num_cols, nnz;
  int32_t idtype_bits;  /* 32 or 64: element type of indptr / indices / data */
  const void* indptr;   /* [num_rows + 1] */
  const void* indices;  /* [nnz] column ids */
  const void* data;     /* [nnz] edge-id map, or NULL: edge id == position */
} dgla_csr;

/* COOMatrix (include/dgl/aten/coo.h): row = source ids, col = destination ids. */
typedef struct {
  int64_t num_rows, num_cols, nnz;
  int32_t idtype_bits;
  const void* row;
  const void* col;
  const void* data;
} dgla_coo;

/* Dense, contiguous, row-major feature tensor.  shape[0] is the number of nodes / edges,
 * ndim >= 2 (src/array/check.h:46-50).  data == NULL means "operand absent" (the
 * reference passes an empty int64 NDArray, python/dgl/ndarray.py:309-312). */
typedef struct {
  void* data;
  int32_t ndim;
  const int64_t* shape;
} dgla_tensor;

const char* dgla_last_error(void);
int dgla_abi_version(void);

/*
 * g-SpMM on CSR:  out[r, k] = reduce_{j in row r} op(ufeat[indices[j], lhs_off(k)],
 *                                                  efeat[eid(j), rhs_off(k)])
 * Replaces aten::CSRSpMM (src/array/array.cc:1148-1168) -> SpMMCsr<kDGLCUDA,...>
 * (src/array/cuda/spmm.cu:26-106).
 *   op      "add" | "sub" | "mul" | "div" | "copy_lhs" | "copy_rhs"
 *   reduce  "sum" | "max" | "min"
 *   arg_u / arg_e   [same shape as out], element type = idtype; written for max/min only
 *                   (arg_u iff op uses lhs, arg_e iff op uses rhs); may be NULL for sum.
 *   workspace       device scratch of at least dgla_spmm_csr_workspace_bytes() bytes.
 */
int dgla_spmm_csr(const char* op, const char* reduce, const dgla_csr* csr, dgla_dtype dtype,
                  const dgla_tensor* ufeat, const dgla_tensor* efeat, const dgla_tensor* out,
                  void* arg_u, void* arg_e, void* workspace, size_t workspace_bytes,
                  uint32_t flags, void* hip_stream);

size_t dgla_spmm_csr_workspace_bytes(const char* op, const char* reduce, const dgla_csr* csr,
                                     dgla_dtype dtype, const dgla_tensor* ufeat,
                                     const dgla_tensor* efeat, const dgla_tensor* out);

/*
 * Multi-relation g-SpMM with reduce = sum in ONE launch.  Replaces the per-relation loop of
 * SpMMCsrHetero<kDGLCUDA,...> (src/array/cuda/spmm_hetero.cu:26-200), which launches one
 * accumulating kernel per edge type and so re-reads and re-writes the destination buffer
 * once per relation.
 *   csr         row-wise concatenation ("stack") of the in-edge CSRs of all relations that
 *               share the destination node type: row r lists relation 0's edges into r, then
 *               relation 1's, ...; `data` maps a stacked position to the relation-local edge id.
 *   rel         uint8 [nnz]: relation index of every stacked edge, in [0, num_rel)
 *   ufeat0 / efeat0   relation 0's operands (feature shapes are taken from them; all
 *               relations must agree, src/array/kernel.cc:194-199)
 *   ufeat_ptrs / efeat_ptrs   DEVICE arrays of num_rel device pointers: each relation's
 *               source-node / edge feature tensor (NULL when the operator does not use it)
 *   op          "copy_lhs" | "copy_rhs" | "mul"
 * Workspace as for dgla_spmm_csr (same byte count for the stacked csr).
 */
size_t dgla_spmm_csr_stacked_workspace_bytes(const char* op, const dgla_csr* csr,
                                             dgla_dtype dtype, const dgla_tensor* ufeat0,
                                             const dgla_tensor* efeat0, const dgla_tensor* out);
int dgla_spmm_csr_stacked(const char* op, const dgla_csr* csr, const void* rel, int num_rel,
                          dgla_dtype dtype, const dgla_tensor* ufeat0, const dgla_tensor* efeat0,
                          const void* const* ufeat_ptrs, const void* const* efeat_ptrs,
                          const dgla_tensor* out, void* workspace, size_t workspace_bytes,
                          uint32_t flags, void* hip_stream);

/*
 * Multi-relation g-SpMM with reduce = max / min in ONE launch, with the node / edge type trackers
 * of SpMMCsrHetero's compare path (src/array/cuda/spmm_hetero.cu:87-117,160-188 ->
 * SpMMCmpCsrHeteroKernel, spmm.cuh:552-606: a running compare relation by relation, an earlier
 * relation keeps a tie).  `csr`, `rel`, the operand tables and `op` as for dgla_spmm_csr_stacked.
 *   src_ntype / etype   HOST arrays [num_rel]: source node type / edge type of every stacked relation
 *   arg_u, arg_u_ntype  [num_rows, out_len] ids: winning source node and its node type
 *                       (required when the operator reads ufeat, else NULL)
 *   arg_e, arg_e_etype  [num_rows, out_len] ids: winning relation-local edge id and its edge type
 *                       (required when the operator reads efeat, else NULL)
 * An output element no edge reaches holds the reducer's identity, args 0 and trackers -1.
 */
size_t dgla_spmm_csr_stacked_cmp_workspace_bytes(const char* op, const char* reduce, const dgla_csr* csr,
                                                 dgla_dtype dtype, const dgla_tensor* ufeat0,
                                                 const dgla_tensor* efeat0, const dgla_tensor* out);
int dgla_spmm_csr_stacked_cmp(const char* op, const char* reduce, const dgla_csr* csr, const void* rel,
                              int num_rel, const int32_t* src_ntype, const int32_t* etype,
                              dgla_dtype dtype, const dgla_tensor* ufeat0, const dgla_tensor* efeat0,
                              const void* const* ufeat_ptrs, const void* const* efeat_ptrs,
                              const dgla_tensor* out, void* arg_u, void* arg_e, void* arg_u_ntype,
                              void* arg_e_etype, void* workspace, size_t workspace_bytes,
                              uint32_t flags, void* hip_stream);

/*
 * g-SpMM on COO (edge-parallel with device atomics).  Replaces aten::COOSpMM
 * (array.cc:1170-1190) -> SpMMCoo<kDGLCUDA,...> (spmm.cu:80-106, spmm.cuh:624-682).
 * `out` (and arg_*) are fully written by the call.  fp16 / bf16 are refused like the
 * reference does (spmm.cuh:633-641).
 */
int dgla_spmm_coo(const char* op, const char* reduce, const dgla_coo* coo, dgla_dtype dtype,
                  const dgla_tensor* ufeat, const dgla_tensor* efeat, const dgla_tensor* out,
                  void* arg_u, void* arg_e, void* hip_stream);

/*
 * g-SDDMM:  out[eid, k] = op(lhs[sel(lhs_target), lhs_off(k)], rhs[sel(rhs_target), rhs_off(k)])
 * Replaces aten::COOSDDMM / CSRSDDMM (array.cc:1192-1233) -> SDDMMCoo / SDDMMCsr
 * (src/array/cuda/sddmm.cu:17-42, sddmm.hip.h:97-362).
 *   op       "add" | "sub" | "mul" | "div" | "copy_lhs" | "copy_rhs" | "dot"
 *   targets  0 = u (source node), 1 = e (edge), 2 = v (destination node)
 */
int dgla_sddmm_coo(const char* op, const dgla_coo* coo, dgla_dtype dtype,
                   const dgla_tensor* lhs, const dgla_tensor* rhs, const dgla_tensor* out,
                   int lhs_target, int rhs_target, void* hip_stream);

int dgla_sddmm_csr(const char* op, const dgla_csr* csr, dgla_dtype dtype,
                   const dgla_tensor* lhs, const dgla_tensor* rhs, const dgla_tensor* out,
                   int lhs_target, int rhs_target, void* hip_stream);

/*
 * Fused edge softmax over the in-edge CSR (rows = destination nodes), forward and
 * backward.  The reference only has these on CPU (src/array/cpu/spmm.h:484-570, FFI
 * src/array/kernel.cc:542-561; GPU is a TODO at kernel.cc:313,331 and runs 5 kernels,
 * python/dgl/backend/pytorch/sparse.py:709-713).
 *   score / out / grad tensors: [nnz, ...] indexed by edge id.
 *   workspace  optional device scratch of dgla_edge_softmax_workspace_bytes() bytes: with it
 *              (and a feature length <= 16) the degree-balanced merge-path kernels run and
 *              hub rows cost no more than any other 256 edges; without it (NULL / 0) a
 *              row-per-lane-group kernel needing no scratch is used.  DGLA_PLAN_VALID in
 *              `flags`: the workspace still holds the plan of an earlier call on this csr.
 *   DGLA_ESM_OUT_POSITION (merge-path kernels only).  Forward: `score` is read by edge id through the CSR's map as
 *              ever, `out` is written in the CSR's POSITION order — a softmax kept in position order costs one
 *              scattered 32-byte READ per edge instead of a scattered read and a scattered WRITE.  Backward: `out`
 *              (that position-ordered softmax) is read and `back` written by position, `sds` (the caller's gradient)
 *              is read by edge id through the map.  The Python side keeps the position-ordered tensors to itself and
 *              hands out edge-id order through one gather by the inverse map (dgl_amd/autograd.py EdgeSoftmax).
 *   DGLA_ESM_B_IS_GRAD (backward, merge-path kernels only): `sds` holds the upstream gradient g itself; the product
 *              out * g of python/dgl/backend/pytorch/sparse.py:709-713 is formed inside the kernel (rounded to the
 *              storage type as the separate elementwise kernel leaves it: same bits, 6 bytes per element less traffic).
 */
size_t dgla_edge_softmax_workspace_bytes(const dgla_csr* csr, dgla_dtype dtype, int64_t dim);
int dgla_edge_softmax_forward(const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* score,
                              const dgla_tensor* out, void* workspace, size_t workspace_bytes,
                              uint32_t flags, void* hip_stream);
int dgla_edge_softmax_backward(const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* out,
                               const dgla_tensor* sds, const dgla_tensor* back, void* workspace,
                               size_t workspace_bytes, uint32_t flags, void* hip_stream);

/*
 * GAT attention block as ONE operator (csrc/gat_attention.hip):
 *     out[v, h, :] = sum_{u -> v} softmax_v( leaky_relu(el[u, h] + er[v, h]) ) * ft[u, h, :]
 * i.e. the sequence u_add_v -> leaky_relu -> edge_softmax -> u_mul_e_sum of the reference's GATConv
 * (python/dgl/nn/pytorch/conv/gatconv.py:330-347; the softmax alone is five launches on the reference's GPU path,
 * python/dgl/backend/pytorch/sparse.py:709-713, with a fused version left as a TODO at src/array/kernel.cc:313,331)
 * in one pass over the in-edges: no (E, H) tensor is written or read, so an edge-id map costs nothing.
 *   csc        in-edge CSR (rows = destination nodes); its `data` (edge-id map) is not read
 *   ft         (N_src, H, D);  el (N_src, H, 1);  er (N_dst, H, 1);  out (N_dst, H, D): all of element type `dtype`
 *   mz         float [N_dst, H, 2] WHATEVER `dtype` is: the row's softmax maximum and normaliser, written by the forward
 *              and read by the backward, which recomputes the attention weights from them
 * Accepted set (dgla_gat_attention_supported; anything else returns -1 and callers compose the four operators): with
 * s = sizeof(element) (4 for DGLA_F32, 2 for DGLA_F16 / DGLA_BF16; DGLA_F64 is not taken),
 *     V   = min(16 / s, largest power of two that divides D)      elements a lane owns (one aligned load of V * s bytes)
 *     LPH = next_pow2(ceil(D / V))                                lanes per head, idle ones included
 * the call is taken iff H >= 1, D >= 1 and H * LPH <= 64 (a row fits one wavefront).  For fp32 with D a power of two >= 4
 * that is H * D <= 256; fp32 also takes e.g. D = 1..7, 12, 24, 40, 48, 96, D = 47 with H = 1, D = 100 with H <= 2; 16-bit
 * operands take H * D up to 512 for D a multiple of 8 (H8 D64, H2 D256).
 * 16-bit contract: every fp16 / bf16 value is widened on load; the running maximum, the normaliser, the accumulators, the
 * partial states of rows that cross chunks, `mz` and the backward's per-node record are fp32; the ONLY roundings to 16
 * bits are the final stores of out, d_ft, d_el and d_er (one round-to-nearest-even each).  The backward does not read
 * `out`'s values for 16-bit operands (it forms <dout, out> itself, in fp32).  fp32 calls with D a power of two >= 4 run
 * the same kernels, bit for bit, as before the set was widened.
 *   workspace  dgla_gat_attention_workspace_bytes(csc, H, D) bytes of device scratch (required when nnz > 0)
 * Backward: `csr` is the out-edge CSR (rows = source nodes) of the same graph; d_ft / d_el / d_er get the gradients
 * of ft / el / er for the upstream gradient `dout` (every row is written, rows without edges with zeros).
 * Rows without in-edges: out = 0.  Deterministic: no atomics, partial rows are merged in a fixed order.
 */
/* 1 when the fused operator takes (dtype, heads, dim) — the rule above —, 0 otherwise.  Host-only: needs no GPU. */
int dgla_gat_attention_supported(dgla_dtype dtype, int64_t heads, int64_t dim);
size_t dgla_gat_attention_workspace_bytes(const dgla_csr* csc, int64_t heads, int64_t dim);
int dgla_gat_attention_forward(const dgla_csr* csc, dgla_dtype dtype, const dgla_tensor* ft, const dgla_tensor* el,
                               const dgla_tensor* er, float negative_slope, const dgla_tensor* out, void* mz,
                               void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_gat_attention_backward(const dgla_csr* csc, const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* ft,
                                const dgla_tensor* el, const dgla_tensor* er, const dgla_tensor* out, const void* mz,
                                const dgla_tensor* dout, float negative_slope, const dgla_tensor* d_ft,
                                const dgla_tensor* d_el, const dgla_tensor* d_er, void* workspace,
                                size_t workspace_bytes, void* hip_stream);

/*
 * Training form of the block above (csrc/gat_attention_train.hip): dropout on the attention weights, as GATConv's
 *     a = attn_drop(edge_softmax(graph, e));   out[v, h, :] = sum_{u -> v} a_e,h * ft[u, h, :]
 * (python/dgl/nn/pytorch/conv/gatconv.py:337-347), and the weights themselves on request.  No mask is stored:
 * Keep rule (csrc/gat_dropout.h, gat_keep — ONE definition, compiled for the host and the device):
 *     w    = Philox4x32-10(key = the 64-bit seed, counter = (eid low 32, eid high 32, head / 4, 0))[head % 4]
 *     keep = (w >> 8) >= threshold,   threshold = (uint32_t)(p * 16777216.0),   kept weights are scaled by 1 / (1 - p)
 *   threshold and the fp32 scale are computed once on the host from the float `p`, 0 <= p < 1 (anything else is an
 *   error), and handed to the kernels as they are, so host and device agree bit for bit.
 * Edge-id keying: eid = data ? data[pos] : pos of WHICHEVER CSR a kernel walks (csc in the forward, in pass 1 of the
 *   backward and in dgla_gat_attention_weights, csr in pass 2 of the backward).  An edge therefore gets the same bit in
 *   every pass and the mask does not depend on the sparse format; csc and csr must carry the edge-id maps of ONE graph
 *   (a NULL `data` means edge id == position, as everywhere in this header).
 * mz: exactly the mz of dgla_gat_attention_forward — the maximum and the normaliser of the softmax WITHOUT dropout —
 *   so a row whose edges are all dropped gives out = 0, and the backward and the weights kernel recompute a from it.
 * With c = keep / (1 - p), x_e = <dout_v, ft_u>_h and l'_e = leaky_relu'(el_u + er_v):
 *     d_ft[u] = sum_e a c dout_v,   d_er[v] = S2 - S1 S3,   d_el[u] = sum_e l' a (c x - t_v),
 *     S1 = t_v = sum a c x,  S2 = sum l' a c x,  S3 = sum l' a      (fp32 sums over the in-edges of v)
 * Every accepted shape (dgla_gat_attention_supported, same workspace) runs the V-elements-per-lane scheme of the wide
 * kernels — fp32 with D a power of two too, with V = 4 — with fp32 state and one rounding at the final store.  p = 0
 * evaluates no Philox round.  No atomics; same chunk and fix-up order as above: deterministic for a given seed.
 * dgla_gat_attention_weights writes attn[eid, h] = exp(leaky_relu(el[u, h] + er[v, h]) - m_v,h) / z_v,h * c_e,h for every
 * edge, in EDGE-ID order, rounded once to `dtype`: attn is (E, H, 1) (or (E, H)); it needs mz of a forward on the same
 * operands and no workspace.
 * dgla_gat_dropout_mask_host: keep[i * heads + h] = gat_keep(seed, eids[i], h) as 0 / 1 bytes.  Host-only: needs no GPU.
 */
int dgla_gat_attention_train_forward(const dgla_csr* csc, dgla_dtype dtype, const dgla_tensor* ft, const dgla_tensor* el,
                                     const dgla_tensor* er, float negative_slope, float p, uint64_t seed,
                                     const dgla_tensor* out, void* mz, void* workspace, size_t workspace_bytes,
                                     void* hip_stream);
int dgla_gat_attention_train_backward(const dgla_csr* csc, const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* ft,
                                      const dgla_tensor* el, const dgla_tensor* er, const void* mz, const dgla_tensor* dout,
                                      float negative_slope, float p, uint64_t seed, const dgla_tensor* d_ft,
                                      const dgla_tensor* d_el, const dgla_tensor* d_er, void* workspace,
                                      size_t workspace_bytes, void* hip_stream);
int dgla_gat_attention_weights(const dgla_csr* csc, dgla_dtype dtype, const dgla_tensor* el, const dgla_tensor* er,
                               const void* mz, float negative_slope, float p, uint64_t seed, const dgla_tensor* attn,
                               void* hip_stream);
int dgla_gat_dropout_mask_host(uint64_t seed, float p, const int64_t* eids, int64_t n, int heads, uint8_t* keep);

/* ---- segment reduce / scatter add ----------------------------------------
 * Replace SegmentReduce / ScatterAdd / BackwardSegmentCmp<kDGLCUDA,…>
 * (src/array/kernel_decl.h, kernels src/array/cuda/segment_reduce.cuh:30-113; registered as
 * sparse._CAPI_DGLKernelSegmentReduce / ScatterAdd / BwdSegmentCmp, src/array/kernel.cc:658-708).
 *
 * dgla_segment_reduce: out[i, :] = reduce_{j in [offsets[i], offsets[i+1])} feat[j, :],
 *   reduce in {"sum","max","min"}; offsets has num_segments + 1 entries of idtype_bits;
 *   `arg` (idtype, shape of out; required for max/min) receives the winning row j, or -1 for
 *   an element nothing won (empty segment).  Empty segments give 0 / -inf / +inf like the
 *   reference.  `workspace` may be NULL: scratch is then taken from the stream-ordered HIP
 *   allocator for the duration of the call.
 * dgla_scatter_add: out[idx[i], :] += feat[i, :]   (atomic; out is NOT zeroed)
 * dgla_backward_segment_cmp: out[arg[i, k], k] = feat[i, k] wherever arg[i, k] >= 0
 * dgla_update_grad_minmax: out[idx[i, k], k] += feat[i, k] wherever idx_type[i, k] == type —
 *   one relation's share of the max / min gradient on a heterograph
 *   (UpdateGradMinMax_hetero<kDGLCUDA,…>, src/array/cuda/segment_reduce.cuh:73-92,184-225):
 *   idx = the winning node / edge ids the forward pass recorded, idx_type = the node / edge type
 *   of every winner (-1: nothing won), both [n, dim] of idtype; out is NOT zeroed (atomic).
 * dgla_spmm_cmp_backward: backward of g-SpMM max / min on one relation, ONE pass
 *   (python/dgl/backend/pytorch/sparse.py:217-244 is two .long() casts, a gather and an atomic
 *   scatter_add_): out[arg[i, k], k] (+)= dz[i, k] * (other ? other[arg_other[i, k], (k / other_group) %
 *   row_len(other)] : 1) wherever arg[i, k] >= 0; arg / arg_other = the winners the forward pass recorded
 *   ([n, dim] of idtype_bits).  atomic = 0 for the EDGE operand (an edge has one destination: every
 *   target element is written at most once, plain stores, deterministic), 1 for the NODE operand (a node
 *   can win at many destinations: hardware float atomics, like the reference).  out is NOT zeroed. */
size_t dgla_segment_reduce_workspace_bytes(const char* reduce, int idtype_bits, dgla_dtype dtype,
                                           const dgla_tensor* feat, int64_t num_segments,
                                           const dgla_tensor* out);
int dgla_segment_reduce(const char* reduce, int idtype_bits, dgla_dtype dtype,
                        const dgla_tensor* feat, const void* offsets, int64_t num_segments,
                        const dgla_tensor* out, void* arg, void* workspace,
                        size_t workspace_bytes, uint32_t flags, void* hip_stream);
int dgla_scatter_add(int idtype_bits, dgla_dtype dtype, const dgla_tensor* feat, const void* idx,
                     const dgla_tensor* out, void* hip_stream);
int dgla_update_grad_minmax(int idtype_bits, dgla_dtype dtype, const dgla_tensor* feat,
                            const void* idx, const void* idx_type, int64_t type,
                            const dgla_tensor* out, void* hip_stream);
int dgla_backward_segment_cmp(int idtype_bits, dgla_dtype dtype, const dgla_tensor* feat,
                              const void* arg, const dgla_tensor* out, void* hip_stream);
int dgla_spmm_cmp_backward(int idtype_bits, dgla_dtype dtype, const dgla_tensor* dz, const void* arg,
                           const dgla_tensor* other, const void* arg_other, int64_t other_group,
                           const dgla_tensor* out, int atomic, void* hip_stream);
/* The NODE operand's max / min gradient for copy_lhs / add WITHOUT atomics — the same scatter_add_ of
 * python/dgl/backend/pytorch/sparse.py:216-224 turned into a gather over the reverse graph, so that the result has the
 * same bits on every run:  dX[u, k] = sum over the out-edges e = (u -> v) of [e delivered the winner of (v, k)] dZ[v, k].
 *   dgla_spmm_cmp_mask    `csr` = the FORWARD matrix (rows = destinations); `arg` [num_rows, F] of idtype = arg_u
 *       (by_edge = 0: the first edge of row v whose source is arg_u[v, k] gets bit k) or arg_e (by_edge != 0: the
 *       edge whose id it names).  Writes, for every edge in the CSR's POSITION order, dgla_spmm_cmp_mask_words(dtype, F)
 *       words of the feature type's width (16 / 32 / 64 bits), bit (k mod width) of word k / width = column k.  An
 *       element no edge of its row claims (empty row, or nothing beat the identity: arg = 0) goes to dX[0, k] here,
 *       exactly where the reference's scatter sends it, summed in a fixed order: `dx` must be ZEROED before this call.
 *       Two-step form (round 6, saves the zero fill and the g-SpMM's read of dx): `by_edge | DGLA_CMP_MASK_DEFER` writes
 *       the bits and keeps the sums aside WITHOUT touching dx; dgla_spmm_csr_masked then STORES its rows (no
 *       DGLA_ACCUMULATE, dx may be uninitialised memory); the same call again with `by_edge | DGLA_CMP_MASK_FINISH` adds
 *       what was kept aside (and, only if an unclaimed element named a non-zero target, scans again for those).
 *   dgla_spmm_csr_masked  `csr` = the REVERSE matrix (rows = sources) whose `data` maps each of ITS positions to the
 *       forward position of the same edge (always present); `ufeat` = dZ, `mask` from above, `out` = dX with
 *       DGLA_ACCUMULATE (the atomics above are already in it).  One merge-path launch of the g-SpMM kernel.
 */
#define DGLA_CMP_MASK_DEFER 0x100
#define DGLA_CMP_MASK_FINISH 0x200
int64_t dgla_spmm_cmp_mask_words(dgla_dtype dtype, int64_t feat_len);
/* bytes of `mask`: the words of every edge + the mask pass's own partial sums behind them (no allocation inside the
 * call: it can be captured in a hipGraph) */
size_t dgla_spmm_cmp_mask_bytes(dgla_dtype dtype, int64_t num_rows, int64_t nnz, int64_t feat_len);
int dgla_spmm_cmp_mask(const dgla_csr* csr, dgla_dtype dtype, const void* arg, int by_edge, const dgla_tensor* dz,
                       void* mask, const dgla_tensor* dx, void* hip_stream);
size_t dgla_spmm_csr_masked_workspace_bytes(const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* ufeat,
                                            const dgla_tensor* out);
int dgla_spmm_csr_masked(const dgla_csr* csr, dgla_dtype dtype, const dgla_tensor* ufeat, const void* mask,
                         const dgla_tensor* out, void* workspace, size_t workspace_bytes, uint32_t flags,
                         void* hip_stream);

/* ---- segment / gather matrix multiply --------------------------------------
 * Replace SegmentMM / SegmentMMBackwardB / GatherMM / GatherMMScatter<kDGLCUDA,…>
 * (src/array/cuda/gather_mm.cu:201-360; registered as sparse._CAPI_DGLKernelSEGMENTMM,
 * …SEGMENTMMBackwardB, …GATHERMM, …GATHERMMSCATTER, src/array/kernel.cc:501-540).
 * All matrices row-major and contiguous; `seglen` has num_rel entries of idtype_bits and may
 * live in HOST memory (seglen_on_host = 1, as the reference passes it) or on the device.
 *
 * dgla_segment_mm:  for every relation r with rows [o_r, o_r + seglen[r]) of A:
 *     b_trans == 0:  C[rows] = A[rows] (m x k) . B[r] (k x n),  B is [num_rel, k, n]
 *     b_trans != 0:  C[rows] = A[rows] (m x k) . B[r]^T,        B is [num_rel, n, k]
 *   ONE grouped launch on the MFMA units (fp32 accumulate; fp64 on the vector ALUs).  Rows
 *   beyond sum(seglen) come back ZERO, as the reference's do (its output starts as th.zeros,
 *   python/dgl/backend/pytorch/sparse.py:975).
 * dgla_segment_mm_backward_b:  dB[r] (d1 x d2) = A[rows_r]^T (d1 x m) . dC[rows_r] (m x d2);
 *   relations without rows get zeros.  fp32 default route (round 6): operands as two fp16 terms under per-column
 *   power-of-two scales estimated from a row sample and verified in the launch (>= 2^-21 per element; elements more than
 *   26 binades under their column's sample maximum are added exactly from a short list); inputs that leave the estimated
 *   range, Inf / NaN included, are redone by the three-bf16-term kernel inside the same call.  DGLA_TUNE_MM_X3 /
 *   DGLA_TUNE_MM_F32 select the three-term / v_mfma_f32_32x32x2_f32 routes.
 * dgla_segment_mm_backward_b_last_route: statistics of the most recent fp32 two-term weight-gradient launch on the
 *   current device (synchronising read): whether it was redone by the three-term kernel, and how many elements went
 *   through the exact list.  No reference counterpart (diagnostics for tests / benchmarks).
 * dgla_gather_mm:  C[idx_c ? idx_c[i] : i] = A[idx_a ? idx_a[i] : i] (1 x k) . B[idx_b ? idx_b[i] : i]
 *   (k x n), one wavefront per row (the small-shape path of dgl.ops.gather_mm).
 * `workspace` may be NULL (stream-ordered scratch for the duration of the call). */
size_t dgla_segment_mm_workspace_bytes(dgla_dtype dtype, int64_t num_rel, int64_t d1, int64_t d2);
int dgla_segment_mm(int idtype_bits, dgla_dtype dtype, const void* a, const void* b, void* c,
                    const void* seglen, int seglen_on_host, int64_t num_rows, int64_t num_rel,
                    int64_t k, int64_t n, int b_trans, void* workspace, size_t workspace_bytes,
                    void* hip_stream);
int dgla_segment_mm_backward_b(int idtype_bits, dgla_dtype dtype, const void* a, const void* dc,
                               void* db, const void* seglen, int seglen_on_host,
                               int64_t num_rows, int64_t num_rel, int64_t d1, int64_t d2,
                               void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_segment_mm_backward_b_last_route(uint32_t* fell_back, uint32_t* listed_elements);
/* The same two operators over rows that are NOT stored grouped by relation: logical row r (the
 * order `seglen` describes) lives at physical row row_index[r] of A and of C (forward) / of A and
 * dC (weight gradient).  This is dgl.ops.gather_mm for large inputs without its two
 * index_select copies (python/dgl/ops/gather_mm.py:44-60): sort idx_b once, pass the permutation. */
int dgla_segment_mm_indexed(int idtype_bits, dgla_dtype dtype, const void* a, const void* b, void* c,
                            const void* seglen, int seglen_on_host, const int64_t* row_index,
                            int64_t num_rows, int64_t num_rel, int64_t k, int64_t n, int b_trans,
                            void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_segment_mm_backward_b_indexed(int idtype_bits, dgla_dtype dtype, const void* a, const void* dc,
                                       void* db, const void* seglen, int seglen_on_host,
                                       const int64_t* row_index, int64_t num_rows, int64_t num_rel,
                                       int64_t d1, int64_t d2, void* workspace, size_t workspace_bytes,
                                       void* hip_stream);
int dgla_gather_mm(int idtype_bits, dgla_dtype dtype, const void* a, const void* b, void* c,
                   const void* idx_a, const void* idx_b, const void* idx_c, int64_t num_rows,
                   int64_t k, int64_t n, void* hip_stream);

/* ---- COO -> CSR / CSC materialisation -----------------------------------
 * Replaces aten::COOToCSR<kDGLCUDA> (src/array/cuda/coo2csr.cu:28-110 = COOSort by row +
 * cusparseXcoo2csr), which UnitGraph::GetInCSR / GetOutCSR run on first use
 * (src/graph/unit_graph.cc:1418-1450).  Stable: edges keep their COO order inside a row.
 *   row / col   [nnz] of idtype_bits: the major index (compressed) and the minor one; pass
 *               (dst, src) for the in-edge CSR ("CSC"), (src, dst) for the out-edge CSR
 *   eids        optional [nnz] edge ids of the COO entries (NULL: position)
 *   indptr      out [num_rows + 1];  indices, eids_out: out [nnz] — eids_out[i] is the edge id
 *               of CSR position i (the reference's csr.data)
 * `workspace` may be NULL (stream-ordered scratch for the duration of the call). */
size_t dgla_coo_to_csr_workspace_bytes(int idtype_bits, int64_t num_rows, int64_t nnz);
int dgla_coo_to_csr(int idtype_bits, int64_t num_rows, int64_t nnz, const void* row, const void* col,
                    const void* eids, void* indptr, void* indices, void* eids_out, void* workspace,
                    size_t workspace_bytes, void* hip_stream);
/* The same with the caller's promise that every minor id (`col`) is below num_minor: with int64 ids
 * and num_rows, num_minor, nnz < 2^31 the sort then runs on 32-bit keys with the minor id packed into
 * its 64-bit value, like the int32 form (3.35 -> ~2.1 ms at 62 M edges). */
int dgla_coo_to_csr_bounded(int idtype_bits, int64_t num_rows, int64_t num_minor, int64_t nnz, const void* row,
                            const void* col, const void* eids, void* indptr, void* indices, void* eids_out,
                            void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- sparse x sparse: CSRMM, CSRSum, CSRMask (csrc/csr_mm.hip) ------------------------------
 * Replace aten::CSRMM / CSRSum / CSRGetData<kDGLCUDA> behind _CAPI_DGLCSRMM / _CAPI_DGLCSRSum /
 * _CAPI_DGLCSRMask (src/array/kernel.cc:725-800; CPU kernels src/array/cpu/csr_mm.cc:20-130, csr_sum.cc; GPU kernels
 * src/array/cuda/csr_mm.cu, csr_sum.cu over cusparseSpGEMM / csrgeam2).  Operands are CSR matrices of SIMPLE graphs (no
 * duplicate column in a row, as the reference requires) with optional edge-id maps; weights are one scalar per edge,
 * read as w[data ? data[pos] : pos] (csr_mm.cc:67-70).
 *   C = A . B  (A: M x K, B: K x P)   /   C = A_0 + ... + A_{n-1}  (n >= 1 operands of one shape)
 * Structure of C: the structural product / union — an entry exists wherever at least one term exists, also when the
 * terms cancel to 0.0 ("Unlike scipy", python/dgl/transforms/functional.py:2583); C carries no edge-id map; the columns of a row ascend
 * strictly; the same structure on every run.  Values: fp32 / fp64 in their own arithmetic; fp16 / bf16 are widened on
 * load, multiplied and added in fp32 and rounded once at the store of c_w.  The terms of an entry are added in a fixed
 * order (product: position order of A's row; sum: operand order): no floating-point atomics, same bits on every run.
 * Term counts and nnz(C) are int64 inside; with int32 ids an nnz(C) above 2^31 - 1 is an error, with int64 ids there
 * is no limit of the reference's 2^31 kind.  Zero sizes (M, K, P, nnz(A), nnz(B) == 0) are valid calls.
 * Two calls around one workspace, every output allocated by the caller:
 *   *_count  writes c_indptr [M + 1] and *nnz_out (HOST memory; reading it is the call's one synchronisation);
 *   *_fill   writes c_indices / c_w [nnz(C)] for the c_indptr of a count on the same operands.
 * `workspace` may be NULL (stream-ordered scratch for the duration of the call); the bound is a host computation from the
 * row count alone — no path expands terms into global memory, so there is nothing to chunk.
 * dgla_csr_mm_row_classes: the term-count thresholds between the row classes (one wavefront per row / one workgroup
 * per row / dense accumulator over column windows), ascending; returns their number (2) and writes min(max, 2). */
size_t dgla_csr_mm_workspace_bytes(const dgla_csr* a, const dgla_csr* b);
int dgla_csr_mm_count(const dgla_csr* a, const dgla_csr* b, void* c_indptr, int64_t* nnz_out, void* workspace,
                      size_t workspace_bytes, void* hip_stream);
int dgla_csr_mm_fill(const dgla_csr* a, dgla_dtype dtype, const void* a_w, const dgla_csr* b, const void* b_w,
                     const void* c_indptr, void* c_indices, void* c_w, void* workspace, size_t workspace_bytes,
                     void* hip_stream);
int dgla_csr_mm_row_classes(int64_t* bounds, int max);
/* `ops`: HOST array of n operand descriptors; `weights`: HOST array of n device pointers (dgla_csr_sum_fill). */
size_t dgla_csr_sum_workspace_bytes(const dgla_csr* const* ops, int n);
int dgla_csr_sum_count(const dgla_csr* const* ops, int n, void* c_indptr, int64_t* nnz_out, void* workspace,
                       size_t workspace_bytes, void* hip_stream);
int dgla_csr_sum_fill(const dgla_csr* const* ops, int n, dgla_dtype dtype, const void* const* weights,
                      const void* c_indptr, void* c_indices, void* c_w, void* workspace, size_t workspace_bytes,
                      void* hip_stream);
/* CSRMask (kernel.cc:775-800, CSRGetData with filler 0): out[eid(e)] = A[row_b[e], col_b[e]], or 0 where A has no such
 * entry, for every entry e of the COO `b` (eid(e) = b.data ? b.data[e] : e); a copy, no arithmetic.  One group of 8
 * lanes per query: bisection when the columns of A ascend strictly in every row (checked on the device in the same
 * call), else a strided scan of the row in which the smallest matching position wins.  A or b without entries is valid. */
int dgla_csr_mask(const dgla_csr* a, dgla_dtype dtype, const void* a_w, const dgla_coo* b, void* out, void* hip_stream);

/* ---- uniform neighbour sampling and block construction -------------------
 * Replace CSRRowWiseSamplingUniform<kDGLCUDA> (src/array/cuda/rowwise_sampling.cu:43-330, behind
 * dgl.sampling.sample_neighbors) and ToBlock<kDGLCUDA> (src/graph/transform/cuda/cuda_to_block.cu,
 * behind dgl.to_block) for the uniform, single-relation case of mini-batch GraphSAGE.
 *
 * dgla_sample_neighbors: for every seed (a row of the in-edge CSR `csc`) picks min(deg, fanout)
 *   in-neighbours uniformly without replacement (fanout with replacement when `replace`;
 *   fanout = -1: all).  Output is itself a CSR over the seeds: out_indptr [num_seeds + 1],
 *   out_src (GLOBAL source ids) and out_eids (edge ids) of out_indptr[num_seeds] entries —
 *   allocate num_seeds * fanout (or call once with out_src == NULL to get out_indptr only, for
 *   fanout = -1).  The picks depend only on (rng_seed, seed node): reproducible.
 * dgla_to_block: renumbers `src` (global ids, nnz entries) into block-local ids with the seeds
 *   first in the given order and the remaining nodes by ascending id.  `node_map` is caller-owned
 *   int32 scratch with one entry per node of the graph, all -1 on entry and again on exit;
 *   src_nodes [>= num_seeds + nnz] receives the global id of every local source node,
 *   *num_src_out (device memory) their number. */
 /* dgla_sample_neighbors_weighted: the same with per-edge probabilities `prob` (float32 / float64,
 *   indexed by EDGE ID like every edge feature) — CSRRowWiseSampling<kDGLCUDA> of
 *   src/array/cuda/rowwise_sampling_prob.cu: without replacement the A-Res rule (here in its
 *   exponential-clock form, keys recomputed from a counter-based generator instead of stored and
 *   sorted), with replacement inverse-CDF picks; edges with prob <= 0 are never returned, so a row
 *   yields min(fanout, #positive edges) entries (the reference removes them after sampling).
 *   Call with out_src == NULL first to get out_indptr when the caller does not want to
 *   over-allocate num_seeds * fanout. */
/* The rule of the three calls (tests/neighbor_cases.py restates it in Python; the device is held to that model bit for
 * bit).  mix64, walk_key(seed, i) = mix64(seed ^ (i * 0xD1B54A32D192ED03)), step_key(wk, t) = mix64(wk + t) and
 * index(r, n) = (r * n) >> 64 are those of csrc/random_walk_step.h.
 *
 * Uniform.  Seed row i with node id r = seeds[i], deg in-edges starting at position start, call seed S.
 *   Count: fanout = -1: deg.  With replacement: fanout, or 0 for deg == 0.  Otherwise min(deg, fanout).
 *   Positions: with fanout = -1, or deg <= fanout without replacement: 0 .. deg-1 in order.  With replacement slot k
 *   gets index(step_key(walk_key(S, r), k), deg).  Without replacement the rule is Floyd's: for m = 0 .. fanout-1 let
 *   j = deg - fanout + m and t = index(step_key(walk_key(S, r), m), j + 1); slot m gets t unless an earlier slot holds
 *   t, then it gets j.
 *   The generator is keyed by the NODE ID, not by the position in `seeds`: a node listed twice gets the same picks, and
 *   permuting `seeds` permutes the rows.  The picks do not depend on the launch geometry.
 *   Output: slot k of row i, at out_indptr[i] + k, holds indices[start + pos] and data ? data[start + pos] : start + pos.
 *
 * Weighted.  `prob` is indexed by edge id: the weight at position j of the row is w_j = prob[data ? data[start+j] :
 *   start+j].  A position is positive iff w_j > 0, so NaN, negative weights and +-0 are never positive.
 *   Count: without replacement min(fanout, #positive); with replacement fanout, or 0 with no positive edge.
 *   Without replacement: u_j = ((mix64(walk_key(S, r) + 0x5851F42D4C957F2D * (j+1)) >> 11) + 1) * 2^-53 and
 *   key_j = -ln(u_j) / (double) w_j.  The slots hold the positive positions in ascending (key, j).
 *   With replacement: total is the fp64 sum of the positive weights (the order of the additions is free).  For slot t,
 *   rr = mix64(walk_key(S, r) + 0x2545F4914F6CDD1D * (t+1)) and target = ((double)(rr >> 11) + 0.5) * 2^-53 * total,
 *   evaluated left to right.  The pick is the first positive position whose inclusive prefix of positive weights is
 *   >= target; if rounding leaves none, the last positive position.
 *
 * Block.  src_nodes = seeds in the given order, then the ids of `src` that are not seeds, ascending, each once.
 *   local_src[e] is the index of src[e] in src_nodes, *num_src_out the length of src_nodes, and node_map is all -1
 *   again on return. */
size_t dgla_sample_neighbors_workspace_bytes(int idtype_bits, int64_t num_seeds);
int dgla_sample_neighbors_weighted(const dgla_csr* csc, const void* prob, dgla_dtype prob_dtype,
                                   const void* seeds, int64_t num_seeds, int fanout, int replace,
                                   uint64_t rng_seed, void* out_indptr, void* out_src, void* out_eids,
                                   void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_sample_neighbors(const dgla_csr* csc, const void* seeds, int64_t num_seeds, int fanout,
                          int replace, uint64_t rng_seed, void* out_indptr, void* out_src,
                          void* out_eids, void* workspace, size_t workspace_bytes, void* hip_stream);
size_t dgla_to_block_workspace_bytes(int idtype_bits, int64_t nnz);
int dgla_to_block(int idtype_bits, const void* seeds, int64_t num_seeds, const void* src, int64_t nnz,
                  void* node_map, void* local_src, void* src_nodes, int64_t* num_src_out,
                  void* workspace, size_t workspace_bytes, void* hip_stream);

/* Padded (static-shape) forms of the two calls above: no size ever travels to the host, so a whole
 * mini-batch step — sample, build blocks, gather, g-SpMM, backward, update — can be captured in ONE
 * hipGraph and replayed (the reference synchronises after every sampling layer to size the next
 * allocation: python/dgl/dataloading/neighbor_sampler.py sample_blocks -> cuda_to_block.cu).
 * dgla_sample_neighbors_padded: `seeds` has num_seeds SLOTS of which the first *num_valid (device
 *   memory; NULL = all) are real — the rest are padding (any valid node id) and pick nothing.
 *   fanout > 0.  out_src / out_eids hold cap = num_seeds * fanout entries: the picks in
 *   [0, out_indptr[num_seeds]), then the edges of `sink_rows` extra SINK rows (rows num_seeds ..
 *   num_seeds + sink_rows - 1 in equal shares; out_indptr has num_seeds + 1 + sink_rows entries,
 *   the last = cap) that point at the real seeds in turn.  A consumer sees a well-formed CSR with
 *   num_seeds + sink_rows rows and cap edges whose real rows are exactly the unpadded call's; the
 *   sink rows' results are garbage to be ignored.  The draw counter is
 *   rng_seed + *rng_counter * 0x9E3779B97F4A7C15 (rng_counter: device int64 or NULL), so a
 *   captured launch samples afresh whenever the caller bumps the counter on the device.
 *   `prob` != NULL: weighted picks as dgla_sample_neighbors_weighted (float32 / float64 per EDGE ID).
 *   `workspace` (dgla_sample_neighbors_workspace_bytes) is REQUIRED: the call allocates nothing.
 * dgla_to_block_padded: like dgla_to_block over all cap entries of the padded `src`; only the first
 *   *num_valid seeds claim a local id (padding slots keep their row — the destination nodes of the
 *   block are still its first num_seeds source nodes — but edges never resolve to them); new nodes
 *   get ids from num_seeds upwards; entries of src_nodes past *num_src_out are left untouched
 *   (pre-fill the buffer with a valid node id).  num_nodes > 0 (the graph's node count) lets the
 *   sort look at the used key bits only.  `workspace` (dgla_to_block_workspace_bytes(nnz))
 *   is required. */
int dgla_sample_neighbors_padded(const dgla_csr* csc, const void* prob, dgla_dtype prob_dtype, const void* seeds,
                                 int64_t num_seeds, const int64_t* num_valid, int fanout, int replace,
                                 uint64_t rng_seed, const int64_t* rng_counter, int sink_rows, void* out_indptr,
                                 void* out_src, void* out_eids, void* workspace, size_t workspace_bytes,
                                 void* hip_stream);
int dgla_to_block_padded(int idtype_bits, const void* seeds, int64_t num_seeds, const int64_t* num_valid,
                         const void* src, int64_t nnz, int64_t num_nodes, void* node_map, void* local_src,
                         void* src_nodes, int64_t* num_src_out, void* workspace, size_t workspace_bytes,
                         void* hip_stream);

/* ---- random walks: metapath, weighted and restart forms ------------------------------------------
 * Replace RandomWalk<kDGLCUDA> and its restart forms (src/graph/sampling/randomwalks/randomwalk_gpu.cu, behind
 * dgl.sampling.random_walk, python/dgl/sampling/randomwalks.py:31-226).  The reference seeds one curand state per thread
 * (its picks depend on the launch geometry) and scans a weighted row linearly; here the picks are a pure function of
 * (rng_seed, walk index, step, draw slot) and the weighted step is a bisection in a CDF built once per relation.
 * The step rule (ONE definition for device and host, csrc/random_walk_step.h):
 *
 * Generator.  mix64 is the function of csrc/sampling.hip (the splitmix64 finaliser including its increment).  For walk
 * index i (position in `seeds`, not the node id, so a node listed twice gets two independent walks), step t (0-based)
 * and draw slot k:
 *     r(seed,i,t,k) = mix64( mix64( mix64(seed ^ (i * 0xD1B54A32D192ED03)) + t ) + k )      (all mod 2^64)
 *     uniform index in [0,n):  (r * n) >> 64    (multiply-high)
 *     uniform double in [0,1): (r >> 11) * 2^-53
 * Slot 0 is the neighbour pick and slot 1 is the restart test.
 *
 * One step of walk i at node curr, step t, relation R = rels[metapath[t]].  R is the out-edge CSR: rows are source
 * nodes, `indices` are successors, and `data` is the edge-id map or NULL.
 *  1. Restart: if a restart probability p_t is given (scalar, or restart_steps[t] converted to double) and
 *     u(seed,i,t,1) < p_t, the walk halts.
 *  2. lo = indptr[curr], hi = indptr[curr+1].  If hi == lo, the walk halts.
 *  3. Uniform relation (cdf == NULL): pos = lo + index(r(seed,i,t,0), hi - lo).
 *  4. Weighted relation: total = cdf[hi-1].  If !(total > 0) or total is not finite, the walk halts.  Otherwise
 *     x = u(seed,i,t,0) * total (one fp64 multiply).  pos is the first position in [lo,hi) with cdf[pos] > x.  If there
 *     is none (rounding), pos is the first position with cdf[pos] == total.  The search is a bisection, O(log deg).
 *  5. trace[i][t+1] = indices[pos], eids[i][t] = data ? data[pos] : pos, curr = indices[pos].
 * A halted walk writes -1 into trace[i][t+1 ..] and eids[i][t ..].  trace[i][0] = seeds[i] always.  A seed outside
 * [0, num_rows of rels[metapath[0]]) halts at once and touches no memory through that id.
 *
 * CDF of a relation, as double[nnz] in CSR position order: cdf[pos] = sum_{q = lo..pos} w'(q), with
 * w'(q) = max((double)prob[data ? data[q] : q], 0) and NaN -> 0.  `prob` is indexed by EDGE ID.  The order of additions
 * is free, but cdf never decreases inside a row, and w'(pos) == 0 implies cdf[pos] == cdf[pos-1], so a zero-weight
 * edge is never picked.
 *
 * dgla_random_walk_cdf: builds that CDF (device memory, double[nnz]) from `prob` (float32 / float64 per EDGE ID); no
 *   floating-point atomics, the same bits on every run.  Its workspace is empty today; pass what
 *   dgla_random_walk_cdf_workspace_bytes says.
 * dgla_random_walk: `rels` and `metapath` are HOST arrays (the table holds device pointers), everything else is device
 *   memory of the table's id type.  Up to 16 relations and 256 steps travel in the kernel arguments; a larger table or
 *   metapath goes through `workspace` (dgla_random_walk_workspace_bytes, 0 while both fit).  eids may be NULL.
 *   restart_prob is used when restart_steps == NULL (0 = no restart); restart_steps is float32 / float64 [num_steps].
 * The calls allocate nothing, read nothing back and do not synchronise.  They fail with -1 and a message for a NULL
 *   table, relations of mixed id width, metapath[t] out of range, a metapath whose node types do not chain
 *   (rels[metapath[t]].csr->num_cols != rels[metapath[t+1]].csr->num_rows) and a workspace that is too small.
 *   num_seeds == 0 and num_steps == 0 are valid.
 * dgla_random_walk_host: the same arguments with every pointer in HOST memory, no stream and no workspace: the same
 *   rule run by the CPU, bit for bit what the kernel writes.  Host-only: needs no GPU. */
typedef struct {
  const dgla_csr* csr; /* out-edge CSR: rows = source nodes */
  const double* cdf;   /* [nnz] from dgla_random_walk_cdf, or NULL = uniform */
} dgla_walk_relation;
size_t dgla_random_walk_cdf_workspace_bytes(const dgla_csr* csr);
int dgla_random_walk_cdf(const dgla_csr* csr, const void* prob, dgla_dtype prob_dtype, double* cdf, void* workspace,
                         size_t workspace_bytes, void* hip_stream);
size_t dgla_random_walk_workspace_bytes(int num_rels, int64_t num_steps);
int dgla_random_walk(const dgla_walk_relation* rels, int num_rels, const int32_t* metapath, int64_t num_steps,
                     const void* seeds, int64_t num_seeds, double restart_prob, const void* restart_steps,
                     dgla_dtype restart_dtype, uint64_t rng_seed, void* traces, void* eids, void* workspace,
                     size_t workspace_bytes, void* hip_stream);
int dgla_random_walk_host(const dgla_walk_relation* rels, int num_rels, const int32_t* metapath, int64_t num_steps,
                          const void* seeds, int64_t num_seeds, double restart_prob, const void* restart_steps,
                          dgla_dtype restart_dtype, uint64_t rng_seed, void* traces, void* eids);

/* ---- node2vec walks: a bounded second-order step (csrc/node2vec.hip) ------------------------------
 * Replace Node2vecRandomWalk (src/graph/sampling/randomwalks/node2vec_randomwalk.h:67-147, CPU only, behind
 * dgl.sampling.node2vec_random_walk, python/dgl/sampling/node2vec_randomwalk.py).  The reference's step is an unbounded
 * rejection loop; here a step makes at most K attempts and then scans the row once, with the same law.  The generator,
 * the draws r(seed,i,t,k), index() and u(), and the CDF are those of "Random walks" above.  The step rule (ONE
 * definition for device and host, csrc/node2vec_step.h):
 *
 * Setting.  One relation with num_rows == num_cols, as its out-edge CSR (indptr, indices, data = edge-id map or NULL),
 * an optional CDF (double[nnz] from dgla_random_walk_cdf, NULL = uniform) and a membership list member[nnz]: the
 * column ids of every row in ascending order, duplicates kept, over the same indptr (dgla_csr_sorted_columns).
 *
 * Parameters.  p and q are finite and > 0.  The host computes, once per call,
 *     m = max(1/p, 1, 1/q),   a0 = (1/p)/m,   a1 = 1/m,   a2 = (1/q)/m
 * and refuses the call when m is not finite or some a is not > 0; the walk itself divides nothing.
 *
 * Class of a candidate x when the previous node is prev: class 0 if x == prev (a self-loop or a duplicate edge is
 * judged by node id); else class 1 if the edge x -> prev exists, i.e. a bisection of member[indptr[x] .. indptr[x+1])
 * finds prev; else class 2.  a_class(x) is a0, a1 or a2.
 *
 * Step t = 0 of walk i at its seed: rules 2-5 of csrc/random_walk_step.h (no restart), the pick from slot 0.
 * Step t >= 1 at curr with row [lo, hi), deg = hi - lo, the node before curr being prev:
 *  1. If deg == 0, the walk halts.
 *  2. Weighted relation: total = cdf[hi-1]; if !(total > 0) or total is not finite, the walk halts.
 *  3. Bounded rejection.  K = min(max(deg, 8), 1024).  For attempt k = 0 .. K-1: the candidate position is
 *     pos = lo + index(r(seed,i,t,2k), deg) (uniform) or the weighted pick of rule 4 of csrc/random_walk_step.h with
 *     r(seed,i,t,2k) (weighted); x = indices[pos]; the candidate is accepted iff u(seed,i,t,2k+1) < a_class(x).
 *     (A class whose a is 1.0 always accepts, because u < 1.)
 *  4. After K rejections, an exact scan of the row in position order, in fp64, every operation rounded on its own:
 *     d_j = 1 (uniform) or cdf[j] - (j > lo ? cdf[j-1] : 0) (weighted);  g_j = fl(d_j * a_class(indices[j]));
 *     S = fl(S + g_j) for j = lo .. hi-1 in that order, from S = 0.  If !(S > 0), the walk halts.
 *     x = u(seed,i,t,2K) * S.  A second pass forms the same running sum and takes the first j whose running sum
 *     is > x.  If there is none (rounding), it takes the last j with g_j > 0.
 *  5. trace[i][t+1] = indices[pos], eids[i][t] = data ? data[pos] : pos, prev = curr, curr = indices[pos].
 * A halted walk writes -1 into trace[i][t+1 ..] and eids[i][t ..].  trace[i][0] = seeds[i] always.  A seed outside
 * [0, num_rows) halts at once and touches no memory through that id.
 *
 * What follows from the rule.  Picks are a pure function of (seed, walk index, step, slot).  Rejection and the scan
 * draw from the same law, P(j) proportional to d_j * a_class(indices[j]), so falling through after K rejections does
 * not bias the walk.  With p == q == 1 every a is 1.0, attempt 0 accepts, and the walk is the one of
 * csrc/random_walk_step.h under the same seed, bit for bit.  A step costs at most K attempts and two scans of the row.
 *
 * K follows the degree because an attempt and one row position of the scan cost about the same (one gather and one
 * bisection): K is part of the rule, not a tuned number.
 *
 * Floating point.  g_j and S are a multiply followed by an add: two roundings.  A device compiler contracts the pair
 * into one fused multiply-add (one rounding) unless told otherwise, a host compiler does not, and the two would then
 * disagree in the last bit of S: `#pragma clang fp contract(off)` in n2v_scan keeps them apart on every target.
 * Everything else is integer arithmetic, single fp64 operations and fp64 compares.
 *
 * dgla_csr_sorted_columns: writes the membership list of `csr` to member[nnz] (device memory, the CSR's id type):
 *   every row's column ids in ascending order, duplicates kept, over the same indptr.  Two runs of the stable sort of
 *   dgla_coo_to_csr (by column, then by row); multigraphs and self-loops are fine; the same bytes on every run; the
 *   edge-id map plays no part.  `workspace` must hold dgla_csr_sorted_columns_workspace_bytes bytes: the call
 *   allocates nothing, reads nothing back and does not synchronise.
 * dgla_node2vec_walk: csr, cdf (NULL = uniform), member, seeds, traces [num_seeds, num_steps + 1] and eids
 *   [num_seeds, num_steps] (may be NULL) are device memory of the CSR's id type; no workspace, no allocation, nothing
 *   read back, no synchronisation.
 * dgla_node2vec_walk_host: the same arguments with every pointer in HOST memory and no stream: the same rule run by
 *   the CPU, bit for bit what the kernel writes.  Host-only: needs no GPU.  `stats` may be NULL; otherwise it receives
 *   {steps t >= 1 that recorded a node, candidates drawn by the rejection loops, steps that reached the scan}.  The
 *   device kernel keeps no such counters.
 * All fail with -1 and a message, before any launch, for a NULL csr / indices / member / seeds / traces, an id width
 *   other than 32 / 64, num_rows != num_cols, negative sizes, p or q that is not finite and > 0 (or whose m or
 *   acceptance probabilities are not usable) and a workspace that is too small.  num_seeds == 0 and num_steps == 0
 *   are valid. */
size_t dgla_csr_sorted_columns_workspace_bytes(const dgla_csr* csr);
int dgla_csr_sorted_columns(const dgla_csr* csr, void* member, void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_node2vec_walk(const dgla_csr* csr, const double* cdf, const void* member, const void* seeds, int64_t num_seeds,
                       int64_t num_steps, double p, double q, uint64_t rng_seed, void* traces, void* eids,
                       void* hip_stream);
int dgla_node2vec_walk_host(const dgla_csr* csr, const double* cdf, const void* member, const void* seeds,
                            int64_t num_seeds, int64_t num_steps, double p, double q, uint64_t rng_seed, void* traces,
                            void* eids, int64_t* stats);

/* ---- Negative sampling: global uniform pairs and the edge lookup (csrc/negative_sampling.hip) -----
 * Replace CSRGlobalUniformNegativeSampling<kDGLCUDA> (src/array/cuda/negative_sampling.cu, behind
 * dgl.sampling.global_uniform_negative_sampling, python/dgl/sampling/negative.py) and the search behind
 * DGLGraph.has_edges_between.  The reference draws with Philox, selects with cub and, without replacement, sorts the
 * pairs and returns the lexicographically smallest num_samples of them; here the first occurrences are kept in slot
 * order, so the truncation is an unbiased sample.  The generator and the draws are those of "Random walks" above.  The
 * rule (ONE definition for device and host, csrc/negative_sample_step.h):
 *
 * Setting.  One relation as its out-edge CSR (R = num_rows source nodes, C = num_cols destination nodes, indptr) and
 * its membership list member[nnz]: the column ids of every row in ascending order, duplicates kept, over the same
 * indptr (dgla_csr_sorted_columns).  Parameters: n_slots >= 0 slots, num_samples >= 0 result entries, num_trials T in
 * 1..64, the flags exclude_self_loops and replace, and a 64-bit seed.
 *
 * The rule:
 *  1. Draw.  For slot i in [0, n_slots), trial t = 0 .. T-1:  s = rw_step_key(rw_walk_key(seed, i), t),
 *     u = rw_index(rw_draw(s, 0), R), v = rw_index(rw_draw(s, 1), C).  The trial is rejected in either of two cases:
 *     exclude_self_loops and u == v; or n2v_member(member, indptr[u], indptr[u+1], v) finds v (u -> v is an edge).
 *     The first trial that is not rejected gives the slot its pair (u, v).  A slot with T rejections is empty.
 *     R == 0 or C == 0 leaves every slot empty and reads no graph memory.
 *  2. Accept.  A is the list of non-empty slots in ascending i.
 *  3. Select.  With replace, the result is the first min(|A|, num_samples) pairs of A.  Without replace, first drop
 *     from A every slot whose pair equals the pair of an earlier slot of A (first occurrences are kept, in slot order),
 *     then take the first num_samples.
 *  4. Pad.  out_src and out_dst have num_samples entries of the CSR's id type; the entries beyond the count are -1.
 *     The count is one int64.
 *
 * What follows from the rule.  The result is a pure function of (graph, seed, n_slots, num_samples, T, flags),
 * whatever the launch geometry.  The result for num_samples = k is a prefix of the result for k' > k at the same
 * n_slots.  A slot's pair is uniform over the cells that are neither edges nor (when excluded) self-loops, slots are
 * independent, and first occurrences are kept in slot order, so the truncation to num_samples is an unbiased sample
 * without replacement.  How duplicates are found (a hash bucket sort on the device, a set on the host) is no part of
 * the rule.
 *
 * Integer arithmetic and integer compares only: host and device agree bit for bit.
 *
 * dgla_negative_sample: csr->indptr, member, out_src[num_samples], out_dst[num_samples] (the CSR's id type) and
 *   out_count (one int64) are device memory; csr->indices and csr->data are not read.  `workspace` must hold
 *   dgla_negative_sample_workspace_bytes(idtype_bits, n_slots) bytes, a number that depends on n_slots only (50 to 100
 *   bytes per slot; nothing is sized by num_rows, num_cols or nnz).  Everything is stream-ordered: no allocation,
 *   nothing read back, no synchronisation, usable inside a hipGraph capture.  The accepted count stays on the device:
 *   the duplicate search sorts all n_slots slots, the empty ones spread over the buckets by slot index and stepped over.
 * dgla_negative_sample_host: the same arguments with every pointer in HOST memory, no workspace and no stream: the
 *   whole rule run sequentially by the CPU, bit for bit what the kernels write.  Host-only: needs no GPU.
 * dgla_csr_has_edges: out[i] = 1 iff 0 <= u[i] < R, 0 <= v[i] < C and the bisection of row u[i] of the membership list
 *   finds v[i], else 0; u, v (the CSR's id type) and out (n bytes) are device memory.  An id out of range touches no
 *   memory.  dgla_csr_has_edges_host: the same on host memory.
 * All fail with -1 and a message, before any launch, for a NULL csr / indptr / member / output, an id width other than
 *   32 / 64, negative sizes, num_trials outside 1..64, n_slots or num_samples >= 2^31 and a workspace that is too small.
 *   n_slots == 0 and num_samples == 0 are valid. */
size_t dgla_negative_sample_workspace_bytes(int idtype_bits, int64_t n_slots);
int dgla_negative_sample(const dgla_csr* csr, const void* member, int64_t n_slots, int64_t num_samples, int num_trials,
                         int exclude_self_loops, int replace, uint64_t seed, void* out_src, void* out_dst,
                         int64_t* out_count, void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_negative_sample_host(const dgla_csr* csr, const void* member, int64_t n_slots, int64_t num_samples, int num_trials,
                              int exclude_self_loops, int replace, uint64_t seed, void* out_src, void* out_dst,
                              int64_t* out_count);
int dgla_csr_has_edges(const dgla_csr* csr, const void* member, const void* u, const void* v, int64_t n, uint8_t* out,
                       void* hip_stream);
int dgla_csr_has_edges_host(const dgla_csr* csr, const void* member, const void* u, const void* v, int64_t n, uint8_t* out);

/* ---- Layer-neighbour sampling: LABOR-0 over whole rows (csrc/labor.hip) -----------------------------
 * Replace CSRLaborSampling<kDGLCUDA> (src/array/cuda/labor_sampling.cu over src/array/labor_pick.h, behind
 * dgl.sampling.sample_labors and dgl.dataloading.LaborSampler, python/dgl/sampling/labor.py): layer-neighbour sampling
 * of Balin and Catalyurek (arXiv:2210.13339) with importance_sampling = 0.  One random variate per SOURCE NODE instead
 * of one per edge, so seeds that share a neighbour keep or drop it together.  The generator and the draws are those of
 * "Random walks" above.  The rule (ONE definition for device and host, csrc/labor_step.h):
 *
 * Setting.  One relation as a CSR whose rows are the seed side (the in-edge CSR for edge_dir = "in", the out-edge CSR
 * for "out"): indptr, indices (neighbour ids), data (the edge-id map or NULL).  Parameters: seeds[n], a fanout k (an
 * int >= 0, or negative for "all"), a 64-bit seed and optionally prob, indexed by EDGE ID (fp32 or fp64).  A seed
 * outside [0, num_rows) is a row of degree 0 and touches no memory through that id.
 *
 * Variate.  r(t) = rw_draw(rw_step_key(rw_walk_key(seed, t), 0), 0) for neighbour node id t: a function of (seed, t)
 * only.  The seed row, the relation, the layer and the position in `seeds` do not enter it.
 *
 * Uniform rule (no prob).  Row i with lo = indptr[seeds[i]], hi = indptr[seeds[i] + 1], d = hi - lo.  If k < 0 or
 * d <= k every position is kept.  Otherwise position q is kept iff rw_index(r(indices[q]), d) < k (integers only; the
 * inclusion probability is k / d to within 2^-64).
 *
 * Weighted rule.  w'(q) = rw_weight(prob[data ? data[q] : q]) (negative and NaN weights count as 0).  P = the number of
 * positions of the row with w' > 0, W = their sum.  With the row's scale c_i, p(q) = min(1, c_i * w'(q)), ONE fp64
 * multiply, and q is kept iff c_i > 0, w'(q) > 0 and rw_uniform(r(indices[q])) < p(q).  The scale carries the special rows:
 *   W not finite -> c_i = 0 (nothing is kept);  else k < 0 or P <= k -> c_i = +inf (p = 1 exactly where w' > 0);
 *   else c_i finite, by the iteration below.
 *
 * Scale.  c_i solves sum_q min(1, c * w'(q)) = k (the paper's definition: the expected number of kept edges is k), by
 * the finite saturation iteration:  c <- k / W;  repeat  m = #{q: c * w'(q) >= 1},  U = sum of w'(q) over
 * c * w'(q) < 1,  c <- (k - m) / U;  stop when m no longer changes.  c only rises and m < k holds throughout.  At most
 * kLaborMaxPasses = 64 passes; when the bound is reached the current c is used.  The law stays exact for any c: the
 * importances use the actual p, only the expected count drifts.  The order of the additions is free, so the scale is a
 * separate step with its own output double c[n] (device and host agree to rounding), and the pick takes c as an input.
 * (The reference instead matches a variance target, equation 22 of the paper, labor_pick.h:122-152, and so samples
 * more than k edges per seed on a weighted graph.)
 *
 * Importances (weighted form only).  For a kept q, a(q) = w'(q) / p(q); the output is a(q) * (n_i / S_i) in prob's
 * dtype, n_i the row's kept count and S_i the sum of a over the row's kept positions, computed in fp64 in the fixed
 * order csrc/labor_step.h states (64 position classes, then a tree).  A row's importances sum to n_i.
 *
 * Order.  Output goes seed by seed in the given order and, within a seed, in ascending CSR position.  For every kept
 * edge: the neighbour id indices[q], the edge id (data[q], or q) and, weighted, the importance.
 *
 * The result is a pure function of (graph, seeds, k, seed, prob, c), whatever the launch geometry; pick on the device
 * and pick on the host agree bit for bit from the same c.  No atomics.
 *
 * dgla_labor_workspace_bytes: the workspace dgla_labor_count and dgla_labor_fill share, 16 bytes per seed plus the
 *   scan's scratch; 0 for num_seeds <= 0 or another id width.  Nothing is sized by the graph.
 * dgla_labor_scale: c[num_seeds] (device) for a weighted call; csr->indptr, csr->data, prob, seeds are device memory,
 *   csr->indices is not read.  One launch, a group of lanes per row, up to 64 passes over the row.
 * dgla_labor_count: out_indptr[num_seeds + 1] (the CSR's id type) and *total (one int64), both device memory; prob
 *   NULL = uniform (c is then ignored), else c from dgla_labor_scale.  Offsets by the library's own scan; stream-ordered,
 *   no allocation, nothing read back.  It leaves the offsets and the rows' importance sums in the workspace.
 * dgla_labor_fill: with the same arguments and the workspace count left, writes out_nbr / out_eid (the id type) and,
 *   weighted, out_imp (prob's dtype), each of `capacity` >= total entries; no write goes past capacity.
 * A group of 16 lanes serves a row when csr->nnz / csr->num_rows <= 32, a wavefront of 64 otherwise; the bits written
 *   do not depend on it.
 * dgla_labor_scale_host / dgla_labor_pick_host: the same rule run by the CPU on HOST pointers, no workspace and no
 *   stream.  pick_host with out_nbr == NULL writes out_indptr only (the sizes); otherwise out_nbr / out_eid / out_imp
 *   must hold out_indptr[num_seeds] entries.  Host-only: need no GPU.
 * All fail with -1 and a message, before any launch, for a NULL csr / indptr / indices / seeds / output, an id width
 *   other than 32 / 64, negative sizes, num_seeds >= 2^31, a prob dtype other than fp32 (0) / fp64 (1), a weighted call
 *   without c and a workspace that is too small.  num_seeds == 0 and nnz == 0 are valid and read no graph memory. */
size_t dgla_labor_workspace_bytes(int idtype_bits, int64_t num_seeds);
int dgla_labor_scale(const dgla_csr* csr, const void* prob, int prob_dtype, const void* seeds, int64_t num_seeds,
                     int64_t fanout, double* c, void* hip_stream);
int dgla_labor_count(const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, const void* seeds,
                     int64_t num_seeds, int64_t fanout, uint64_t seed, void* out_indptr, int64_t* total, void* workspace,
                     size_t workspace_bytes, void* hip_stream);
int dgla_labor_fill(const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, const void* seeds,
                    int64_t num_seeds, int64_t fanout, uint64_t seed, int64_t capacity, void* out_nbr, void* out_eid,
                    void* out_imp, const void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_labor_scale_host(const dgla_csr* csr, const void* prob, int prob_dtype, const void* seeds, int64_t num_seeds,
                          int64_t fanout, double* c);
int dgla_labor_pick_host(const dgla_csr* csr, const void* prob, int prob_dtype, const double* c, const void* seeds,
                         int64_t num_seeds, int64_t fanout, uint64_t seed, void* out_indptr, void* out_nbr, void* out_eid,
                         void* out_imp);

/* ---- Point-cloud graphs: k nearest neighbours per segment, farthest points (csrc/knn.hip) -----------
 * Replace BruteforceKnnKernel / BruteforceKnnShareKernel (src/graph/transform/cuda/knn.cu, behind dgl.knn_graph,
 * dgl.segmented_knn_graph and dgl.functional.knn) and fps_kernel (src/geometry/cuda/geometry_op_impl.cu, behind
 * dgl.geometry.farthest_point_sampler).  The reference's result depends on heap order and on which thread wins a tie;
 * here it has one total order.  The rule (ONE definition for device and host, csrc/knn_step.h):
 *
 * Distance.  Rows have D >= 1 columns of the operand type T (fp32 or fp64; fp16 / bf16 are refused).  d(q, p) is the
 * squared Euclidean distance computed in T as ONE chain of fused multiply-adds in ASCENDING COLUMN ORDER:
 *     acc = 0;   for j = 0, 1, ..., D - 1:   t = q[j] - p[j];   acc = fma(t, t, acc);   d = acc.
 * The chain does not depend on launch geometry, tile sizes, k or the segment; a wide row walked in column chunks
 * carries acc from chunk to chunk.  fma is spelled as fma on both sides, never left to contraction.
 *
 * Abandoning.  The partial sums of a chain never decrease (a NaN partial sum stays NaN), so a candidate whose partial
 * sum compares greater than the distance of the current k-th key may be abandoned: its key loses whatever the
 * remaining columns hold.  Permitted, never required; the result cannot change.
 *
 * Order.  Candidates compare by the key (d, data row id), ascending.  A NaN distance orders as +inf and is written as
 * +inf; ties in d fall to the smaller id.
 *
 * k-NN result.  x_offsets[S + 1] and y_offsets[S + 1] (HOST arrays, ascending from 0, ending at num_x / num_y) cut the
 * data rows x and the query rows y into S segments.  For query row i of y in segment s the result is the k smallest
 * keys among the rows of x in segment s, written to slots i * k ... i * k + k - 1 in ascending key order:
 * out_ids[slot] = i, out_ids[k * num_y + slot] = the GLOBAL row id in x (the reference's (2, k * num_y) tensor, in the
 * id type), out_dist[slot] = d (type T; out_dist may be NULL).  A segment with fewer than k data rows leaves its last
 * slots at id -1 and distance +inf.  y == NULL is the self-query y = x (then num_y == num_x).
 *
 * Farthest points.  Per cloud of N rows (pos is [batch, N, D]) with start row s = start[cloud] and n <= N samples:
 *   1. mind[i] = +inf for every row;  out[0] = s.
 *   2. After choosing c = out[t]:  mind[c] = -1 (chosen, never chosen again); for every other row
 *      dd = d(p_i, p_c);  mind[i] = dd < mind[i] ? dd : mind[i].
 *   3. out[t + 1] = the row with the largest mind; ties go to the smallest i.
 * On distinct points this is the textbook sampler; coincident points come in ascending id, never one row twice.  A NaN
 * distance lowers nothing: a row with a NaN coordinate keeps mind = +inf until it is chosen (such rows go first, in
 * ascending i) and lowers no other row's mind afterwards.  out holds row numbers INSIDE the cloud, int64.
 *
 * The results are a pure function of the inputs: no atomics, the same bytes on every run, device == host bit for bit.
 *
 * dgla_knn_max_k: kKnnMaxK = 64, the largest k.  dgla_knn_tile_sizes: queries per workgroup and data rows per LDS tile.
 * dgla_knn_workspace_bytes: the tile table (three int64 per segment boundary, 256-byte aligned); 0 for num_segs <= 0.
 * dgla_knn: x, y, out_ids, out_dist and the workspace are device memory; the offsets are host memory and are copied
 *   to the workspace in stream order.  One launch: a wavefront owns 64 queries of one segment and streams the segment's
 *   data rows through LDS; the k best keys of a query live in LDS.  No allocation, nothing read back.
 * dgla_fps_workspace_bytes: 0 up to 4096 rows per cloud (mind lives in LDS), else batch * num_rows values of T.
 * dgla_fps: pos, start [batch] (int64), out [batch, npoints] (int64) and the workspace are device memory.  One launch,
 *   one workgroup per cloud, the loop over the samples inside it.  A start outside [0, num_rows) counts as row 0.
 * dgla_knn_host / dgla_fps_host: the same rule run by the CPU on HOST pointers, no workspace and no stream.
 * All fail with -1 and a message, before any launch, for fp16 / bf16 operands (by name), an id width other than
 *   32 / 64, dim < 1, k < 1, k above kKnnMaxK (by name), NULL x / offsets / outputs, offsets that do not match (not
 *   starting at 0, descending, or not ending at the row count), num_x or num_y >= 2^31 - 64, k * num_y >= 2^31 with
 *   int32 ids, npoints outside [1, num_rows] and a workspace that is too small.  num_y == 0 and batch == 0 are valid. */
int dgla_knn_max_k(void);
int dgla_knn_tile_sizes(int* query_tile, int* data_tile);
size_t dgla_knn_workspace_bytes(int64_t num_segs);
int dgla_knn(const void* x, int64_t num_x, const void* y, int64_t num_y, int dtype, int64_t dim, const int64_t* x_offsets,
             const int64_t* y_offsets, int64_t num_segs, int64_t k, int idtype_bits, void* out_ids, void* out_dist,
             void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_knn_host(const void* x, int64_t num_x, const void* y, int64_t num_y, int dtype, int64_t dim,
                  const int64_t* x_offsets, const int64_t* y_offsets, int64_t num_segs, int64_t k, int idtype_bits,
                  void* out_ids, void* out_dist);
size_t dgla_fps_workspace_bytes(int dtype, int64_t batch, int64_t num_rows);
int dgla_fps(const void* pos, int dtype, int64_t batch, int64_t num_rows, int64_t dim, int64_t npoints, const int64_t* start,
             int64_t* out, void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_fps_host(const void* pos, int dtype, int64_t batch, int64_t num_rows, int64_t dim, int64_t npoints,
                  const int64_t* start, int64_t* out);

/* ---- Graph matching: neighbour matching for edge coarsening (csrc/matching.hip) ---------------------
 * Replaces NeighborMatching<kDGLCUDA> (src/geometry/cuda/edge_coarsening_impl.cu, behind
 * dgl.geometry.neighbor_matching): the edge-coarsening step of Graclus pooling and of multilevel partitioning.  The
 * reference reads `result` while the same kernel writes it, so its output depends on thread timing, and it never ends
 * on a CSR that is not symmetric.  The rule (ONE definition for device and host, csrc/matching_step.h):
 *
 * Input.  One CSR with indptr[n + 1], indices[nnz] and data[nnz] as the edge-id map (or NULL); ids are int32 or int64.
 * Optional non-negative edge weights are indexed by EDGE ID, fp32 or fp64.  A 64-bit seed is given.
 *
 * State.  label[n] starts at -1 and prop[n] starts at -1 (NONE), both in the id type.  The rule runs in rounds
 * t = 0, 1, ....  A node is ACTIVE in round t when its label is negative at the start of the round.
 *
 * Colour.  Node v in round t is BLUE when rw_draw(rw_step_key(rw_walk_key(seed, v), t), 0), the generator of
 * "Random walks" used unchanged, is below 0x88b827fa1a0cf000 = floor(0.53406 * 2^64) (0.53406 as fp64; the BLUE_P of
 * the reference, from Fagginger Auer and Bisseling).  Otherwise v is RED.  A colour is a function of (seed, v, t)
 * only; it is never stored, and a neighbour's colour is recomputed in registers, not gathered.
 *
 * Key of entry q = (u -> v): the tuple (w', h, v).  w' = max((double)weight[data ? data[q] : q], 0) with NaN -> 0
 * (the w' of "Random walks"), so every active neighbour stays a candidate and the loop cannot starve on such weights.
 * Without weights w' = 0 and NO weight array exists or is read.  With a = min(u, v) and b = max(u, v),
 *     h = mix64( mix64( (seed ^ 0x6D61746368696E67) ^ (a * 0xD1B54A32D192ED03) ) + b )          (all mod 2^64),
 * so both directions of an edge agree on h; it breaks weight ties at random (the all-ones weights users pass are the
 * common case).  The larger (w', h) wins; on a full tie the smaller v wins.  Entries with v == u are ignored, and so are
 * entries whose v is outside [0, n).
 *
 * Propose.  Reads label and writes only prop[u], for every active u.  If u has no active neighbour, prop[u] = SINGLE
 * (-2).  Else if u is BLUE, prop[u] = the active RED neighbour with the best key, or NONE (-1) if it has none.  Else
 * prop[u] = NONE.
 *
 * Respond.  Reads prop and writes label.  An active u whose prop[u] is SINGLE takes label[u] = u.  An active RED u
 * picks the neighbour v with the best key among those that are BLUE and proposed to u IN THIS ROUND, and sets
 * label[u] = label[v] = min(u, v).  No other node writes label[v]; the only reader of label[v] in this phase is v
 * itself, and v does nothing whichever value it sees.  (Propose rewrites the prop of every active node in every round,
 * so prop[v] == u is this round's proposal for an active v; for an inactive v it can only name a u that matched in
 * the round v did: csrc/matching_step.h.)
 *
 * End.  The loop ends when no node is active; `rounds` is the number of rounds that started with an active node.  It
 * also stops after max_rounds rounds: if nodes are still active then, the call fails with a message that says the graph
 * is probably not bi-directed (a CSR that is not symmetric can cycle for ever; a directed 3-cycle does).  On
 * bi-directed graphs a numpy model of the rule used 13 - 18 rounds at 100 000 nodes.
 *
 * What follows from the rule:
 *   - The labels (and `rounds`) are a pure function of (CSR, weights, seed, max_rounds), whatever the launch geometry,
 *     the thread timing, the batching of rounds between read-backs and the symmetry of the CSR; device == host bit for
 *     bit.
 *   - Every label is the smaller id of its cluster, and label[label[i]] == label[i].
 *   - Clusters have one or two nodes.
 *   - The two nodes of a pair are joined by an entry of the CSR.
 *   - On a symmetric CSR no two singleton clusters are adjacent: the matching is maximal.
 *
 * Relabelling.  new[i] = the number of j < label[i] with label[j] == j: consecutive cluster ids in ascending order of
 * label, np.unique(label, return_inverse=True)[1].
 *
 * dgla_neighbor_matching_workspace_bytes: one workspace for both device entry points (prop or the ranks, one status
 *   word, the scan's temporary); 0 for another id width or num_nodes <= 0.
 * dgla_neighbor_matching: the CSR's arrays, weight, label [num_rows] and the workspace are device memory; *rounds is
 *   HOST memory.  n = csr->num_rows.  Two launches per round, no atomics.  The host queues batch_rounds rounds (<= 0:
 *   the default, 8), reads ONE device word back and stops when the last queued round found no active node; rounds after
 *   that are no-ops, so batch_rounds never changes a result.  workspace == NULL: stream-ordered scratch is allocated
 *   for the call; a workspace that is given but too small is refused with the bytes required.
 * dgla_neighbor_matching_relabel: label -> out [num_nodes] (device, the id type): a flag pass, the library's scan and a
 *   gather; nothing is read back.  The workspace as above.
 * dgla_neighbor_matching_host: the same rule run by the CPU on HOST pointers; `relabel` (may be NULL) receives the
 *   relabelled ids.
 * All fail with -1 and a message that names the entry point for a NULL csr / indptr / indices / label / rounds / out,
 *   an id width other than 32 / 64, fp16 / bf16 weights (by name) or another unknown weight dtype, max_rounds < 1, a
 *   workspace that is too small, and the round cap. */
size_t dgla_neighbor_matching_workspace_bytes(int idtype_bits, int64_t num_nodes);
int dgla_neighbor_matching(const dgla_csr* csr, const void* weight, int weight_dtype, uint64_t seed, int64_t max_rounds,
                           int64_t batch_rounds, void* label, int64_t* rounds, void* workspace, size_t workspace_bytes,
                           void* hip_stream);
int dgla_neighbor_matching_relabel(const void* label, int idtype_bits, int64_t num_nodes, void* out, void* workspace,
                                   size_t workspace_bytes, void* hip_stream);
int dgla_neighbor_matching_host(const dgla_csr* csr, const void* weight, int weight_dtype, uint64_t seed, int64_t max_rounds,
                                void* label, int64_t* rounds, void* relabel);

/* ---- Induced subgraphs: the edges among a list of nodes (csrc/subgraph.hip) ----------------------------
 * The step behind dgl.node_subgraph on a mini-batch of nodes, dgl.khop_in_subgraph / khop_out_subgraph and the ShaDow
 * and SAINT samplers of dgl.dataloading (python/dgl/subgraph.py, python/dgl/dataloading/shadow.py, graphsaint.py).  The
 * reference cuts the subgraph on the CPU (src/graph/unit_graph.cc VertexSubgraph over aten::CSRSliceMatrix).  Here the
 * work is O(sum of deg(selected rows)); nothing of graph size is filled or scanned.  The rule (ONE definition for device
 * and host, csrc/subgraph_step.h):
 *
 * Setting.  One relation as a CSR: indptr, indices, data (the edge-id map, or NULL for the identity).  For
 * in-neighbourhoods this is the in-edge CSR: rows are destinations, indices are sources.  A list rows[nr] of selected
 * row ids, and a dense col_map with one int32 per COLUMN node (csr->num_cols entries): -1 = not selected, otherwise the
 * node's local id.  On a homogeneous graph rows and the column selection are the same list and col_map[rows[i]] == i.
 *
 * Rule.  For position i and row r = rows[i], visit every j in [indptr[r], indptr[r + 1]) in order, with u = indices[j]
 * and l = col_map[u].  The entry is kept iff l >= 0, and then yields the triple
 *     (local_row = i, local_col = l, eid = data ? data[j] : j).
 * A row id outside [0, num_rows) keeps nothing and is never dereferenced; neither is a column id outside [0, num_cols).
 *
 * Order.  Rows of the result go by i, then by j.  out_indptr[i] = the number of kept entries of the positions before i,
 * out_indptr[nr] = the total.  Integer arithmetic only: device == host bit for bit, whatever the launch geometry.
 *
 * dgla_node_map_mark: map[ids[i]] = i for the ids inside [0, map_len); ORs DGLA_SUBGRAPH_OUT_OF_RANGE (1) into the
 *   device word *flags when some id lies outside, and, in a second launch, DGLA_SUBGRAPH_DUPLICATE (2) when
 *   map[ids[i]] != i for some i, i.e. an id appears twice (the racing plain stores are benign: one writer wins and the
 *   loser is seen by the check).  *flags is only ORed into: the caller zeroes it, and may share it between calls.
 * dgla_node_map_clear: writes -1 back at the ids inside [0, map_len).  `map` is caller-owned scratch, all -1 between
 *   calls, exactly like the node_map of dgla_to_block.  Both refuse n >= 2^31 (local ids are int32).
 * dgla_induced_subgraph_workspace_bytes: the workspace of count (total = 0) and of fill in eid order (the `total` count
 *   reported): 8 bytes per row plus the scan's scratch, and for the eid order two id arrays, two 64-bit key arrays of
 *   `total` entries and the sort's tables.  Monotone in total.  0 for another id width or negative sizes.
 * dgla_induced_subgraph_count: out_indptr[nr + 1] (device, the CSR's id type): the kept entries per row, counted by a
 *   group of 16 lanes per row when csr->nnz / csr->num_rows <= 32 and a wavefront of 64 otherwise (the bits written do
 *   not depend on it), then the library's own scan.  Stream-ordered, no allocation, no atomics, nothing read back: the
 *   caller reads out_indptr[nr] (and the flags word of mark) before it sizes the outputs of fill.
 * dgla_induced_subgraph_fill: the same sweep; a kept entry goes to out_indptr[i] + (kept so far in the row) +
 *   popcount(lower lanes of the group's ballot bits).  out_row / out_col / out_eid hold `total` = out_indptr[nr] entries
 *   (the caller read it back); no write goes past total.  eid_order == 0: the outputs stay in row order and, with
 *   out_indptr, are the subgraph's CSR over the selected rows.  eid_order != 0: the call finishes by permuting the three
 *   arrays into ascending eid, ties by row-order position, with the library's own stable sort (csrc/sort.hip.h) over
 *   keys (eid << bits(total)) | position; edge ids are distinct, so the result is unique.  Edge ids must lie in
 *   [0, csr->nnz) (the edge-id map is a permutation, as everywhere in this header), and bits(nnz) + bits(total) <= 63.
 *   Row-order calls need no workspace.
 * dgla_induced_subgraph_host: the same rule run by the CPU on HOST pointers, no workspace and no stream.  It takes the
 *   column selection as the list cols[nc] and builds its own map; *total and *flags (the bits above, also set for a row
 *   id outside [0, num_rows)) are host words.  out_row == NULL: out_indptr, *total and *flags only (the sizes).
 * All fail with -1 and a message, before any launch, for a NULL csr / indptr / indices / rows / ids / map / flags /
 *   output, an id width other than 32 / 64, negative sizes, nr or n >= 2^31 and a workspace that is too small.  nr == 0
 *   and total == 0 are valid. */
#define DGLA_SUBGRAPH_OUT_OF_RANGE 1
#define DGLA_SUBGRAPH_DUPLICATE 2
int dgla_node_map_mark(int idtype_bits, const void* ids, int64_t n, int32_t* map, int64_t map_len, int32_t* flags,
                       void* hip_stream);
int dgla_node_map_clear(int idtype_bits, const void* ids, int64_t n, int32_t* map, int64_t map_len, void* hip_stream);
size_t dgla_induced_subgraph_workspace_bytes(int idtype_bits, int64_t nr, int64_t total);
int dgla_induced_subgraph_count(const dgla_csr* csr, const void* rows, int64_t nr, const int32_t* col_map, void* out_indptr,
                                void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_induced_subgraph_fill(const dgla_csr* csr, const void* rows, int64_t nr, const int32_t* col_map,
                               const void* out_indptr, int64_t total, void* out_row, void* out_col, void* out_eid,
                               int eid_order, void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_induced_subgraph_host(const dgla_csr* csr, const void* rows, int64_t nr, const void* cols, int64_t nc,
                               int eid_order, void* out_indptr, void* out_row, void* out_col, void* out_eid, int64_t* total,
                               int32_t* flags);

/* ---- Edge exclusion and compaction: link-prediction batches (csrc/exclude.hip) ------------------------
 * The steps a link-prediction / edge-classification mini-batch needs on top of neighbour sampling: drop the seed edges
 * (and their reverses) from every sampled frontier (python/dgl/sampling/utils.py EidExcluder, dataloading/base.py
 * find_exclude_eids) and renumber the end points of the positive and negative pair graphs into one compact node space
 * (dgl.compact_graphs, src/graph/transform/cuda/cuda_compact_graph.cu).  The rules (ONE definition for device and host,
 * csrc/exclude_step.h):
 *
 * The exclusion set X.  n_x edge ids sorted ascending, duplicates allowed, in the graph's id width.  member(X, n_x, e)
 * is a lower-bound bisection (the first position whose id is >= e) followed by an equality test.  No atomics, nothing
 * sized by the graph, no state to clean afterwards.
 *
 * Building X.  Seed edge ids ids[n] and optionally a reverse map rev[num_edges].  Slot k of the unsorted list holds
 * ids[k] for k < n and rev[ids[k - n]] for n <= k < 2n (n slots without rev); X is the slots sorted ascending by the
 * library's own sort.  An id outside [0, num_edges) is never used as an index: its slots hold num_edges (no edge's id)
 * and DGLA_EXCLUDE_OUT_OF_RANGE (1) is ORed into *flags; a rev entry outside the range does the same for its slot.
 *
 * The frontier filter.  A frontier is a CSR over the seeds in the form dgla_sample_neighbors* returns: indptr[nr + 1],
 * src[nnz], eids[nnz].  Entry j is kept iff !member(X, n_x, eids[j]); row i of the result holds the kept entries of
 * [indptr[i], indptr[i + 1]) in their order, out_indptr their offsets.  Sample first, then drop: a row may come out
 * shorter than its fanout.  Row bounds are clamped into [0, nnz].  A pure function of (frontier, X): it does not depend
 * on the launch geometry.
 *
 * Compaction of one node type.  preserve[n_preserve] (repeats allowed) and ends[n_ends] (the end points of this type of
 * every edge of every graph).  nodes = the ids of preserve in the order given, a repeated id at its first position only,
 * then the ids of ends that are not in preserve, ascending, each once (the block rule of dgla_to_block).  local[e] = the
 * index of ends[e] in nodes, *num_out = the length of nodes.  An id outside [0, num_nodes) ORs the bit above into
 * *flags, is never used as an index and gets local -1.
 *
 * dgla_exclude_set: out[n or 2n] (device) = X.  One gather launch, then the sort.  `flags` is one device word the caller
 *   zeroes and reads back.  `workspace` (dgla_exclude_set_workspace_bytes(bits, n, rev != NULL)) is optional: NULL takes
 *   stream-ordered scratch; one that is too small is refused.  n < 2^30.
 * dgla_frontier_exclude: count (a group of 16 lanes per row when nnz / num_rows <= 32, a wavefront of 64 otherwise; every
 *   lane bisects X for its entry, the keep flags of a step are one ballot, the count their popcount; ONE KEEP BYTE per
 *   entry goes to the workspace), the library's scan, fill (reads the keep bytes; a kept entry goes to offset + kept so
 *   far + popcount(lower lanes)).  out_src / out_eids hold nnz entries (the upper bound), out_indptr num_rows + 1; the
 *   first out_indptr[num_rows] entries are the result.  Plain stores, no atomics, nothing read back.  Workspace as above
 *   (dgla_frontier_exclude_workspace_bytes(bits, num_rows, nnz)).
 * dgla_compact_nodes: `node_map` is caller-owned int32 scratch with num_nodes entries, all -1 on entry and again on exit
 *   (exactly the node map of dgla_to_block).  First occurrences in preserve are found with one unsigned atomic min per
 *   id on the map; the rest is the library's sort and scan.  local[n_ends], nodes[n_preserve + n_ends], *num_out and
 *   *flags are device memory; the caller reads the two words back together.  n_preserve + n_ends < 2^31.
 * dgla_exclude_set_host / dgla_frontier_exclude_host / dgla_compact_nodes_host: the same rules run by the CPU on HOST
 *   pointers (*flags, *num_out host words), no workspace, no stream, no node map.
 * All fail with -1 and a message, before any launch, for a NULL array that is needed, an id width other than 32 / 64,
 *   negative sizes, sizes above the bounds given and a workspace that is too small.  Empty inputs are valid. */
#define DGLA_EXCLUDE_OUT_OF_RANGE 1
size_t dgla_exclude_set_workspace_bytes(int idtype_bits, int64_t n, int with_reverse);
int dgla_exclude_set(int idtype_bits, const void* ids, int64_t n, const void* rev, int64_t num_edges, void* out,
                     int32_t* flags, void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_exclude_set_host(int idtype_bits, const void* ids, int64_t n, const void* rev, int64_t num_edges, void* out,
                          int32_t* flags);
size_t dgla_frontier_exclude_workspace_bytes(int idtype_bits, int64_t num_rows, int64_t nnz);
int dgla_frontier_exclude(int idtype_bits, const void* indptr, const void* src, const void* eids, int64_t num_rows,
                          int64_t nnz, const void* x, int64_t n_x, void* out_indptr, void* out_src, void* out_eids,
                          void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_frontier_exclude_host(int idtype_bits, const void* indptr, const void* src, const void* eids, int64_t num_rows,
                               int64_t nnz, const void* x, int64_t n_x, void* out_indptr, void* out_src, void* out_eids);
size_t dgla_compact_nodes_workspace_bytes(int idtype_bits, int64_t n_preserve, int64_t n_ends);
int dgla_compact_nodes(int idtype_bits, const void* preserve, int64_t n_preserve, const void* ends, int64_t n_ends,
                       int32_t* node_map, int64_t num_nodes, void* local, void* nodes, int64_t* num_out, int32_t* flags,
                       void* workspace, size_t workspace_bytes, void* hip_stream);
int dgla_compact_nodes_host(int idtype_bits, const void* preserve, int64_t n_preserve, const void* ends, int64_t n_ends,
                            int64_t num_nodes, void* local, void* nodes, int64_t* num_out, int32_t* flags);

/* ---- Graph traversal: BFS and topological frontiers (csrc/traversal.hip) -------------------------------
 * The frontiers of dgl.bfs_nodes_generator, bfs_edges_generator and topological_nodes_generator, which prop_nodes_bfs /
 * prop_nodes_topo walk (TreeLSTM, junction-tree encoders, sweeps over a DAG).  The reference has no GPU form:
 * python/dgl/traversal.py copies the graph to the CPU on every call and runs a sequential queue there
 * (src/graph/traversal.cc).  The rule (ONE definition for device and host, csrc/traversal_step.h):
 *
 * Input.  One CSR (indptr[n + 1], indices[nnz], data[nnz] = the edge-id map or NULL; int32 or int64 ids): the out-edge
 * CSR for a forward traversal, the in-edge CSR for a reverse one.  For BFS a list of source ids.
 *
 * Expansion position.  Let the current frontier be f[0 .. m) and base[r] the exclusive scan of the row lengths of f[r].
 * Entry j of row f[r] has the position x = off + base[r] + j, where off is the number of entries all earlier frontiers
 * expanded, so positions keep growing across levels and nothing has to be cleared.  x is a 64-bit integer (a level can
 * expand more than 2^32 entries).
 *
 * BFS.  Frontier 0 is the source list as given; duplicates are kept.  From a frontier, every node that no earlier
 * frontier holds and that some entry points at takes key[v] = min x over those entries.  The next frontier is the
 * targets whose entry holds the winning x, in ascending x; the tree edge of v is the edge id of that entry.  Self-loops
 * and parallel edges need no special case.  The loop ends at an empty frontier.
 *
 * Topological.  count[v] = the row length of v in the OPPOSITE CSR (the in-degree for a forward traversal; parallel
 * edges count once each).  Frontier 0 is the nodes with count == 0, ascending.  From a frontier, every entry into v
 * decrements count[v] and key[v] = max x.  The next frontier is the targets with count[v] == 0 whose entry holds the
 * winning x, in ascending x.  If fewer than n nodes were emitted by the end the call fails with "loop detected"; a
 * self-loop is such a loop.
 *
 * This is the order of the reference's sequential queue, which pops the rows of a frontier in order and scans each row
 * in order (ascending x): BFS appends v at the first entry that finds it unseen, the topological sort at the entry that
 * takes its count to 0, which is the last.  Integer arithmetic only; min, max and the decrement commute, so the integer
 * atomics of the kernels leave the same values whatever the arrival order: device == host bit for bit, whatever the
 * launch geometry.  An entry whose target lies outside [0, n) is ignored and nothing is read or written through it.
 *
 * Result.  ids = the frontiers one after the other, sections[k] = the size of the k-th reported frontier; frontiers of
 * size 0 are never reported.  DGLA_TRAVERSE_BFS_NODES reports every frontier, the sources included (ids holds up to
 * n + num_sources entries); DGLA_TRAVERSE_BFS_EDGES reports the tree-edge ids of every frontier after the sources (up to
 * n); DGLA_TRAVERSE_TOPO_NODES reports every frontier (n).  `sections` has the capacity of ids.
 *
 * dgla_traverse_workspace_bytes: the optional workspace: two 64-bit words per node (key, count), the node frontiers of
 *   the edge form, and per frontier row two 64-bit words with the scan's temporary: O(n), nothing of size nnz.  0 for
 *   another id width or num_nodes <= 0.
 * dgla_traverse: the CSR's arrays, sources, ids and the workspace are device memory; sections, *num_ids and
 *   *num_sections are HOST memory (the host loop knows every size).  n = csr->num_rows.  `opposite` is read only by
 *   the topological mode (its indptr), and may be NULL otherwise; `sources` is ignored by the topological mode.  A row
 *   of the frontier is streamed by a group of 16 lanes when csr->nnz / csr->num_rows <= 32 and by a wavefront of 64
 *   otherwise (the bits written do not depend on it).  A level is 6 launches (row lengths, scan, mark, count, scan,
 *   fill; a scan is 3 launches above 32 768 rows) and ONE read-back of 24 bytes; the frontiers land in ids in their
 *   final order, without a sort.  workspace == NULL: stream-ordered scratch is allocated for the call; a workspace that
 *   is given but too small is refused with the bytes required.  A source list longer than n takes scratch of its own
 *   for the row arrays of frontier 0.
 * dgla_traverse_host: the same rule run by the CPU on HOST pointers, no workspace and no stream.
 * Both fail with -1 and a message that names the entry point, before any launch and before any array is read, for an
 *   unknown mode, a NULL csr, an invalid csr (negative sizes, not square, NULL indptr / indices), an id width other than
 *   32 / 64, NULL outputs, a topological call whose opposite CSR is NULL or does not match (its count array has another
 *   number of rows or entries than the csr), and a workspace that is too small.  A source outside [0, n) is refused and
 *   no memory is touched through it: the host twin checks the list (and that indptr is a row pointer) before anything
 *   else; the device form finds it in its first launch, treats it as an empty row and fails at the first read-back. */
#define DGLA_TRAVERSE_BFS_NODES 0
#define DGLA_TRAVERSE_BFS_EDGES 1
#define DGLA_TRAVERSE_TOPO_NODES 2
size_t dgla_traverse_workspace_bytes(int idtype_bits, int64_t num_nodes);
int dgla_traverse(int mode, const dgla_csr* csr, const dgla_csr* opposite, const void* sources, int64_t num_sources,
                  void* ids, int64_t* sections, int64_t* num_ids, int64_t* num_sections, void* workspace,
                  size_t workspace_bytes, void* hip_stream);
int dgla_traverse_host(int mode, const dgla_csr* csr, const dgla_csr* opposite, const void* sources, int64_t num_sources,
                       void* ids, int64_t* sections, int64_t* num_ids, int64_t* num_sections);

/* ---- Top-k neighbour selection (csrc/topk.hip) ------------------------------------------------------------
 * dgl.sampling.select_topk: for every seed the k in- or out-edges with the largest (or smallest) weight.  The reference
 * has no GPU form: python/dgl/sampling/neighbor.py asserts a CPU graph and sorts every row with std::sort
 * (src/array/cpu/rowwise_topk.cc).  The rule (ONE definition for device and host, csrc/topk_step.h):
 *
 * Input.  One CSR (indptr[num_rows + 1], indices[nnz], data[nnz] = the edge-id map or NULL; int32 or int64 ids): the
 * in-edge CSR for edge_dir = "in", the out-edge CSR for "out".  `weight` holds one value per EDGE ID.
 *
 * Key of an edge.  An order-preserving map of its weight to an unsigned integer: 32 bits for fp32 / fp16 / bf16 / int32,
 * 64 bits for fp64 / int64.  Floats: -0.0 becomes +0.0, then a set sign bit complements the pattern and a clear one sets
 * it (the sign-flip map).  fp16 and bf16 widen to the fp32 pattern first, exactly.  Signed integers have their sign bit
 * flipped.  ascending complements the key.  NaN loses to every number in both directions: after the direction is applied
 * its key is 0, below the key of every float that is a number.  An edge id outside [0, nnz) reads no weight and gets
 * key 0 as well.
 *
 * Total order within a row.  Larger key first; among equal keys the smaller EDGE ID first (not the CSR position, so the
 * result is a function of (graph, weights) whichever sparse format is read); among equal edge ids, which only a
 * malformed edge-id map produces, the smaller position.  The order is strict.  The reference's std::sort is unstable:
 * its order among equal weights is unspecified, and this order is one of its possible results; on tie-free weights the
 * two agree element for element.
 *
 * Picks of seed i.  picks = min(k, deg); k = -1: deg; k = 0: none.  The picks are the first `picks` entries of the row in
 * that order, emitted in rank order (best first).  Output is a CSR over the seeds: out_indptr[num_seeds + 1], out_nbr
 * (the `indices` entry of every pick) and out_eids, of out_indptr[num_seeds] entries.  A seed listed twice is selected
 * twice.  Row bounds are clamped into [0, nnz], so a malformed indptr reads nothing outside the arrays.  Integer
 * comparisons only: device == host bit for bit, whatever the launch geometry.
 *
 * dgla_select_topk_max_picks: 1024, the largest number of picks one row may yield.
 * dgla_select_topk_workspace_bytes: the optional workspace: one 64-bit word per seed, the scan's temporary and 8 flag
 *   words.  0 for another id width or num_seeds <= 0.
 * dgla_select_topk: all arrays are device memory.  weight_dtype is a dgla_dtype code, DGLA_TOPK_I32 or DGLA_TOPK_I64.
 *   out_nbr == NULL: the sizes only (out_indptr).  For 0 <= k <= 1024 nothing is read back (the call can be captured when
 *   a workspace is given; allocate num_seeds * k entries) and a seed outside [0, num_rows) is an empty row that touches
 *   no memory.  For k = -1 or k > 1024 the pick counts depend on the degrees: the call reads 8 flag words back after the
 *   count pass and before any selection launch, and refuses a seed outside [0, num_rows) and a row that yields more than
 *   1024 picks ("a row yields N picks, which exceeds the limit of 1024"); the library stays usable afterwards.  A row is
 *   selected by a group of 16 lanes (at most 32 picks, csr->nnz / csr->num_rows <= 32), a wavefront of 64 (at most 128
 *   picks) or a workgroup of 256 (at most 1024), in ONE pass over the row: every selected row's edge ids and weights
 *   are read once.  workspace == NULL: stream-ordered scratch is allocated for the call; a workspace that is given but
 *   too small is refused with the bytes required.
 * dgla_select_topk_host: the same rule run by the CPU on HOST pointers, no workspace and no stream.  It checks the seeds
 *   and the pick counts before it writes anything, for every k.
 * Both fail with -1 and a message that names the entry point, before any launch and before any array is read, for a NULL
 *   csr, an invalid csr, an id width other than 32 / 64, a NULL weight, an unsupported weight dtype, NULL seeds or
 *   outputs, k < -1 and a workspace that is too small. */
#define DGLA_TOPK_I32 4
#define DGLA_TOPK_I64 5
int dgla_select_topk_max_picks(void);
size_t dgla_select_topk_workspace_bytes(int idtype_bits, int64_t num_seeds);
int dgla_select_topk(const dgla_csr* csr, const void* weight, int weight_dtype, const void* seeds, int64_t num_seeds,
                     int64_t k, int ascending, void* out_indptr, void* out_nbr, void* out_eids, void* workspace,
                     size_t workspace_bytes, void* hip_stream);
int dgla_select_topk_host(const dgla_csr* csr, const void* weight, int weight_dtype, const void* seeds, int64_t num_seeds,
                          int64_t k, int ascending, void* out_indptr, void* out_nbr, void* out_eids);

/* ---- PinSAGE neighbour selection: visit-count top-k over walk traces (csrc/pinsage.hip) -----------
 * Replace SelectPinSageNeighbors<kDGLCUDA> (src/graph/sampling/randomwalks/randomwalk_gpu.cu:443 over
 * frequency_hashmap.cu, behind python/dgl/sampling/pinsage.py).  The reference's GPU form fills a global hash table with
 * atomic inserts and leaves ties between equal visit counts in a run-dependent order; here a segment is selected in LDS
 * by one workgroup, without atomics, and the result is the one of the reference's CPU form (randomwalk_cpu.cc:41-102).
 * The rule (ONE statement for device and host):
 *
 * Inputs are src[num_dst * S] and dst[num_dst * S], both int32 or both int64; S = num_samples_per_node >= 1, k >= 1.
 * For segment j take the multiset of src[j*S .. (j+1)*S) with its -1 entries removed.  Rank its distinct ids by
 * (count descending, id descending) and keep the first min(k, number of distinct ids).  For each kept id emit
 * (id, dst[j*S], count) with the count in the id dtype; the segments follow each other in the order of j.
 * Ids cover the full non-negative range of the dtype (an id is never packed into a narrower key); ids are compared as
 * unsigned words, so an id below -1 is outside the contract but ranks the same way on the device and on the host.
 *
 * dgla_pinsage_max_samples: the largest S the kernel accepts (the segment lives in LDS): 4096 for both id widths, 0
 *   for another width.  A larger S is refused with a message before any launch; there is no CPU fallback.
 * dgla_pinsage_size_classes: the largest S of each size class, ascending (one wavefront per segment / a 256-thread
 *   workgroup / a 512-thread workgroup); returns their number.
 * dgla_pinsage_select_padded: the static-shape result.  With k' = min(k, S): out_src and out_cnt are [num_dst, k'] in
 *   the id dtype with the kept (id, count) pairs of segment j in rank order and -1 / 0 in the unused slots; out_num
 *   [num_dst] is the number kept; out_dst (may be NULL, then dst may be NULL) [num_dst] receives dst[j*S], the one
 *   read of dst per segment.  No workspace, no allocation, nothing read back, no synchronisation.
 * dgla_pinsage_select_count / _fill: the compact result around one workspace of
 *   dgla_pinsage_select_workspace_bytes bytes (it holds the padded result: proportional to num_dst * k', not to
 *   num_dst * S).  `count` selects, scans the kept numbers and returns their total in *total_out — the one host
 *   synchronisation, which the reference pays too; `fill` then writes res_src / res_dst / res_cnt [total] allocated by
 *   the caller, from the same workspace on the same stream.
 * dgla_pinsage_select_host: the rule run by the CPU on HOST pointers, no stream and no workspace; res_* must hold
 *   num_dst * k' entries, *total_out receives the number written.  Host-only: needs no GPU, accepts any S.
 * All fail with -1 and a message for an id width other than 32 / 64, S < 1, k < 1, num_dst < 0 and (device forms)
 * S above the limit or a workspace that is too small.  num_dst == 0 is valid. */
int64_t dgla_pinsage_max_samples(int idtype_bits);
int dgla_pinsage_size_classes(int64_t* bounds, int max);
int dgla_pinsage_select_padded(int idtype_bits, const void* src, const void* dst, int64_t num_dst,
                               int64_t num_samples_per_node, int64_t k, void* out_src, void* out_cnt, void* out_num,
                               void* out_dst, void* hip_stream);
size_t dgla_pinsage_select_workspace_bytes(int idtype_bits, int64_t num_dst, int64_t num_samples_per_node, int64_t k);
int dgla_pinsage_select_count(int idtype_bits, const void* src, const void* dst, int64_t num_dst,
                              int64_t num_samples_per_node, int64_t k, int64_t* total_out, void* workspace,
                              size_t workspace_bytes, void* hip_stream);
int dgla_pinsage_select_fill(int idtype_bits, int64_t num_dst, int64_t num_samples_per_node, int64_t k, void* res_src,
                             void* res_dst, void* res_cnt, const void* workspace, size_t workspace_bytes,
                             void* hip_stream);
int dgla_pinsage_select_host(int idtype_bits, const void* src, const void* dst, int64_t num_dst,
                             int64_t num_samples_per_node, int64_t k, void* res_src, void* res_dst, void* res_cnt,
                             int64_t* total_out);

/* ---- k-way node-cut partitioner (host code) ---------------------------------
 * Stands where METIS stands in the reference: metis_partition_assignment
 * (python/dgl/partition.py:278-397 -> _CAPI_DGLMetisPartition_Hetero).  Multilevel
 * size-constrained label propagation (csrc/partition.cc).  The CSR (HOST pointers, rows =
 * destination nodes, square) is symmetrised internally like the reference does.
 *   imbalance      allowed excess of a part's weight over the average, e.g. 0.03
 *   balance_edges  vertex weight = 1 + in-degree instead of 1 (the reference's flag)
 *   out_part       [num_nodes] int64, the part of every node
 *   stats          optional [4]: cut edges, heaviest part weight, average part weight, levels */
int dgla_partition_kway(int idtype_bits, int64_t num_nodes, const void* indptr,
                        const void* indices, int num_parts, double imbalance, int balance_edges,
                        uint64_t seed, int64_t* out_part, int64_t* stats);
/* The reference's other METIS options (python/dgl/partition.py:278-397 -> src/graph/metis_partition.cc:60-90):
 *   objtype     0 = "cut" (edge cut), 1 = "vol" (total communication volume: the number of distinct remote
 *               columns the parts read = the rows a row-sharded SpMM exchanges per step);
 *   ntype       (may be NULL) node type of every node, values in [0, num_ntypes): balance_ntypes — every node
 *               type is balanced across the parts by its own constraint;
 *   init_part   (may be NULL) an assignment to REFINE instead of running the multilevel scheme (e.g. contiguous
 *               ranges of a graph whose vertex order already reflects its structure).
 * Refinement under either objective is a greedy k-way pass over the directed CSR with exact gains from a
 * per-(column, part) reference-count table.  stats8 = {cut edges, heaviest part, average part, levels, total
 * volume, largest halo (distinct remote columns of one part), largest (part, type) excess over its limit,
 * refinement moves}. */
int dgla_partition_kway_ex(int idtype_bits, int64_t num_nodes, const void* indptr, const void* indices,
                           int num_parts, double imbalance, int balance_edges, uint64_t seed, int objtype,
                           int num_ntypes, const int32_t* ntype, const int64_t* init_part, int64_t* out_part,
                           int64_t* stats8);

/* ---- multi-GPU exchange step -----------------------------------------
 * Device side of the halo all-to-all: the collective itself is RCCL (torch.distributed), these
 * are the pack / unpack kernels around it and the NDArrayPartition index maps.
 *
 * dgla_gather_rows: dst[i, :] = src[idx[i], :], rows of `row_bytes` bytes — `value[perm]`,
 *   `value[resp_idx]` in python/dgl/cuda/nccl.py:69-70,176 (torch index kernels there); the
 *   scatter-add direction of the gradient push is dgla_scatter_add above.
 * dgla_partition_map / dgla_partition_to_global: MapToLocalFromRemainder / ...FromRange and
 *   MapToGlobal... of src/partition/cuda/partition_op.cu (declared src/partition/partition_op.h:
 *   36-130; objects src/partition/ndarray_partition.cc:30-230).
 *   mode 0 = remainder: part = id % num_parts, local = id / num_parts
 *   mode 1 = range:     part = the p with range[p] <= id < range[p + 1], local = id - range[p];
 *                       `range` = DEVICE array of num_parts + 1 ids (idtype_bits), as the
 *                       reference requires (ndarray_partition.cc:104-112)
 *   part_out / local_out may be NULL.  GeneratePermutation = dgla_partition_map (parts) +
 *   dgla_coo_to_csr over the part ids (a stable sort: eids_out is the permutation, indptr the
 *   prefix of the per-part counts). */
int dgla_gather_rows(int idtype_bits, const void* src, const void* idx, int64_t n,
                     int64_t row_bytes, void* dst, void* hip_stream);
/* dst[idx[i], :] = src[i, :] (idx a permutation, or at least injective). */
int dgla_scatter_rows(int idtype_bits, const void* src, const void* idx, int64_t n,
                      int64_t row_bytes, void* dst, void* hip_stream);

int dgla_partition_map(int idtype_bits, int mode, int num_parts, const void* range, const void* idx,
                       int64_t n, void* part_out, void* local_out, void* hip_stream);
int dgla_partition_to_global(int idtype_bits, int mode, int num_parts, const void* range,
                             const void* local_idx, int64_t n, int part_id, void* out,
                             void* hip_stream);

/* ---- peer-mapped halo exchange (replaces the value exchange of sparse_all_to_all_pull,
 * python/dgl/cuda/nccl.py:98-183, when every GPU of the node can map every other GPU's memory) ----
 * dgla_peer_alloc: device memory that can be exported (kind 0 = hipMalloc, 1 = fine-grained, 2 = uncached;
 *   falls back to hipMalloc when the flavour is refused), zero filled.  dgla_ipc_export / _import / _release =
 *   hipIpcGetMemHandle / OpenMemHandle / CloseMemHandle on 64-byte handles.
 * dgla_peer_push: ONE launch writes rows serve_rows[seg.row_begin .. seg.row_end) of x_local into every
 *   segment's destination (a peer's halo buffer) and then stores `epoch` into the segment's flag in the peer's
 *   memory.  `segments` = DEVICE array of num_segments records {int64 row_begin, row_end; void* dst;
 *   uint64* flag; int64 blk_begin} with blk_begin = exclusive prefix of max(1, ceil(rows / 64)), num_blocks
 *   its total; `arrive` = num_segments zeroed uint32 counters in device memory (kept zero between calls).
 * dgla_peer_wait: one wavefront on the stream polls flags[0 .. num_flags) until each is >= epoch (bounded:
 *   after max_spins polls *status (device int) becomes 1 and the stream continues). */
int dgla_peer_alloc(size_t bytes, int kind, void** out);
int dgla_peer_free(void* ptr);
int dgla_ipc_export(void* ptr, void* handle64);
int dgla_ipc_import(const void* handle64, void** out);
int dgla_ipc_release(void* ptr);
int dgla_peer_push(const void* x_local, int64_t row_bytes, const int64_t* serve_rows, const void* segments,
                   int num_segments, int64_t num_blocks, uint64_t epoch, void* arrive, void* hip_stream);
int dgla_peer_wait(const void* flags, int num_flags, uint64_t epoch, void* status, int64_t max_spins,
                   void* hip_stream);

/* Process-wide tuning bits.  The SpMM bits change no result bit; they select memory-system behaviour
 * and exist so that a benchmark can A/B them:
 *   DGLA_TUNE_XCD     units visit the merge path in XCD-contiguous order (block b runs on XCD
 *                     b % 8, so each XCD's L2 sees one contiguous eighth of the rows)
 *   DGLA_TUNE_SPLIT   when a gathered ufeat row touches one 128-byte line more than its length needs
 *                     (F = 100 fp32: 400 B = 4 lines per gather) the call first copies the rows' ragged
 *                     ends (16-byte lanes, rows of >= 256 bytes: one side line per row + a dense array of
 *                     the last bytes; the line-aligned interior is gathered in place) or the straddling
 *                     rows (8-byte lanes, e.g. bf16 F = 100) into the workspace — unless the locality
 *                     probe made with the merge plan found at least 15/16 of the sampled edges within
 *                     64 Ki rows of their own row (the copy costs 0.1 ms on the headline graph and pays
 *                     even at 81 % local edges)
 *   DGLA_TUNE_SPLIT_FORCE  ignore the locality probe
 *   DGLA_TUNE_GLDS    dgla_segment_mm / dgla_gather_mm, 16-bit and fp32 storage, operands in
 *                     whole aligned 16-byte pieces: operands go global -> LDS directly (global_load_lds,
 *                     slab rings) instead of through registers; 16-bit results bit-identical,
 *                     fp32 contracts k in a permuted order; the 16-bit weight gradient reads
 *                     its fragments with transposing LDS loads (default on)
 *   DGLA_TUNE_MM_F32  dgla_segment_mm / dgla_gather_mm and their gradients, fp32: multiply on
 *                     v_mfma_f32_32x32x2_f32.  Default (bit off): every fp32 operand is split into
 *                     three round-to-nearest bf16 terms and the six products of order <= 2 run on
 *                     v_mfma_f32_32x32x16_bf16 with fp32 accumulation — fp32-level accuracy (dropped
 *                     terms < 2^-26 |a b|) at 2.7x less matrix-pipe time; gfx950 has no xf32 MFMA
 *   DGLA_TUNE_MM_X3   dgla_segment_mm / dgla_gather_mm forward, fp32, weights-stationary kernel (long inputs, K <= 256):
 *                     the three-bf16-term split above.  Default (bit off, round 5): TWO fp16 terms under exact per-row /
 *                     per-column power-of-two scales — three products (hh, hl, lh) instead of six, dropped term
 *                     < 2^-22 |a b|; a row whose non-zero magnitudes span more than 2^18, or whose maximum is not finite
 *                     or outside 2^+-60, is recomputed as the plain fp32 dot product inside the same launch
 *   DGLA_TUNE_NO_GATE dgla_spmm_csr_masked (max / min backward as a gather): gather every piece of every row.  Default (bit
 *                     off, round 6): the bit words are fetched one batch ahead and a lane whose columns are all off for an
 *                     edge reads a fixed cached address instead of its piece of the row — a 128-byte line of the gathered
 *                     operand is requested only when one of its columns is wanted.  Changes no result bit (A/B switch).
 *   DGLA_TUNE_NO_STAGE_W  dgla_spmm_csr with ONE 4-byte edge weight per edge and the sum reducer (u_mul_e / u_add_e + sum): read the
 *                     weight from global memory in every gather batch.  Default (bit off, round 6): the unit's weights are
 *                     staged in LDS together with its column ids (one load per edge).  Changes no result bit (A/B switch).
 * Removed in round 4 (values retired, dgla_set_tuning rejects them): NT_OUT 2 and NT_IDX 4 (non-temporal
 * output-row stores / index-stream loads: measured neutral), SPLIT_NT 32, SPLIT_CLASSIC 256
 * (whole-row copy: 0.33 ms against 0.10), TAIL_PASS 512 (column-sliced pass over the 16-byte row tails:
 * -5 % .. +3.5 %), NT_STREAM 1024 (now a fixed rule: copy_rhs without an edge-id map over rows of >= 64
 * edges on average loads the edge operand non-temporally; measured 1.10 -> 1.01 ms on a 64-segment sum,
 * +7 .. 10 % on short rows, hence the rule).  The reference has no counterpart (its kernels take no hints). */
#define DGLA_TUNE_XCD 1u
#define DGLA_TUNE_SPLIT 8u
#define DGLA_TUNE_GLDS 16u
#define DGLA_TUNE_SPLIT_FORCE 64u
#define DGLA_TUNE_MM_F32 128u
#define DGLA_TUNE_MM_X3 2048u
#define DGLA_TUNE_NO_GATE 4096u
#define DGLA_TUNE_NO_STAGE_W 8192u
int dgla_set_tuning(uint32_t flags);
uint32_t dgla_get_tuning(void);

/* dgla_spmm_csr / dgla_segment_reduce calls of this process served by the narrow-feature kernels (csrc/narrow_reduce.hip:
 * 1 ... 8 fp32 output columns — copy_rhs, copy_lhs, u (+ - * /) e —, one lane per four EDGES instead of one lane per column; same results as the
 * merge kernel up to the order of fp32 additions, winners and their edge ids identical).  A counter for tests and
 * benches to see which kernel family took a call; DGLA_NARROW_REDUCE=0 in the environment keeps the merge kernel.
 * (DGLA_NARROW_STAGE=0: edge rows of 4 / 8 columns in position order are gathered lane by lane instead of being fetched as
 * whole wavefront loads and transposed through LDS — an A/B switch, same bits either way.)
 * The reference has one kernel for every width (src/array/cuda/spmm.cuh:440-520). */
int64_t dgla_narrow_reduce_calls(void);

/* Benchmark hook: when both are non-NULL (hipEvent_t), the calling thread's next
 * dgla_spmm_csr calls record `before` / `after` on the launch stream around the dominant
 * (merge) kernel only, so its duration can be read with hipEventElapsedTime.  NULL disables. */
int dgla_spmm_set_profile_events(void* before, void* after);

/* Measured-peak helper used by bench.py: streams `bytes` from src to dst with 16-byte
 * lane accesses (the "float4 copy" the HBM roofline is quoted against). */
int dgla_stream_copy(void* dst, const void* src, size_t bytes, void* hip_stream);
/* Same with an explicit kernel variant (benchmarks/bench_peak.py): bits 0-1 = 0 copy with
 * non-temporal accesses, 1 copy with default cache policy, 2 read-only (dst receives one
 * 16-byte value per lane of the grid: needs >= 32 MiB); bits 2-3 = log2(blocks per CU) - 2;
 * bit 4 = 8 instead of 4 loads in flight per lane. */
int dgla_stream_copy_variant(void* dst, const void* src, size_t bytes, int variant,
                             void* hip_stream);

/* ======================================================================================
 * (2) Registry layer — same names and layouts as include/dgl/runtime/c_runtime_api.h.
 * ====================================================================================== */

/* type codes (c_runtime_api.h:66-91) */
typedef enum {
  kObjectInt = 0,
  kObjectUInt = 1,
  kObjectFloat = 2,
  kHandle = 3,
  kNull = 4,
  kDGLDataType = 5,
  kDGLContext = 6,
  kArrayHandle = 7,
  kObjectHandle = 8,
  kModuleHandle = 9,
  kFuncHandle = 10,
  kStr = 11,
  kBytes = 12,
  kNDArrayContainer = 13
} DGLTypeCode;

/* Device types.  kDGLROCM = 10 is DLPack's kDLROCM, which PyTorch-ROCm exports; the
 * reference only knows kDGLCPU = 1 / kDGLCUDA = 2 (c_runtime_api.h:51-60). */
typedef enum { kDGLCPU = 1, kDGLCUDA = 2, kDGLROCM = 10 } DGLDeviceType;

typedef struct {
  int32_t device_type;
  int32_t device_id;
} DGLContext;

typedef struct {
  uint8_t code; /* 0 int, 1 uint, 2 float, 4 bfloat (DLPack codes) */
  uint8_t bits;
  uint16_t lanes;
} DGLDataType;

/* DGLValue (c_runtime_api.h:205-212) */
typedef union {
  int64_t v_int64;
  double v_float64;
  void* v_handle;
  const char* v_str;
  DGLDataType v_type;
  DGLContext v_ctx;
} DGLValue;

/* DGLArray (c_runtime_api.h:150-196): DLTensor-compatible. */
typedef struct {
  void* data;
  DGLContext ctx;
  int32_t ndim;
  DGLDataType dtype;
  int64_t* shape;
  int64_t* strides; /* NULL = compact row-major */
  uint64_t byte_offset;
} DGLArray;

typedef void* DGLFunctionHandle;
typedef DGLArray* DGLArrayHandle;

const char* DGLGetLastError(void);
void DGLAPISetLastError(const char* msg);
int DGLFuncListGlobalNames(int* out_size, const char*** out_array);
int DGLFuncGetGlobal(const char* name, DGLFunctionHandle* out);
int DGLFuncCall(DGLFunctionHandle func, DGLValue* args, int* type_codes, int num_args,
                DGLValue* ret_val, int* ret_type_code);
int DGLFuncFree(DGLFunctionHandle func);

/* DLPack hand-over (include/dgl/runtime/dlpack_convert.h:60-80, src/runtime/dlpack_convert.cc:
 * 57-140; the reference's Python wraps every tensor this way, backend/pytorch/tensor.py:432-435).
 * DGLArrayFromDLPack takes ownership of `from` (its deleter runs when the array is freed) and
 * returns a handle that points at a DGLArray — the first member of the array's container, as
 * with NDArray::Container.  device_type travels unchanged: PyTorch-ROCm exports kDLROCM = 10 =
 * kDGLROCM.  DGLArrayToDLPack shares the memory and keeps the array alive until the consumer
 * calls the returned tensor's deleter. */
#ifndef DLPACK_DLPACK_H_
typedef struct {
  int32_t device_type;
  int32_t device_id;
} DLDevice;
typedef struct {
  uint8_t code;
  uint8_t bits;
  uint16_t lanes;
} DLDataType;
typedef struct {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
} DLTensor;
typedef struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(struct DLManagedTensor* self);
} DLManagedTensor;
#endif
int DGLArrayFromDLPack(DLManagedTensor* from, void** out /* DGLArrayHandle* */);
int DGLArrayToDLPack(void* from /* DGLArrayHandle */, DLManagedTensor** out, int alignment);
int DGLArrayFree(void* handle /* DGLArrayHandle made by DGLArrayFromDLPack */);
void DGLDLManagedTensorCallDeleter(DLManagedTensor* dltensor);
/* include/dgl/runtime/c_object_api.h: DGLObjectFree — releases an object handle returned by a
 * registry function: the List<Value> / Value boxes of the global functions `_List` / `_Value`
 * (how the reference passes Python lists, python/dgl/_ffi/object_generic.py:27-59), the
 * heterograph handle of dgl_amd._CAPI_HeteroGraphCreate, a unit-graph handle. */
int DGLObjectFree(void* handle);
/* c_runtime_api.h: DGLSetStream — the stream kernels of this thread are queued on. */
int DGLSetStream(int device_type, int device_id, void* stream);
int DGLGetStream(int device_type, int device_id, void** stream);

#ifdef __cplusplus
}
#endif
#endif /* DGL_AMD_H_ */
