"""Torch-tensor front end of the graph-free C seam (include/dgl_amd.h, `dgla_*`).

Everything here is plumbing: it turns torch tensors into (pointer, shape) pairs, picks the
current HIP stream (reference: kernels are queued on the current PyTorch stream,
tests/python/pytorch/test_ffi-stream.py:45-64) and calls the shared library.  No arithmetic
happens in Python.
"""
import ctypes

import torch

from . import _lib
from ._lib import COO, CSR, LIB, Tensor, check_call

_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
TARGETS = {"u": 0, "e": 1, "v": 2}


def _require_gpu(t):
    if not t.is_cuda:
        raise _lib.DGLAMDError(
            "dgl_amd kernels run on a ROCm GPU; got a tensor on %s (no CPU fallback)" % t.device)


def _tensor(t, keep):
    """dgla_tensor for a contiguous torch tensor (1-D is viewed as (n, 1), the reference's
    unsqueeze in python/dgl/_sparse_ops.py:208-217)."""
    if t is None:
        return Tensor(None, 0, None)
    if type(t) is not torch.Tensor:
        from .edge_order import reject_tagged
        reject_tagged(t)
    _require_gpu(t)
    if not t.is_contiguous():
        raise _lib.DGLAMDError("feature tensors must be contiguous")
    shape = tuple(t.shape) if t.dim() > 1 else (t.shape[0], 1)
    arr = (ctypes.c_int64 * len(shape))(*shape)
    keep.append(arr)
    return Tensor(t.data_ptr(), len(shape), arr)


def _idbits(t):
    if t.dtype == torch.int32:
        return 32
    if t.dtype == torch.int64:
        return 64
    raise _lib.DGLAMDError("index tensors must be int32 or int64")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(workspace):
    """(pointer, bytes) of an optional workspace.  Workspaces are uint8 tensors, so numel() is already the byte count;
    the product with element_size() only keeps a caller's tensor of another dtype honest."""
    return _ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size()


def _id_bits(idtype):
    """The id width of a torch id dtype, for the size queries that take no tensor."""
    return 32 if idtype == torch.int32 else 64


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _u64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF   # (negative seeds wrap)


def _workspace(need, device):
    return torch.empty(need, dtype=torch.uint8, device=device) if need else None   # (None: the call needs none)


def _all_on(gpu, who, *tensors):
    """The device twin of an entry point takes GPU tensors, the host twin `who` CPU tensors; None entries are skipped."""
    for t in tensors:
        if t is None:
            continue
        if gpu:
            _require_gpu(t)
        elif t.is_cuda:
            raise _lib.DGLAMDError("%s takes CPU tensors" % who)


def _prob_ok(prob):
    if prob.dtype not in (torch.float32, torch.float64) or prob.dim() != 1 or not prob.is_contiguous():
        raise _lib.DGLAMDError("prob must be a contiguous 1-D float32 / float64 tensor")


def _member_ok(csr, member):
    if member is None or _idbits(member) != csr.idtype_bits or member.numel() != csr.nnz or not member.is_contiguous():
        raise _lib.DGLAMDError("member must be a contiguous tensor of the csr's id type with one entry per edge")


def make_csr(indptr, indices, eids, num_cols):
    _require_gpu(indptr)
    c = CSR(indptr.shape[0] - 1, int(num_cols), indices.shape[0], _idbits(indptr),
            indptr.data_ptr(), _ptr(indices), _ptr(eids))
    c._keep = (indptr, indices, eids)  # the struct borrows the pointers: keep the tensors alive with it
    return c


def make_coo(row, col, eids, num_src, num_dst):
    _require_gpu(row)
    c = COO(int(num_src), int(num_dst), row.shape[0], _idbits(row), _ptr(row), _ptr(col), _ptr(eids))
    c._keep = (row, col, eids)
    return c


def spmm_csr_workspace_bytes(op, reduce, csr, dtype, ufeat, efeat, out):
    keep = []
    tu, te, to = _tensor(ufeat, keep), _tensor(efeat, keep), _tensor(out, keep)
    return LIB.dgla_spmm_csr_workspace_bytes(op.encode(), reduce.encode(), ctypes.byref(csr),
                                             _DTYPES[dtype], ctypes.byref(tu), ctypes.byref(te),
                                             ctypes.byref(to))


def spmm_csr(op, reduce, csr, ufeat, efeat, out, arg_u=None, arg_e=None, workspace=None,
             accumulate=False, plan_valid=False, mean=False, split_keep=False, split_valid=False,
             prepare_only=False):
    """out = g-SpMM over `csr` (rows = destination nodes).  `workspace` is a uint8 tensor of
    at least spmm_csr_workspace_bytes(); it also caches the merge plan between calls.
    `split_keep`: `ufeat` is static (the caller will pass the same unchanged tensor again), so
    the split-row copy is made whatever the locality probe says; `split_valid`: the workspace
    still holds that copy of this very `ufeat` — only for callers that own the tensor;
    `prepare_only` (with `split_keep`): plan + side copy only, for the PRODUCER of `ufeat`."""
    keep = []
    tu, te, to = _tensor(ufeat, keep), _tensor(efeat, keep), _tensor(out, keep)
    flags = (_lib.DGLA_ACCUMULATE if accumulate else 0) | (_lib.DGLA_PLAN_VALID if plan_valid else 0) | \
        (_lib.DGLA_MEAN if mean else 0) | (_lib.DGLA_SPLIT_VALID if split_valid else 0) | \
        (_lib.DGLA_SPLIT_KEEP if split_keep else 0) | (_lib.DGLA_PREPARE_ONLY if prepare_only else 0)
    check_call(LIB.dgla_spmm_csr(
        op.encode(), reduce.encode(), ctypes.byref(csr), _DTYPES[out.dtype], ctypes.byref(tu),
        ctypes.byref(te), ctypes.byref(to), _ptr(arg_u), _ptr(arg_e), *_ws(workspace), flags,
        _stream(out)))


def pointer_table(tensors, device):
    """Device array of the tensors' data pointers (int64), as dgla_spmm_csr_stacked wants."""
    return torch.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch.int64,
                        device=device)


def spmm_csr_stacked_workspace_bytes(op, csr, ufeat0, efeat0, out):
    keep = []
    tu, te, to = _tensor(ufeat0, keep), _tensor(efeat0, keep), _tensor(out, keep)
    return LIB.dgla_spmm_csr_stacked_workspace_bytes(op.encode(), ctypes.byref(csr),
                                                     _DTYPES[out.dtype], ctypes.byref(tu),
                                                     ctypes.byref(te), ctypes.byref(to))


def spmm_csr_stacked(op, csr, rel, ufeats, efeats, out, workspace, u_table=None, e_table=None,
                     accumulate=False, plan_valid=False):
    """Fused sum over several relations (SpMMCsrHetero in one launch).  `csr` is the stacked
    matrix, `rel` the uint8 relation id per stacked edge, `ufeats` / `efeats` lists with one
    tensor per relation (or None when the operator does not read that side)."""
    keep = []
    u0 = None if ufeats is None else ufeats[0]
    e0 = None if efeats is None else efeats[0]
    tu, te, to = _tensor(u0, keep), _tensor(e0, keep), _tensor(out, keep)
    if u_table is None and ufeats is not None:
        u_table = pointer_table(ufeats, out.device)
    if e_table is None and efeats is not None:
        e_table = pointer_table(efeats, out.device)
    n_rel = len(ufeats if ufeats is not None else efeats)
    flags = (_lib.DGLA_ACCUMULATE if accumulate else 0) | (_lib.DGLA_PLAN_VALID if plan_valid else 0)
    check_call(LIB.dgla_spmm_csr_stacked(
        op.encode(), ctypes.byref(csr), rel.data_ptr(), n_rel, _DTYPES[out.dtype], ctypes.byref(tu),
        ctypes.byref(te), _ptr(u_table), _ptr(e_table), ctypes.byref(to), *_ws(workspace), flags,
        _stream(out)))
    return u_table, e_table


def spmm_coo(op, reduce, coo, ufeat, efeat, out, arg_u=None, arg_e=None):
    keep = []
    tu, te, to = _tensor(ufeat, keep), _tensor(efeat, keep), _tensor(out, keep)
    check_call(LIB.dgla_spmm_coo(op.encode(), reduce.encode(), ctypes.byref(coo),
                                 _DTYPES[out.dtype], ctypes.byref(tu), ctypes.byref(te),
                                 ctypes.byref(to), _ptr(arg_u), _ptr(arg_e), _stream(out)))


def sddmm_coo(op, coo, lhs, rhs, out, lhs_target, rhs_target):
    keep = []
    tl, tr, to = _tensor(lhs, keep), _tensor(rhs, keep), _tensor(out, keep)
    check_call(LIB.dgla_sddmm_coo(op.encode(), ctypes.byref(coo), _DTYPES[out.dtype],
                                  ctypes.byref(tl), ctypes.byref(tr), ctypes.byref(to),
                                  lhs_target, rhs_target, _stream(out)))


def sddmm_csr(op, csr, lhs, rhs, out, lhs_target, rhs_target):
    keep = []
    tl, tr, to = _tensor(lhs, keep), _tensor(rhs, keep), _tensor(out, keep)
    check_call(LIB.dgla_sddmm_csr(op.encode(), ctypes.byref(csr), _DTYPES[out.dtype],
                                  ctypes.byref(tl), ctypes.byref(tr), ctypes.byref(to),
                                  lhs_target, rhs_target, _stream(out)))


def edge_softmax_workspace_bytes(csr, dtype, dim):
    return LIB.dgla_edge_softmax_workspace_bytes(ctypes.byref(csr), _DTYPES[dtype], int(dim))


def _ws_args(workspace, plan_valid):
    return (*_ws(workspace), _lib.DGLA_PLAN_VALID if plan_valid else 0)


def edge_softmax_forward(csr, score, out, workspace=None, plan_valid=False, out_position=False):
    """`workspace` (uint8 tensor of edge_softmax_workspace_bytes) selects the degree-balanced
    merge-path kernels; None runs the scratch-free lane-group kernel.  `out_position` (merge-path only):
    scores are read through the CSR's edge-id map, `out` is written in position order
    (DGLA_ESM_OUT_POSITION)."""
    keep = []
    ts, to = _tensor(score, keep), _tensor(out, keep)
    wp, wn, fl = _ws_args(workspace, plan_valid)
    if out_position:
        fl |= _lib.DGLA_ESM_OUT_POSITION
    check_call(LIB.dgla_edge_softmax_forward(ctypes.byref(csr), _DTYPES[out.dtype],
                                             ctypes.byref(ts), ctypes.byref(to), wp, wn, fl, _stream(out)))


def edge_softmax_backward(csr, out, sds, back, workspace=None, plan_valid=False, sds_is_grad=False,
                          out_position=False):
    """`sds_is_grad` (merge-path kernels only): `sds` is the upstream gradient itself, the product with `out` is
    formed inside the kernel (DGLA_ESM_B_IS_GRAD).  `out_position` (merge-path only): `out` is read and `back` written
    in the CSR's position order, `sds` is read through the edge-id map (DGLA_ESM_OUT_POSITION)."""
    keep = []
    to, ts, tb = _tensor(out, keep), _tensor(sds, keep), _tensor(back, keep)
    wp, wn, fl = _ws_args(workspace, plan_valid)
    if sds_is_grad:
        fl |= _lib.DGLA_ESM_B_IS_GRAD
    if out_position:
        fl |= _lib.DGLA_ESM_OUT_POSITION
    check_call(LIB.dgla_edge_softmax_backward(ctypes.byref(csr), _DTYPES[out.dtype],
                                              ctypes.byref(to), ctypes.byref(ts),
                                              ctypes.byref(tb), wp, wn, fl, _stream(back)))


def gat_attention_supported(dtype, heads, dim):
    """Whether the one-pass GAT attention kernels take (dtype, H, D) (dgla_gat_attention_supported; needs no GPU)."""
    code = _DTYPES.get(dtype)
    return code is not None and bool(LIB.dgla_gat_attention_supported(code, int(heads), int(dim)))


def _gat_same_dtype(ft, *others):
    for t in others:
        if t.dtype != ft.dtype:
            raise _lib.DGLAMDError("gat_attention: every tensor carries the operands' dtype (%s), got %s" % (ft.dtype, t.dtype))


def gat_attention_workspace_bytes(csc, heads, dim):
    return int(LIB.dgla_gat_attention_workspace_bytes(ctypes.byref(csc), int(heads), int(dim)))


def gat_attention_forward(csc, ft, el, er, slope, out, mz, workspace):
    """out[v] = sum_u softmax_v(leaky_relu(el[u] + er[v])) ft[u] per head in one pass (dgla_gat_attention_forward);
    `mz` (N_dst, H, 2) fp32 receives each row's softmax maximum and normaliser for the backward."""
    keep = []
    _gat_same_dtype(ft, el, er, out)
    tf, tl, tr, to = (_tensor(t, keep) for t in (ft, el, er, out))
    _require_gpu(mz)
    if mz.dtype != torch.float32:
        raise _lib.DGLAMDError("gat_attention: mz is fp32 whatever the operands' dtype")
    check_call(LIB.dgla_gat_attention_forward(ctypes.byref(csc), _DTYPES[ft.dtype], ctypes.byref(tf), ctypes.byref(tl),
                                              ctypes.byref(tr), float(slope), ctypes.byref(to), mz.data_ptr(),
                                              *_ws(workspace),
                                              _stream(out)))


def gat_attention_backward(csc, csr, ft, el, er, out, mz, dout, slope, d_ft, d_el, d_er, workspace):
    """Gradients of dgla_gat_attention_forward; `csr` = the out-edge CSR (rows = source nodes) of the same graph."""
    keep = []
    _gat_same_dtype(ft, el, er, out, dout, d_ft, d_el, d_er)
    ts = [_tensor(t, keep) for t in (ft, el, er, out, dout, d_ft, d_el, d_er)]
    check_call(LIB.dgla_gat_attention_backward(ctypes.byref(csc), ctypes.byref(csr), _DTYPES[ft.dtype],
                                               ctypes.byref(ts[0]), ctypes.byref(ts[1]), ctypes.byref(ts[2]),
                                               ctypes.byref(ts[3]), mz.data_ptr(), ctypes.byref(ts[4]), float(slope),
                                               ctypes.byref(ts[5]), ctypes.byref(ts[6]), ctypes.byref(ts[7]),
                                               *_ws(workspace),
                                               _stream(d_ft)))


def gat_attention_train_forward(csc, ft, el, er, slope, p, seed, out, mz, workspace):
    """dgla_gat_attention_train_forward: the forward above with dropout of probability `p` on the attention weights,
    the mask a function of (seed, edge id, head) that is never stored; `mz` is the (max, normaliser) of the softmax
    WITHOUT dropout, as gat_attention_forward writes it."""
    keep = []
    _gat_same_dtype(ft, el, er, out)
    tf, tl, tr, to = (_tensor(t, keep) for t in (ft, el, er, out))
    _require_gpu(mz)
    if mz.dtype != torch.float32:
        raise _lib.DGLAMDError("gat_attention: mz is fp32 whatever the operands' dtype")
    check_call(LIB.dgla_gat_attention_train_forward(ctypes.byref(csc), _DTYPES[ft.dtype], ctypes.byref(tf), ctypes.byref(tl),
                                                    ctypes.byref(tr), float(slope), float(p), int(seed), ctypes.byref(to),
                                                    mz.data_ptr(), *_ws(workspace), _stream(out)))


def gat_attention_train_backward(csc, csr, ft, el, er, mz, dout, slope, p, seed, d_ft, d_el, d_er, workspace):
    """Gradients of dgla_gat_attention_train_forward for the same (p, seed): the mask is evaluated again, from the
    edge-id map of each CSR."""
    keep = []
    _gat_same_dtype(ft, el, er, dout, d_ft, d_el, d_er)
    ts = [_tensor(t, keep) for t in (ft, el, er, dout, d_ft, d_el, d_er)]
    check_call(LIB.dgla_gat_attention_train_backward(ctypes.byref(csc), ctypes.byref(csr), _DTYPES[ft.dtype],
                                                     ctypes.byref(ts[0]), ctypes.byref(ts[1]), ctypes.byref(ts[2]),
                                                     mz.data_ptr(), ctypes.byref(ts[3]), float(slope), float(p), int(seed),
                                                     ctypes.byref(ts[4]), ctypes.byref(ts[5]), ctypes.byref(ts[6]),
                                                     *_ws(workspace),
                                                     _stream(d_ft)))


def gat_attention_weights(csc, el, er, mz, slope, p, seed, attn):
    """attn[eid, h] = the post-dropout attention weight of every edge, (E, H, 1) in edge-id order, from the `mz` of a
    forward on the same operands (dgla_gat_attention_weights)."""
    keep = []
    _gat_same_dtype(el, er, attn)
    tl, tr, ta = (_tensor(t, keep) for t in (el, er, attn))
    check_call(LIB.dgla_gat_attention_weights(ctypes.byref(csc), _DTYPES[el.dtype], ctypes.byref(tl), ctypes.byref(tr),
                                              mz.data_ptr(), float(slope), float(p), int(seed), ctypes.byref(ta),
                                              _stream(attn)))


def gat_dropout_mask_host(seed, p, eids, heads):
    """The keep mask of attention dropout for edge ids `eids` (a CPU int64 tensor) as a (len(eids), heads) uint8 CPU
    tensor — the same gat_keep the kernels evaluate (dgla_gat_dropout_mask_host; needs no GPU)."""
    eids = eids.to(device="cpu", dtype=torch.int64).contiguous()
    keep = torch.empty((eids.numel(), int(heads)), dtype=torch.uint8)
    check_call(LIB.dgla_gat_dropout_mask_host(int(seed), float(p), eids.data_ptr(), eids.numel(), int(heads),
                                              keep.data_ptr()))
    return keep


def stream_copy(dst, src):
    _require_gpu(dst)
    check_call(LIB.dgla_stream_copy(dst.data_ptr(), src.data_ptr(),
                                    src.numel() * src.element_size(), _stream(dst)))


def stream_copy_variant(dst, src, variant):
    _require_gpu(dst)
    check_call(LIB.dgla_stream_copy_variant(dst.data_ptr(), src.data_ptr(),
                                            src.numel() * src.element_size(), int(variant),
                                            _stream(dst)))


def set_profile_events(before, after):
    """Record two torch.cuda.Event objects around the merge kernel of the next spmm_csr calls
    of this thread (None, None disables).  The events must have been recorded once already so
    that their HIP handles exist."""
    if before is None or after is None:
        LIB.dgla_spmm_set_profile_events(None, None)
    else:
        LIB.dgla_spmm_set_profile_events(before.cuda_event, after.cuda_event)


(TUNE_XCD, TUNE_SPLIT, TUNE_GLDS, TUNE_SPLIT_FORCE, TUNE_MM_F32, TUNE_MM_X3, TUNE_NO_GATE, TUNE_NO_STAGE_W) = (1, 8, 16, 64, 128, 2048, 4096, 8192)  # include/dgl_amd.h DGLA_TUNE_*


def set_tuning(flags):
    """Process-wide tuning bits (include/dgl_amd.h: DGLA_TUNE_*).  The SpMM bits XCD, SPLIT*
    never change result bits (SPLIT changes the workspace layout: plans do not survive a change of
    it).  The matrix-multiply bits do change bits: DGLA_TUNE_GLDS contracts fp32 k in a
    permuted order and DGLA_TUNE_MM_F32 selects the exact fp32 MFMA instead of the default
    split-operand kernels (same fp32-level error bound, different low-order bits); DGLA_TUNE_MM_X3 keeps the
    weights-stationary fp32 forward on three bf16 terms instead of two scaled fp16 terms."""
    check_call(LIB.dgla_set_tuning(int(flags)))
    from . import sparse_kernels
    sparse_kernels._tuning_epoch[0] = int(flags)  # scratch sizes remembered per relation depend on the bits


def get_tuning():
    return int(LIB.dgla_get_tuning())


def narrow_reduce_calls():
    """dgla_spmm_csr calls served by the narrow-feature copy_e kernels so far (dgla_narrow_reduce_calls)."""
    return int(LIB.dgla_narrow_reduce_calls())


def segment_reduce(reduce, feat, offsets, out, arg=None, workspace=None, plan_valid=False):
    """out[i] = reduce(feat[offsets[i]:offsets[i+1]]) (dgla_segment_reduce).  `workspace` may
    be None (stream-ordered scratch inside the call) or a uint8 tensor of
    segment_reduce_workspace_bytes() that also caches the merge plan of `offsets`."""
    keep = []
    tf, to = _tensor(feat, keep), _tensor(out, keep)
    _require_gpu(offsets)
    check_call(LIB.dgla_segment_reduce(
        reduce.encode(), _idbits(offsets), _DTYPES[out.dtype], ctypes.byref(tf),
        offsets.data_ptr(), offsets.shape[0] - 1, ctypes.byref(to), _ptr(arg), *_ws(workspace),
        _lib.DGLA_PLAN_VALID if plan_valid else 0, _stream(out)))


def segment_reduce_workspace_bytes(reduce, feat, offsets, out):
    keep = []
    tf, to = _tensor(feat, keep), _tensor(out, keep)
    return LIB.dgla_segment_reduce_workspace_bytes(reduce.encode(), _idbits(offsets),
                                                   _DTYPES[out.dtype], ctypes.byref(tf),
                                                   offsets.shape[0] - 1, ctypes.byref(to))


def scatter_add(feat, idx, out):
    """out[idx[i]] += feat[i] (dgla_scatter_add; `out` is not zeroed)."""
    keep = []
    tf, to = _tensor(feat, keep), _tensor(out, keep)
    _require_gpu(idx)
    check_call(LIB.dgla_scatter_add(_idbits(idx), _DTYPES[out.dtype], ctypes.byref(tf),
                                    idx.data_ptr(), ctypes.byref(to), _stream(out)))


def backward_segment_cmp(feat, arg, out):
    """out[arg[i, k], k] = feat[i, k] where arg >= 0 (dgla_backward_segment_cmp)."""
    keep = []
    tf, to = _tensor(feat, keep), _tensor(out, keep)
    _require_gpu(arg)
    check_call(LIB.dgla_backward_segment_cmp(_idbits(arg), _DTYPES[out.dtype], ctypes.byref(tf),
                                             arg.data_ptr(), ctypes.byref(to), _stream(out)))


def spmm_cmp_backward(dz, arg, out, other=None, arg_other=None, other_group=1, atomic=True):
    """out[arg[i, k], k] (+)= dz[i, k] * other[arg_other[i, k], (k // other_group) % row_len(other)]
    where arg >= 0 (dgla_spmm_cmp_backward; `out` is not zeroed)."""
    keep = []
    tz, to = _tensor(dz, keep), _tensor(out, keep)
    _require_gpu(arg)
    tother = _tensor(other, keep) if other is not None else None
    check_call(LIB.dgla_spmm_cmp_backward(_idbits(arg), _DTYPES[out.dtype], ctypes.byref(tz), arg.data_ptr(),
                                          ctypes.byref(tother) if tother is not None else None,
                                          arg_other.data_ptr() if arg_other is not None else None, int(other_group),
                                          ctypes.byref(to), 1 if atomic else 0, _stream(out)))
    return out


def spmm_cmp_mask_words(dtype, feat_len):
    return int(LIB.dgla_spmm_cmp_mask_words(_DTYPES[dtype], int(feat_len)))


def spmm_cmp_mask_bytes(dtype, num_rows, nnz, feat_len):
    """Size of the `mask` buffer of :func:`spmm_cmp_mask` (edge words + the pass's partial sums)."""
    return int(LIB.dgla_spmm_cmp_mask_bytes(_DTYPES[dtype], int(num_rows), int(nnz), int(feat_len)))


CMP_MASK_DEFER, CMP_MASK_FINISH = 0x100, 0x200   # include/dgl_amd.h DGLA_CMP_MASK_*


def spmm_cmp_mask(csr, arg, dz, mask, dx, by_edge=False, mode=0):
    """Winner bits of a max / min g-SpMM over the FORWARD matrix `csr` (dgla_spmm_cmp_mask): for every edge in
    position order, one bit per output column; elements no edge claims go to ``dx[arg]`` here (``dx`` zeroed by
    the caller).  ``mode=CMP_MASK_DEFER``: ``dx`` is not touched (the masked g-SpMM then stores instead of accumulating);
    the same call with ``mode=CMP_MASK_FINISH`` behind the g-SpMM adds what was kept aside."""
    keep = []
    tz, tx = _tensor(dz, keep), _tensor(dx, keep)
    _require_gpu(arg)
    check_call(LIB.dgla_spmm_cmp_mask(ctypes.byref(csr), _DTYPES[dz.dtype], arg.data_ptr(), (1 if by_edge else 0) | int(mode),
                                      ctypes.byref(tz), _ptr(mask), ctypes.byref(tx), _stream(dx)))


def spmm_csr_masked_workspace_bytes(csr, ufeat, out):
    keep = []
    tu, to = _tensor(ufeat, keep), _tensor(out, keep)
    return LIB.dgla_spmm_csr_masked_workspace_bytes(ctypes.byref(csr), _DTYPES[out.dtype], ctypes.byref(tu),
                                                    ctypes.byref(to))


def spmm_csr_masked(csr, ufeat, mask, out, workspace=None, accumulate=False, plan_valid=False):
    """out (+)= sum over the edges of every row of `csr` of ufeat[col] gated per (edge, column) by `mask`, which is
    indexed through the CSR's edge-id map (dgla_spmm_csr_masked)."""
    keep = []
    tu, to = _tensor(ufeat, keep), _tensor(out, keep)
    flags = (_lib.DGLA_ACCUMULATE if accumulate else 0) | (_lib.DGLA_PLAN_VALID if plan_valid else 0)
    check_call(LIB.dgla_spmm_csr_masked(ctypes.byref(csr), _DTYPES[out.dtype], ctypes.byref(tu), _ptr(mask),
                                        ctypes.byref(to), *_ws(workspace), flags,
                                        _stream(out)))


def _mm_check(*ts):
    for t in ts:
        if t is None:
            continue
        _require_gpu(t)
        if not t.is_contiguous():
            raise _lib.DGLAMDError("matrices handed to segment_mm / gather_mm must be contiguous")


def segment_mm(a, b, c, seglen, b_trans=False, row_index=None):
    """c[rows of r] = a[rows of r] @ b[r]  (or @ b[r].T when b_trans); `seglen` may be a CPU or
    GPU int32/int64 tensor (dgla_segment_mm).  With `row_index` (int64, GPU) the logical row r
    lives at physical row row_index[r] of both a and c (dgla_segment_mm_indexed)."""
    _mm_check(a, b, c, row_index)
    if row_index is not None and row_index.dtype != torch.int64:
        raise _lib.DGLAMDError("row_index must be int64")
    k = a.shape[1]
    n = c.shape[1]
    check_call(LIB.dgla_segment_mm_indexed(
        _idbits(seglen), _DTYPES[a.dtype], a.data_ptr(), b.data_ptr(), c.data_ptr(), seglen.data_ptr(),
        0 if seglen.is_cuda else 1, _ptr(row_index), a.shape[0], seglen.shape[0], k, n,
        1 if b_trans else 0, None, 0, _stream(a)))


def segment_mm_backward_b(a, dc, db, seglen, row_index=None):
    """db[r] = a[rows of r].T @ dc[rows of r] (dgla_segment_mm_backward_b[_indexed])."""
    _mm_check(a, dc, db, row_index)
    if row_index is not None and row_index.dtype != torch.int64:
        raise _lib.DGLAMDError("row_index must be int64")
    check_call(LIB.dgla_segment_mm_backward_b_indexed(
        _idbits(seglen), _DTYPES[a.dtype], a.data_ptr(), dc.data_ptr(), db.data_ptr(),
        seglen.data_ptr(), 0 if seglen.is_cuda else 1, _ptr(row_index), a.shape[0], seglen.shape[0],
        a.shape[1], dc.shape[1], None, 0, _stream(a)))


def segment_mm_backward_b_last_route():
    """(fell_back, listed_elements) of the most recent fp32 two-term weight-gradient launch
    (dgla_segment_mm_backward_b_last_route; synchronises)."""
    fb, n = ctypes.c_uint32(0), ctypes.c_uint32(0)
    check_call(LIB.dgla_segment_mm_backward_b_last_route(ctypes.byref(fb), ctypes.byref(n)))
    return int(fb.value), int(n.value)


def gather_mm(a, b, c, idx_a=None, idx_b=None, idx_c=None):
    """c[idx_c[i]] = a[idx_a[i]] @ b[idx_b[i]] (dgla_gather_mm); absent index = identity."""
    _mm_check(a, b, c, idx_a, idx_b, idx_c)
    ref = next(t for t in (idx_a, idx_b, idx_c) if t is not None)
    rows = ref.shape[0]
    check_call(LIB.dgla_gather_mm(_idbits(ref), _DTYPES[a.dtype], a.data_ptr(), b.data_ptr(),
                                  c.data_ptr(), _ptr(idx_a), _ptr(idx_b), _ptr(idx_c), rows,
                                  a.shape[1], b.shape[-1], _stream(a)))


def coo_to_csr(row, col, eids, num_rows, num_minor=0):
    """(indptr, indices, eids_out) of the CSR that compresses `row` (dgla_coo_to_csr): stable,
    so COO order is kept inside every row; `eids_out[i]` = edge id of CSR position i.  `num_minor`
    (every `col` id is below it) lets int64 graphs take the packed 32-bit sort."""
    _require_gpu(row)
    bits = _idbits(row)
    nnz = row.shape[0]
    indptr = torch.empty(num_rows + 1, dtype=row.dtype, device=row.device)
    indices = torch.empty(nnz, dtype=row.dtype, device=row.device)
    eids_out = torch.empty(nnz, dtype=row.dtype, device=row.device)
    check_call(LIB.dgla_coo_to_csr_bounded(bits, int(num_rows), int(num_minor), nnz, _ptr(row), _ptr(col),
                                           _ptr(eids), indptr.data_ptr(), _ptr(indices), _ptr(eids_out), None, 0,
                                           _stream(row)))
    return indptr, indices, eids_out


def csr_mm_row_classes():
    """Term-count thresholds between the row classes of the sparse x sparse kernels, ascending (host query)."""
    buf = (ctypes.c_int64 * 8)()
    n = LIB.dgla_csr_mm_row_classes(buf, 8)
    return [int(buf[i]) for i in range(n)]


def csr_mm_workspace_bytes(a, b):
    return LIB.dgla_csr_mm_workspace_bytes(ctypes.byref(a), ctypes.byref(b))


def csr_mm(a, a_w, b, b_w, workspace=None):
    """(indptr, indices, weights) of a . b (dgla_csr_mm_count + dgla_csr_mm_fill) on the current stream; `a` / `b` from
    make_csr, weights 1-D per edge id.  The result's columns ascend in every row and it has no edge-id map."""
    _require_gpu(a_w)
    _require_gpu(b_w)
    if a_w.dtype != b_w.dtype:
        raise _lib.DGLAMDError("csr_mm: the weights must share one dtype")
    idt = torch.int32 if a.idtype_bits == 32 else torch.int64
    indptr = torch.empty(a.num_rows + 1, dtype=idt, device=a_w.device)
    nnz = ctypes.c_int64(0)
    wp, wb = _ws(workspace)
    check_call(LIB.dgla_csr_mm_count(ctypes.byref(a), ctypes.byref(b), indptr.data_ptr(), ctypes.byref(nnz), wp, wb,
                                     _stream(a_w)))
    indices = torch.empty(nnz.value, dtype=idt, device=a_w.device)
    w = torch.empty(nnz.value, dtype=a_w.dtype, device=a_w.device)
    check_call(LIB.dgla_csr_mm_fill(ctypes.byref(a), _DTYPES[a_w.dtype], _ptr(a_w), ctypes.byref(b), _ptr(b_w),
                                    indptr.data_ptr(), _ptr(indices), _ptr(w), wp, wb, _stream(a_w)))
    return indptr, indices, w


def csr_sum(ops, weights, workspace=None):
    """(indptr, indices, weights) of the sum of the CSR operands `ops` (dgla_csr_sum_count + dgla_csr_sum_fill)."""
    n = len(ops)
    for t in weights:
        _require_gpu(t)
    arr = (ctypes.POINTER(_lib.CSR) * n)(*[ctypes.pointer(o) for o in ops])
    wts = (ctypes.c_void_p * n)(*[_ptr(t) for t in weights])
    idt = torch.int32 if ops[0].idtype_bits == 32 else torch.int64
    dev = weights[0].device
    indptr = torch.empty(ops[0].num_rows + 1, dtype=idt, device=dev)
    nnz = ctypes.c_int64(0)
    wp, wb = _ws(workspace)
    check_call(LIB.dgla_csr_sum_count(arr, n, indptr.data_ptr(), ctypes.byref(nnz), wp, wb, _stream(weights[0])))
    indices = torch.empty(nnz.value, dtype=idt, device=dev)
    w = torch.empty(nnz.value, dtype=weights[0].dtype, device=dev)
    check_call(LIB.dgla_csr_sum_fill(arr, n, _DTYPES[weights[0].dtype], wts, indptr.data_ptr(), _ptr(indices), _ptr(w),
                                     wp, wb, _stream(weights[0])))
    return indptr, indices, w


def csr_mask(a, a_w, b_coo):
    """out[e] = a[row_b[e], col_b[e]] or 0 (dgla_csr_mask); `a` from make_csr, `b_coo` from make_coo."""
    _require_gpu(a_w)
    out = torch.empty(b_coo.nnz, dtype=a_w.dtype, device=a_w.device)
    check_call(LIB.dgla_csr_mask(ctypes.byref(a), _DTYPES[a_w.dtype], _ptr(a_w), ctypes.byref(b_coo), _ptr(out),
                                 _stream(a_w)))
    return out


def sample_neighbors(csr, seeds, fanout, replace=False, rng_seed=0):
    """Uniform in-neighbour sampling over the in-edge CSR `csr` (dgla_sample_neighbors):
    returns ``(indptr, src, eids)`` — a CSR over the seeds with GLOBAL source / edge ids."""
    _require_gpu(seeds)
    rng_seed = _u64(rng_seed)
    n = seeds.shape[0]
    dev, dt = seeds.device, seeds.dtype
    indptr = torch.empty(n + 1, dtype=dt, device=dev)
    st = _stream(seeds)
    if fanout < 0:  # all neighbours: sizes first
        check_call(LIB.dgla_sample_neighbors(ctypes.byref(csr), seeds.data_ptr(), n, fanout, 0, rng_seed,
                                             indptr.data_ptr(), None, None, None, 0, st))
        cap = int(indptr[-1])
    else:
        cap = n * fanout
    src = torch.empty(cap, dtype=dt, device=dev)
    eids = torch.empty(cap, dtype=dt, device=dev)
    check_call(LIB.dgla_sample_neighbors(ctypes.byref(csr), seeds.data_ptr(), n, fanout, 1 if replace else 0,
                                         rng_seed, indptr.data_ptr(), _ptr(src), _ptr(eids), None, 0, st))
    return indptr, src, eids


def sample_neighbors_weighted(csr, prob, seeds, fanout, replace=False, rng_seed=0):
    """Weighted in-neighbour sampling (dgla_sample_neighbors_weighted): `prob` is a float32 /
    float64 tensor with one non-negative weight per EDGE ID.  Returns ``(indptr, src, eids)``;
    edges of weight 0 never appear, so rows may hold fewer than `fanout` entries."""
    _require_gpu(seeds)
    _require_gpu(prob)
    _prob_ok(prob)
    rng_seed = _u64(rng_seed)
    n = seeds.shape[0]
    dev, dt = seeds.device, seeds.dtype
    indptr = torch.empty(n + 1, dtype=dt, device=dev)
    src = torch.empty(n * fanout, dtype=dt, device=dev)
    eids = torch.empty(n * fanout, dtype=dt, device=dev)
    check_call(LIB.dgla_sample_neighbors_weighted(
        ctypes.byref(csr), prob.data_ptr(), _DTYPES[prob.dtype], seeds.data_ptr(), n, int(fanout),
        1 if replace else 0, rng_seed, indptr.data_ptr(), _ptr(src), _ptr(eids), None, 0, _stream(seeds)))
    return indptr, src, eids


def host_csr(indptr, indices, eids, num_cols):
    """dgla_csr over CPU tensors, for the host-only entry points (dgla_random_walk_host)."""
    for t in (indptr, indices, eids):
        if t is not None and (t.is_cuda or not t.is_contiguous()):
            raise _lib.DGLAMDError("host_csr takes contiguous CPU tensors")
    c = CSR(indptr.shape[0] - 1, int(num_cols), indices.shape[0], _idbits(indptr), indptr.data_ptr(), _ptr(indices),
            _ptr(eids))
    c._keep = (indptr, indices, eids)
    return c


def random_walk_cdf(csr, prob):
    """The row-wise inclusive sums of the weights of `csr` (dgla_random_walk_cdf): float64 [nnz] in CSR position order,
    what the weighted step of :func:`random_walk` bisects.  `prob` is float32 / float64, one weight per EDGE ID."""
    _require_gpu(prob)
    _prob_ok(prob)
    if prob.shape[0] != csr.nnz:
        raise _lib.DGLAMDError("prob must hold one value per edge (%d), got %d" % (csr.nnz, prob.shape[0]))
    cdf = torch.empty(csr.nnz, dtype=torch.float64, device=prob.device)
    need = LIB.dgla_random_walk_cdf_workspace_bytes(ctypes.byref(csr))
    ws = _workspace(need, prob.device)
    check_call(LIB.dgla_random_walk_cdf(ctypes.byref(csr), prob.data_ptr(), _DTYPES[prob.dtype], cdf.data_ptr(),
                                        _ptr(ws), need, _stream(prob)))
    return cdf


def _walk_args(rels, metapath, seeds, restart_prob, restart_steps, rng_seed, return_eids):
    """The argument list the device and the host walker share; `rels` = [(dgla_csr, cdf tensor or None), ...]."""
    table = (_lib.WalkRelation * max(1, len(rels)))()
    for k, (csr, cdf) in enumerate(rels):
        if cdf is not None and (cdf.dtype != torch.float64 or cdf.numel() != csr.nnz or not cdf.is_contiguous()):
            raise _lib.DGLAMDError("a relation's cdf must be a contiguous float64 tensor with one entry per edge")
        table[k].csr = ctypes.pointer(csr)
        table[k].cdf = _ptr(cdf)
    steps = len(metapath)
    path = (ctypes.c_int32 * max(1, steps))(*[int(m) for m in metapath])
    if restart_steps is not None:
        if restart_steps.dtype not in (torch.float32, torch.float64) or restart_steps.dim() != 1 or \
                restart_steps.shape[0] != steps or not restart_steps.is_contiguous():
            raise _lib.DGLAMDError("restart_steps must be a contiguous float32 / float64 tensor with one entry per step")
    n = seeds.shape[0]
    traces = torch.empty((n, steps + 1), dtype=seeds.dtype, device=seeds.device)
    eids = torch.empty((n, steps), dtype=seeds.dtype, device=seeds.device) if return_eids else None
    args = [table if rels else None, len(rels), path, steps, seeds.data_ptr(), n, float(restart_prob or 0.0),
            _ptr(restart_steps), _DTYPES[restart_steps.dtype] if restart_steps is not None else 0,
            _u64(rng_seed), traces.data_ptr(), _ptr(eids)]
    return args, traces, eids, (table, path, rels)


def random_walk(rels, metapath, seeds, restart_prob=0.0, restart_steps=None, rng_seed=0, return_eids=True):
    """Random walks over the out-edge CSRs `rels` = [(dgla_csr, cdf or None), ...] along `metapath` (relation indices),
    one walk per entry of `seeds` (dgla_random_walk).  Returns ``(traces [n, steps + 1], eids [n, steps] or None)``;
    a walk that halts is padded with -1.  Nothing is read back."""
    _all_on(True, "random_walk", seeds, restart_steps, *[c for _, c in rels])
    if not seeds.is_contiguous() or (rels and _idbits(seeds) != rels[0][0].idtype_bits):
        raise _lib.DGLAMDError("seeds must be contiguous and of the relations' id type")
    args, traces, eids, keep = _walk_args(rels, metapath, seeds, restart_prob, restart_steps, rng_seed, return_eids)
    need = LIB.dgla_random_walk_workspace_bytes(len(rels), len(metapath))
    ws = _workspace(need, seeds.device)
    check_call(LIB.dgla_random_walk(*args, _ptr(ws), need, _stream(seeds)))
    return traces, eids


def random_walk_host(rels, metapath, seeds, restart_prob=0.0, restart_steps=None, rng_seed=0, return_eids=True):
    """:func:`random_walk` run by the CPU on CPU tensors (dgla_random_walk_host; `rels` built with :func:`host_csr`):
    the same step rule compiled for the host, bit for bit what the kernel writes.  Needs no GPU."""
    _all_on(False, "random_walk_host", seeds, restart_steps, *[c for _, c in rels])
    if not seeds.is_contiguous() or (rels and _idbits(seeds) != rels[0][0].idtype_bits):
        raise _lib.DGLAMDError("seeds must be contiguous and of the relations' id type")
    args, traces, eids, keep = _walk_args(rels, metapath, seeds, restart_prob, restart_steps, rng_seed, return_eids)
    check_call(LIB.dgla_random_walk_host(*args))
    return traces, eids


def csr_sorted_columns(csr):
    """The membership list of `csr` (dgla_csr_sorted_columns): every row's column ids in ascending order, duplicates
    kept, over the same indptr; what the node2vec step bisects to learn whether an edge exists.  `csr` from
    :func:`make_csr`; nothing is read back."""
    indptr = csr._keep[0]
    _require_gpu(indptr)
    member = torch.empty(csr.nnz, dtype=indptr.dtype, device=indptr.device)
    need = LIB.dgla_csr_sorted_columns_workspace_bytes(ctypes.byref(csr))
    ws = _workspace(need, indptr.device)
    check_call(LIB.dgla_csr_sorted_columns(ctypes.byref(csr), member.data_ptr(), _ptr(ws), need, _stream(indptr)))
    return member


def _n2v_args(csr, cdf, member, seeds, num_steps, p, q, rng_seed, return_eids):
    """The argument list the device and the host node2vec walker share."""
    if cdf is not None and (cdf.dtype != torch.float64 or cdf.numel() != csr.nnz or not cdf.is_contiguous()):
        raise _lib.DGLAMDError("the cdf must be a contiguous float64 tensor with one entry per edge")
    _member_ok(csr, member)
    if not seeds.is_contiguous() or _idbits(seeds) != csr.idtype_bits:
        raise _lib.DGLAMDError("seeds must be contiguous and of the csr's id type")
    n, steps = seeds.shape[0], int(num_steps)
    if steps < 0:
        raise _lib.DGLAMDError("the number of steps must not be negative")
    traces = torch.empty((n, steps + 1), dtype=seeds.dtype, device=seeds.device)
    eids = torch.empty((n, steps), dtype=seeds.dtype, device=seeds.device) if return_eids else None
    args = [ctypes.byref(csr), _ptr(cdf), member.data_ptr(), seeds.data_ptr(), n, steps, float(p), float(q),
            _u64(rng_seed), traces.data_ptr(), _ptr(eids)]
    return args, traces, eids


def node2vec_walk(csr, cdf, member, seeds, num_steps, p, q, rng_seed=0, return_eids=True):
    """node2vec walks over the out-edge CSR `csr` (dgla_node2vec_walk): `cdf` from :func:`random_walk_cdf` or None,
    `member` from :func:`csr_sorted_columns`.  Returns ``(traces [n, steps + 1], eids [n, steps] or None)``; a walk that
    halts is padded with -1.  Nothing is read back."""
    _all_on(True, "node2vec_walk", seeds, member, cdf)
    args, traces, eids = _n2v_args(csr, cdf, member, seeds, num_steps, p, q, rng_seed, return_eids)
    check_call(LIB.dgla_node2vec_walk(*args, _stream(seeds)))
    return traces, eids


def node2vec_walk_host(csr, cdf, member, seeds, num_steps, p, q, rng_seed=0, return_eids=True, stats=False):
    """:func:`node2vec_walk` run by the CPU on CPU tensors (dgla_node2vec_walk_host; `csr` built with :func:`host_csr`):
    the same step rule compiled for the host, bit for bit what the kernel writes.  Needs no GPU.  With ``stats`` a third
    result ``[steps t >= 1 that recorded a node, candidates drawn, steps that reached the scan]``."""
    _all_on(False, "node2vec_walk_host", seeds, member, cdf)
    args, traces, eids = _n2v_args(csr, cdf, member, seeds, num_steps, p, q, rng_seed, return_eids)
    counters = (ctypes.c_int64 * 3)() if stats else None
    check_call(LIB.dgla_node2vec_walk_host(*args, counters))
    return (traces, eids, [int(c) for c in counters]) if stats else (traces, eids)


def _neg_args(csr, member, n_slots, num_samples, num_trials, exclude_self_loops, replace, rng_seed):
    """The argument list the device and the host negative sampler share (outputs on the device of `csr`'s indptr)."""
    _member_ok(csr, member)
    indptr = csr._keep[0]
    n_slots, num_samples = int(n_slots), int(num_samples)
    if n_slots < 0 or num_samples < 0:
        raise _lib.DGLAMDError("the number of slots / samples must not be negative")
    src = torch.empty(num_samples, dtype=indptr.dtype, device=indptr.device)
    dst = torch.empty(num_samples, dtype=indptr.dtype, device=indptr.device)
    count = torch.empty(1, dtype=torch.int64, device=indptr.device)
    args = [ctypes.byref(csr), member.data_ptr(), n_slots, num_samples, int(num_trials), 1 if exclude_self_loops else 0,
            1 if replace else 0, _u64(rng_seed), src.data_ptr(), dst.data_ptr(), count.data_ptr()]
    return args, src, dst, count


def negative_sample(csr, member, n_slots, num_samples, num_trials=3, exclude_self_loops=True, replace=False, rng_seed=0):
    """Global uniform negative pairs of the out-edge CSR `csr` (dgla_negative_sample): `member` from
    :func:`csr_sorted_columns`.  Returns ``(src [num_samples], dst [num_samples], count [1] int64)`` on the device; the
    entries from ``count`` on are -1.  Nothing is read back and nothing is allocated by the library (the workspace is a
    torch tensor), so the call can be captured in a graph."""
    _all_on(True, "negative_sample", csr._keep[0], member)
    args, src, dst, count = _neg_args(csr, member, n_slots, num_samples, num_trials, exclude_self_loops, replace, rng_seed)
    need = LIB.dgla_negative_sample_workspace_bytes(csr.idtype_bits, int(n_slots))
    ws = _workspace(need, src.device)
    check_call(LIB.dgla_negative_sample(*args, _ptr(ws), need, _stream(src)))
    return src, dst, count


def negative_sample_host(csr, member, n_slots, num_samples, num_trials=3, exclude_self_loops=True, replace=False,
                         rng_seed=0):
    """:func:`negative_sample` run by the CPU on CPU tensors (dgla_negative_sample_host; `csr` built with
    :func:`host_csr`): the same rule compiled for the host, bit for bit what the kernels write.  Needs no GPU."""
    _all_on(False, "negative_sample_host", member)
    args, src, dst, count = _neg_args(csr, member, n_slots, num_samples, num_trials, exclude_self_loops, replace, rng_seed)
    check_call(LIB.dgla_negative_sample_host(*args))
    return src, dst, count


def _has_edges_args(csr, member, u, v):
    _member_ok(csr, member)
    if u.shape != v.shape or u.dim() != 1 or _idbits(u) != csr.idtype_bits or _idbits(v) != csr.idtype_bits or \
            not u.is_contiguous() or not v.is_contiguous():
        raise _lib.DGLAMDError("u and v must be contiguous 1-D tensors of the csr's id type and of one length")
    out = torch.empty(u.shape[0], dtype=torch.uint8, device=u.device)
    return [ctypes.byref(csr), member.data_ptr(), u.data_ptr(), v.data_ptr(), u.shape[0], out.data_ptr()], out


def csr_has_edges(csr, member, u, v):
    """Whether u[i] -> v[i] is an edge of `csr` (dgla_csr_has_edges), as a bool tensor: a bisection of the membership
    list of :func:`csr_sorted_columns`; ids out of range give False.  Nothing is read back."""
    _all_on(True, "csr_has_edges", member, u, v)
    args, out = _has_edges_args(csr, member, u, v)
    check_call(LIB.dgla_csr_has_edges(*args, _stream(u)))
    return out.view(torch.bool)


def csr_has_edges_host(csr, member, u, v):
    """:func:`csr_has_edges` on CPU tensors (dgla_csr_has_edges_host).  Needs no GPU."""
    _all_on(False, "csr_has_edges_host", member, u, v)
    args, out = _has_edges_args(csr, member, u, v)
    check_call(LIB.dgla_csr_has_edges_host(*args))
    return out.view(torch.bool)


def _labor_rel(csr, prob, seeds, c=None):
    """The leading arguments the layer-neighbour entry points share: (csr, prob, prob_dtype)."""
    if prob is not None:
        _prob_ok(prob)
        if prob.shape[0] != csr.nnz:
            raise _lib.DGLAMDError("prob must hold one value per edge (%d), got %d" % (csr.nnz, prob.shape[0]))
    if seeds.dim() != 1 or not seeds.is_contiguous() or _idbits(seeds) != csr.idtype_bits:
        raise _lib.DGLAMDError("seeds must be a contiguous 1-D tensor of the csr's id type")
    if c is not None and (c.dtype != torch.float64 or c.shape != seeds.shape or not c.is_contiguous()):
        raise _lib.DGLAMDError("c must be a contiguous float64 tensor with one entry per seed")
    if prob is not None and c is not None and c.device != prob.device:
        raise _lib.DGLAMDError("c and prob must be on one device")
    return [ctypes.byref(csr), _ptr(prob), _DTYPES[prob.dtype] if prob is not None else 0]


def labor_scale(csr, prob, seeds, fanout):
    """The per-seed scale ``c`` of weighted layer-neighbour sampling (dgla_labor_scale; the rule: include/dgl_amd.h):
    float64 [len(seeds)], the solution of ``sum min(1, c w') = fanout`` over each seed's row.  Nothing is read back."""
    _all_on(True, "labor_scale", csr._keep[0], prob, seeds)
    rel = _labor_rel(csr, prob, seeds)
    c = torch.empty(seeds.shape[0], dtype=torch.float64, device=seeds.device)
    check_call(LIB.dgla_labor_scale(*rel, _ptr(seeds), seeds.shape[0], int(fanout), _ptr(c), _stream(seeds)))
    return c


def labor_scale_host(csr, prob, seeds, fanout):
    """:func:`labor_scale` run by the CPU on CPU tensors (dgla_labor_scale_host; `csr` built with :func:`host_csr`).
    Needs no GPU."""
    _all_on(False, "labor_scale_host", prob, seeds)
    rel = _labor_rel(csr, prob, seeds)
    c = torch.empty(seeds.shape[0], dtype=torch.float64)
    check_call(LIB.dgla_labor_scale_host(*rel, _ptr(seeds), seeds.shape[0], int(fanout), _ptr(c)))
    return c


def labor_sample(csr, seeds, fanout, rng_seed=0, prob=None, c=None):
    """Layer-neighbour sampling over the CSR `csr` whose rows are the seed side (dgla_labor_count + dgla_labor_fill):
    returns ``(indptr, nbr, eids, importances)``, a CSR over the seeds with GLOBAL neighbour / edge ids; `importances`
    (prob's dtype) is None without `prob`.  `c` from :func:`labor_scale` (computed here when None).  Reading the total
    is the one host synchronisation."""
    _all_on(True, "labor_sample", csr._keep[0], prob, seeds, c)
    if prob is not None and c is None:
        c = labor_scale(csr, prob, seeds, fanout)
    rel = _labor_rel(csr, prob, seeds, c)
    n, dev, dt = seeds.shape[0], seeds.device, seeds.dtype
    need = LIB.dgla_labor_workspace_bytes(csr.idtype_bits, n)
    ws = _workspace(need, dev)
    indptr = torch.empty(n + 1, dtype=dt, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    st = _stream(seeds)
    args = rel + [_ptr(c), _ptr(seeds), n, int(fanout), _u64(rng_seed)]
    check_call(LIB.dgla_labor_count(*args, _ptr(indptr), _ptr(total), _ptr(ws), need, st))
    cap = int(total.item())
    if csr.idtype_bits == 32 and cap >= 2 ** 31:
        raise _lib.DGLAMDError("labor_sample: %d picked edges do not fit int32 ids; use int64 ids" % cap)
    nbr = torch.empty(cap, dtype=dt, device=dev)
    eids = torch.empty(cap, dtype=dt, device=dev)
    imp = torch.empty(cap, dtype=prob.dtype, device=dev) if prob is not None else None
    check_call(LIB.dgla_labor_fill(*args, cap, _ptr(nbr), _ptr(eids), _ptr(imp), _ptr(ws), need, st))
    return indptr, nbr, eids, imp


def labor_pick_host(csr, seeds, fanout, rng_seed=0, prob=None, c=None):
    """:func:`labor_sample` run by the CPU on CPU tensors (dgla_labor_pick_host; `csr` built with :func:`host_csr`): the
    same rule compiled for the host, bit for bit what the kernels write from the same `c`.  Needs no GPU."""
    _all_on(False, "labor_pick_host", prob, seeds, c)
    if prob is not None and c is None:
        c = labor_scale_host(csr, prob, seeds, fanout)
    rel = _labor_rel(csr, prob, seeds, c)
    n, dt = seeds.shape[0], seeds.dtype
    indptr = torch.empty(n + 1, dtype=dt)
    args = rel + [_ptr(c), _ptr(seeds), n, int(fanout), _u64(rng_seed)]
    check_call(LIB.dgla_labor_pick_host(*args, _ptr(indptr), None, None, None))       # the sizes
    cap = int(indptr[-1])
    nbr, eids = torch.empty(cap, dtype=dt), torch.empty(cap, dtype=dt)
    imp = torch.empty(cap, dtype=prob.dtype) if prob is not None else None
    if cap:     # (an empty tensor has no address to hand over)
        check_call(LIB.dgla_labor_pick_host(*args, _ptr(indptr), _ptr(nbr), _ptr(eids), _ptr(imp)))
    return indptr, nbr, eids, imp


def knn_max_k():
    """kKnnMaxK: the largest k of :func:`knn` (host query)."""
    return int(LIB.dgla_knn_max_k())


def knn_tile_sizes():
    """(queries per workgroup, data rows per LDS tile) of the k-NN kernel (host query)."""
    q, d = ctypes.c_int(), ctypes.c_int()
    LIB.dgla_knn_tile_sizes(ctypes.byref(q), ctypes.byref(d))
    return q.value, d.value


def _knn_args(who, x, y, x_offsets, y_offsets, k, idtype, with_dist, gpu):
    """The arguments the two k-NN entry points share, and their outputs.  The offsets are host sequences of ints."""
    _all_on(gpu, who, x, y)
    for t in (x, y):
        if t is not None and (t.dim() != 2 or not t.is_contiguous()):
            raise _lib.DGLAMDError("%s: x and y must be contiguous 2-D tensors" % who)
    if y is not None and (y.dtype != x.dtype or y.shape[1] != x.shape[1] or y.device != x.device):
        raise _lib.DGLAMDError("%s: x and y must share dtype, width and device" % who)
    if x.dtype not in _DTYPES:
        raise _lib.DGLAMDError("%s: x must be a floating-point tensor, got %s" % (who, x.dtype))
    if len(x_offsets) != len(y_offsets) or len(x_offsets) < 1:
        raise _lib.DGLAMDError("%s: x_offsets and y_offsets do not match: %d and %d entries"
                               % (who, len(x_offsets), len(y_offsets)))
    num_segs = len(x_offsets) - 1
    xo = (ctypes.c_int64 * (num_segs + 1))(*[int(v) for v in x_offsets])
    yo = (ctypes.c_int64 * (num_segs + 1))(*[int(v) for v in y_offsets])
    num_y = x.shape[0] if y is None else y.shape[0]
    k = int(k)
    slots = num_y * max(k, 0)
    ids = torch.empty((2, slots), dtype=idtype, device=x.device)
    dist = torch.empty(slots, dtype=x.dtype, device=x.device) if with_dist else None
    args = [_ptr(x), x.shape[0], _ptr(y), num_y, _DTYPES[x.dtype], x.shape[1], xo, yo, num_segs, k,
            _id_bits(idtype), _ptr(ids), _ptr(dist)]
    return args, num_segs, ids, dist


def knn(x, x_offsets, k, y=None, y_offsets=None, idtype=torch.int64, with_dist=False):
    """k nearest rows of `x` for every row of `y` inside the same segment (dgla_knn; the rule: include/dgl_amd.h
    "Point-cloud graphs").  `x_offsets` / `y_offsets` are host sequences [S + 1]; ``y=None`` is the self-query.  Returns
    the (2, k * num_y) id tensor (queries, global data rows; -1 where a segment is shorter than k) and, with `with_dist`,
    the squared distances.  One launch, nothing read back."""
    args, num_segs, ids, dist = _knn_args("knn", x, y, x_offsets, x_offsets if y_offsets is None else y_offsets, k, idtype,
                                          with_dist, True)
    need = LIB.dgla_knn_workspace_bytes(num_segs)
    ws = _workspace(need, x.device)
    check_call(LIB.dgla_knn(*args, _ptr(ws), need, _stream(x)))
    return (ids, dist) if with_dist else ids


def knn_host(x, x_offsets, k, y=None, y_offsets=None, idtype=torch.int64, with_dist=False):
    """:func:`knn` run by the CPU on CPU tensors (dgla_knn_host): the same rule compiled for the host, bit for bit what
    the kernel writes.  Needs no GPU."""
    args, _, ids, dist = _knn_args("knn_host", x, y, x_offsets, x_offsets if y_offsets is None else y_offsets, k, idtype,
                                   with_dist, False)
    check_call(LIB.dgla_knn_host(*args))
    return (ids, dist) if with_dist else ids


def _fps_args(who, pos, npoints, start, gpu):
    _all_on(gpu, who, pos, start)
    if pos.dim() != 3 or not pos.is_contiguous() or pos.dtype not in _DTYPES:
        raise _lib.DGLAMDError("%s: pos must be a contiguous floating-point (B, N, C) tensor" % who)
    B, N, C = pos.shape
    if start.dtype != torch.int64 or start.shape != (B,) or not start.is_contiguous() or start.device != pos.device:
        raise _lib.DGLAMDError("%s: start must be a contiguous int64 tensor with one row per cloud, on pos's device" % who)
    out = torch.empty((B, max(int(npoints), 0)), dtype=torch.int64, device=pos.device)
    return [_ptr(pos), _DTYPES[pos.dtype], B, N, C, int(npoints), _ptr(start), _ptr(out)], out


def fps(pos, npoints, start):
    """Farthest point sampling of every cloud of `pos` (B, N, C) from the rows `start` (B,) (dgla_fps; the rule:
    include/dgl_amd.h "Point-cloud graphs"): (B, npoints) int64 row numbers inside each cloud.  One launch."""
    args, out = _fps_args("fps", pos, npoints, start, True)
    need = LIB.dgla_fps_workspace_bytes(args[1], args[2], args[3])
    ws = _workspace(need, pos.device)
    check_call(LIB.dgla_fps(*args, _ptr(ws), need, _stream(pos)))
    return out


def fps_host(pos, npoints, start):
    """:func:`fps` run by the CPU on CPU tensors (dgla_fps_host).  Needs no GPU."""
    args, out = _fps_args("fps_host", pos, npoints, start, False)
    check_call(LIB.dgla_fps_host(*args))
    return out


MATCHING_MAX_ROUNDS = 256     # the default round cap of neighbour matching


def _matching_args(who, csr, weight, rng_seed, max_rounds, gpu):
    """The arguments the two neighbour-matching entry points share (csr, weight, weight_dtype, seed, max_rounds)."""
    _all_on(gpu, who, csr._keep[0], weight)
    if weight is not None:
        if weight.dim() != 1 or not weight.is_contiguous() or weight.dtype not in _DTYPES:
            raise _lib.DGLAMDError("%s: weight must be a contiguous 1-D floating-point tensor" % who)
        if weight.shape[0] != csr.nnz:
            raise _lib.DGLAMDError("%s: weight must hold one value per edge (%d), got %d" % (who, csr.nnz, weight.shape[0]))
        if weight.device != csr._keep[0].device:
            raise _lib.DGLAMDError("%s: weight and the csr must be on one device" % who)
    return [ctypes.byref(csr), _ptr(weight), _DTYPES[weight.dtype] if weight is not None else 0, _u64(rng_seed),
            int(max_rounds)]


def neighbor_matching(csr, weight=None, rng_seed=0, max_rounds=MATCHING_MAX_ROUNDS, relabel=False, batch_rounds=0,
                      workspace=None):
    """Neighbour matching of the square CSR `csr` (dgla_neighbor_matching; the rule: include/dgl_amd.h "Graph
    matching"): returns ``(label, rounds)``, `label` [num_rows] in the csr's id type with the smaller id of every
    node's cluster (or, with `relabel`, consecutive cluster ids in ascending label order, dgla_neighbor_matching_relabel).
    `weight` holds one non-negative value per EDGE ID.  The host reads one word back per `batch_rounds` rounds (0: the
    library's default); `workspace` (uint8, dgla_neighbor_matching_workspace_bytes) is optional."""
    args = _matching_args("neighbor_matching", csr, weight, rng_seed, max_rounds, True)
    indptr = csr._keep[0]
    n = csr.num_rows
    label = torch.empty(n, dtype=indptr.dtype, device=indptr.device)
    rounds = ctypes.c_int64(0)
    st = _stream(indptr)
    check_call(LIB.dgla_neighbor_matching(*args, int(batch_rounds), _ptr(label), ctypes.byref(rounds), *_ws(workspace), st))
    if relabel:
        out = torch.empty_like(label)
        check_call(LIB.dgla_neighbor_matching_relabel(_ptr(label), csr.idtype_bits, n, _ptr(out), *_ws(workspace), st))
        label = out
    return label, rounds.value


def neighbor_matching_host(csr, weight=None, rng_seed=0, max_rounds=MATCHING_MAX_ROUNDS, relabel=False):
    """:func:`neighbor_matching` run by the CPU on CPU tensors (dgla_neighbor_matching_host; `csr` built with
    :func:`host_csr`): the same rule compiled for the host, bit for bit what the kernels write.  With `relabel` returns
    ``(label, rounds, relabelled)``.  Needs no GPU."""
    args = _matching_args("neighbor_matching_host", csr, weight, rng_seed, max_rounds, False)
    indptr = csr._keep[0]
    label = torch.empty(csr.num_rows, dtype=indptr.dtype)
    out = torch.empty_like(label) if relabel else None
    rounds = ctypes.c_int64(0)
    check_call(LIB.dgla_neighbor_matching_host(*args, _ptr(label), ctypes.byref(rounds), _ptr(out)))
    return (label, rounds.value, out) if relabel else (label, rounds.value)


SUBGRAPH_OUT_OF_RANGE, SUBGRAPH_DUPLICATE = 1, 2     # the flag bits of node_map_mark (include/dgl_amd.h)


def _node_map_args(who, ids, node_map):
    _all_on(True, who, ids, node_map)
    if ids.dim() != 1 or not ids.is_contiguous():
        raise _lib.DGLAMDError("%s: ids must be a contiguous 1-D tensor" % who)
    if node_map.dtype != torch.int32 or node_map.dim() != 1 or not node_map.is_contiguous() or node_map.device != ids.device:
        raise _lib.DGLAMDError("%s: the node map must be a contiguous 1-D int32 tensor on the ids' device" % who)
    return [_idbits(ids), _ptr(ids), ids.shape[0], _ptr(node_map), node_map.shape[0]]


def node_map_mark(ids, node_map, flags):
    """``node_map[ids[i]] = i`` (dgla_node_map_mark).  `node_map` is int32 scratch that is all -1 between calls; `flags`
    is a one-element int32 device tensor the call ORs SUBGRAPH_OUT_OF_RANGE / SUBGRAPH_DUPLICATE into.  Nothing is read
    back."""
    args = _node_map_args("node_map_mark", ids, node_map)
    if flags.dtype != torch.int32 or flags.numel() != 1 or flags.device != ids.device:
        raise _lib.DGLAMDError("node_map_mark: flags must be one int32 on the ids' device")
    check_call(LIB.dgla_node_map_mark(*args, _ptr(flags), _stream(ids)))


def node_map_clear(ids, node_map):
    """Writes -1 back at ``node_map[ids]`` (dgla_node_map_clear); ids out of range are skipped."""
    check_call(LIB.dgla_node_map_clear(*_node_map_args("node_map_clear", ids, node_map), _stream(ids)))


def _flag_error(who, flags):
    if flags & SUBGRAPH_OUT_OF_RANGE:
        raise _lib.DGLAMDError("%s: node id out of range" % who)
    if flags & SUBGRAPH_DUPLICATE:
        raise _lib.DGLAMDError("%s: duplicate node id" % who)


def _id_tensor_ok(who, name, t, like):
    """`t` is a contiguous 1-D tensor with the dtype and the device of `like`, an array of the csr."""
    if t is None or t.dim() != 1 or not t.is_contiguous() or t.dtype != like.dtype or t.device != like.device:
        raise _lib.DGLAMDError("%s: %s must be a contiguous 1-D tensor of the csr's id type on its device" % (who, name))


def _subgraph_rows_ok(who, csr, rows):
    if rows.dim() != 1 or not rows.is_contiguous() or _idbits(rows) != csr.idtype_bits:
        raise _lib.DGLAMDError("%s: rows must be a contiguous 1-D tensor of the csr's id type" % who)


def induced_subgraph(csr, rows, col_map, eid_order=True, col_ids=None, flags=None, workspace=None):
    """The entries of `csr` whose row is in `rows` and whose column is selected (dgla_induced_subgraph_count + _fill; the
    rule: include/dgl_amd.h "Induced subgraphs").  Returns ``(out_indptr, row, col, eid)``: LOCAL row / column ids and
    the edge ids, in ascending edge-id order (`eid_order`) or in row order, where ``out_indptr`` is the result's CSR.

    `col_map` is the int32 node map of the column side.  With `col_ids` the call owns it: it marks the map from
    `col_ids`, and ALWAYS clears it again, also when it refuses.  Without, the caller has marked it (into the device
    word `flags`) and clears it.  Either way the flags are read back together with the total, the one host
    synchronisation, and a set bit raises ``DGLAMDError`` ("node id out of range" / "duplicate node id").  `workspace`
    (uint8) is optional; one that is too small for the result is refused."""
    who = "induced_subgraph"
    _all_on(True, who, csr._keep[0], rows, col_map, col_ids, flags)
    _subgraph_rows_ok(who, csr, rows)
    if col_map.dtype != torch.int32 or not col_map.is_contiguous() or col_map.shape[0] < csr.num_cols:
        raise _lib.DGLAMDError("%s: col_map must be a contiguous int32 tensor with one entry per column node" % who)
    nr, dev, dt, bits = rows.shape[0], rows.device, rows.dtype, csr.idtype_bits
    st = _stream(rows)
    if flags is None:
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
    try:
        if col_ids is not None:
            node_map_mark(col_ids, col_map, flags)
        need = LIB.dgla_induced_subgraph_workspace_bytes(bits, nr, 0)
        ws = workspace if workspace is not None else _workspace(need, dev)
        out_indptr = torch.empty(nr + 1, dtype=dt, device=dev)
        check_call(LIB.dgla_induced_subgraph_count(ctypes.byref(csr), _ptr(rows), nr, _ptr(col_map), _ptr(out_indptr),
                                                   *_ws(ws), st))
        total, fl = torch.stack([out_indptr[nr].long(), flags[0].long()]).tolist()
        _flag_error(who, fl)
        row = torch.empty(total, dtype=dt, device=dev)
        col = torch.empty(total, dtype=dt, device=dev)
        eid = torch.empty(total, dtype=dt, device=dev)
        if workspace is None and eid_order:
            ws = _workspace(LIB.dgla_induced_subgraph_workspace_bytes(bits, nr, total), dev)
        check_call(LIB.dgla_induced_subgraph_fill(ctypes.byref(csr), _ptr(rows), nr, _ptr(col_map), _ptr(out_indptr), total,
                                                  _ptr(row), _ptr(col), _ptr(eid), 1 if eid_order else 0, *_ws(ws), st))
    finally:
        if col_ids is not None:
            node_map_clear(col_ids, col_map)
    return out_indptr, row, col, eid


def induced_subgraph_host(csr, rows, cols, eid_order=True):
    """:func:`induced_subgraph` run by the CPU on CPU tensors (dgla_induced_subgraph_host; `csr` built with
    :func:`host_csr`): the same rule compiled for the host, bit for bit what the kernels write.  `cols` is the column
    selection as a list of ids.  Returns ``(out_indptr, row, col, eid, flags)``; with a flag set the arrays are not
    meaningful.  Needs no GPU."""
    who = "induced_subgraph_host"
    _all_on(False, who, rows, cols)
    _subgraph_rows_ok(who, csr, rows)
    if cols.dim() != 1 or not cols.is_contiguous() or cols.dtype != rows.dtype:
        raise _lib.DGLAMDError("%s: cols must be a contiguous 1-D tensor of the csr's id type" % who)
    nr, dt = rows.shape[0], rows.dtype
    out_indptr = torch.empty(nr + 1, dtype=dt)
    total, flags = ctypes.c_int64(0), ctypes.c_int32(0)
    args = [ctypes.byref(csr), _ptr(rows), nr, _ptr(cols), cols.shape[0], 1 if eid_order else 0, _ptr(out_indptr)]
    check_call(LIB.dgla_induced_subgraph_host(*args, None, None, None, ctypes.byref(total), ctypes.byref(flags)))   # sizes
    row, col, eid = (torch.empty(total.value, dtype=dt) for _ in range(3))
    if total.value:     # (an empty tensor has no address to hand over)
        check_call(LIB.dgla_induced_subgraph_host(*args, _ptr(row), _ptr(col), _ptr(eid), ctypes.byref(total),
                                                  ctypes.byref(flags)))
    return out_indptr, row, col, eid, flags.value


EXCLUDE_OUT_OF_RANGE = 1     # the flag bit of exclude_set / compact_nodes (include/dgl_amd.h)


def _ids_ok(who, gpu, *tensors):
    """1-D contiguous id tensors of one width, all on the device (`gpu`) or all on the CPU; None entries are skipped."""
    ts = [t for t in tensors if t is not None]
    _all_on(gpu, who, *ts)
    for t in ts:
        if t.dim() != 1 or not t.is_contiguous() or t.dtype != ts[0].dtype or t.device != ts[0].device:
            raise _lib.DGLAMDError("%s: the arrays must be contiguous 1-D tensors of one id type on one device" % who)
    return _idbits(ts[0])


def exclude_set(ids, num_edges, reverse=None, workspace=None):
    """The exclusion set of the seed edges `ids` (dgla_exclude_set; the rule: include/dgl_amd.h "Edge exclusion and
    compaction"): ``sort(ids ++ reverse[ids])``, or ``sort(ids)`` without a reverse map.  The flag word is read back once
    and an id outside ``[0, num_edges)`` raises ``DGLAMDError`` ("edge id out of range").  `workspace` (uint8) is
    optional; one that is too small is refused."""
    who = "exclude_set"
    bits = _ids_ok(who, True, ids, reverse)
    if reverse is not None and reverse.shape[0] != int(num_edges):
        raise _lib.DGLAMDError("%s: the reverse map must have one entry per edge" % who)
    n, dev = ids.shape[0], ids.device
    out = torch.empty(2 * n if reverse is not None else n, dtype=ids.dtype, device=dev)
    if n == 0:
        return out
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    check_call(LIB.dgla_exclude_set(bits, _ptr(ids), n, _ptr(reverse), int(num_edges), _ptr(out), _ptr(flags),
                                    *_ws(workspace), _stream(ids)))
    if int(flags.item()) & EXCLUDE_OUT_OF_RANGE:
        raise _lib.DGLAMDError("%s: edge id out of range" % who)
    return out


def exclude_set_host(ids, num_edges, reverse=None):
    """:func:`exclude_set` run by the CPU on CPU tensors (dgla_exclude_set_host).  Returns ``(x, flags)`` and raises
    nothing for an id out of range: the flag word is the caller's to read.  Needs no GPU."""
    bits = _ids_ok("exclude_set_host", False, ids, reverse)
    n = ids.shape[0]
    out = torch.empty(2 * n if reverse is not None else n, dtype=ids.dtype)
    flags = ctypes.c_int32(0)
    check_call(LIB.dgla_exclude_set_host(bits, _ptr(ids), n, _ptr(reverse), int(num_edges), _ptr(out), ctypes.byref(flags)))
    return out, flags.value


def frontier_exclude(indptr, src, eids, x, workspace=None):
    """Drops the entries of a sampled frontier whose edge id is in the sorted set `x` (dgla_frontier_exclude).  The
    frontier is the CSR over the seeds that :func:`sample_neighbors` returns.  Returns ``(out_indptr, out_src,
    out_eids)`` with the outputs allocated at the frontier's size: the first ``out_indptr[-1]`` entries are the result.
    Nothing is read back."""
    who = "frontier_exclude"
    bits = _ids_ok(who, True, indptr, src, eids, x)
    nr, nnz = indptr.shape[0] - 1, src.shape[0]
    if nr < 0 or eids.shape[0] != nnz:
        raise _lib.DGLAMDError("%s: indptr needs at least one entry, src and eids one length" % who)
    out_indptr, out_src, out_eids = torch.empty_like(indptr), torch.empty_like(src), torch.empty_like(eids)
    check_call(LIB.dgla_frontier_exclude(bits, _ptr(indptr), _ptr(src), _ptr(eids), nr, nnz, _ptr(x), x.shape[0],
                                         _ptr(out_indptr), _ptr(out_src), _ptr(out_eids), *_ws(workspace), _stream(indptr)))
    return out_indptr, out_src, out_eids


def frontier_exclude_host(indptr, src, eids, x):
    """:func:`frontier_exclude` run by the CPU on CPU tensors (dgla_frontier_exclude_host); the outputs are cut to the
    result's length.  Needs no GPU."""
    who = "frontier_exclude_host"
    bits = _ids_ok(who, False, indptr, src, eids, x)
    nr, nnz = indptr.shape[0] - 1, src.shape[0]
    if nr < 0 or eids.shape[0] != nnz:
        raise _lib.DGLAMDError("%s: indptr needs at least one entry, src and eids one length" % who)
    out_indptr, out_src, out_eids = torch.empty_like(indptr), torch.empty_like(src), torch.empty_like(eids)
    check_call(LIB.dgla_frontier_exclude_host(bits, _ptr(indptr), _ptr(src), _ptr(eids), nr, nnz, _ptr(x), x.shape[0],
                                              _ptr(out_indptr), _ptr(out_src), _ptr(out_eids)))
    total = int(out_indptr[-1])
    return out_indptr, out_src[:total], out_eids[:total]


def compact_nodes(preserve, ends, node_map, workspace=None):
    """The compact node space of one node type (dgla_compact_nodes): ``(local, nodes)`` with ``nodes`` = `preserve` in
    the order given (a repeated id at its first position), then the other ids of `ends` ascending, and ``local[e]`` the
    index of ``ends[e]`` in it.  `node_map` is the type's int32 scratch, all -1 before and after, refusals included.  The
    node count and the flag word come back in ONE read-back; an id outside the map raises ``DGLAMDError`` ("node id out
    of range")."""
    who = "compact_nodes"
    bits = _ids_ok(who, True, preserve, ends)
    if node_map.dtype != torch.int32 or node_map.dim() != 1 or not node_map.is_contiguous() or node_map.device != ends.device:
        raise _lib.DGLAMDError("%s: the node map must be a contiguous 1-D int32 tensor on the ids' device" % who)
    np_, ne, dev, dt = preserve.shape[0], ends.shape[0], ends.device, ends.dtype
    local = torch.empty(ne, dtype=dt, device=dev)
    nodes = torch.empty(np_ + ne, dtype=dt, device=dev)
    words = torch.zeros(2, dtype=torch.int64, device=dev)       # [node count, flags (its low int32)]
    check_call(LIB.dgla_compact_nodes(bits, _ptr(preserve), np_, _ptr(ends), ne, _ptr(node_map), node_map.shape[0], _ptr(local),
                                      _ptr(nodes), words.data_ptr(), words.data_ptr() + 8, *_ws(workspace), _stream(ends)))
    num, fl = words.tolist()
    if fl & EXCLUDE_OUT_OF_RANGE:
        raise _lib.DGLAMDError("%s: node id out of range" % who)
    return local, nodes[:num]


def compact_nodes_host(preserve, ends, num_nodes):
    """:func:`compact_nodes` run by the CPU on CPU tensors (dgla_compact_nodes_host).  Returns ``(local, nodes,
    flags)``.  Needs no GPU."""
    bits = _ids_ok("compact_nodes_host", False, preserve, ends)
    np_, ne, dt = preserve.shape[0], ends.shape[0], ends.dtype
    local, nodes = torch.empty(ne, dtype=dt), torch.empty(np_ + ne, dtype=dt)
    num, flags = ctypes.c_int64(0), ctypes.c_int32(0)
    check_call(LIB.dgla_compact_nodes_host(bits, _ptr(preserve), np_, _ptr(ends), ne, int(num_nodes), _ptr(local), _ptr(nodes),
                                           ctypes.byref(num), ctypes.byref(flags)))
    return local, nodes[:num.value], flags.value


TRAVERSE_BFS_NODES, TRAVERSE_BFS_EDGES, TRAVERSE_TOPO_NODES = 0, 1, 2     # the modes of dgla_traverse (include/dgl_amd.h)


def _traverse_args(who, mode, csr, opposite, sources, gpu):
    """The arguments the two traversal entry points share, and the outputs: ``(args, ids, num_ids, num_sections,
    sections)``."""
    indptr = csr._keep[0]
    _all_on(gpu, who, indptr, sources, None if opposite is None else opposite._keep[0])
    ns = 0
    if mode != TRAVERSE_TOPO_NODES:
        _id_tensor_ok(who, "sources", sources, indptr)
        ns = sources.shape[0]
    cap = csr.num_rows + (ns if mode == TRAVERSE_BFS_NODES else 0)
    ids = torch.empty(cap, dtype=indptr.dtype, device=indptr.device)
    sections = (ctypes.c_int64 * max(cap, 1))()
    num_ids, num_sections = ctypes.c_int64(0), ctypes.c_int64(0)
    args = [int(mode), ctypes.byref(csr), None if opposite is None else ctypes.byref(opposite), _ptr(sources), ns, _ptr(ids),
            sections, ctypes.byref(num_ids), ctypes.byref(num_sections)]
    return args, ids, num_ids, num_sections, sections


def traverse_workspace_bytes(idtype, num_nodes):
    """The bytes of the optional workspace of :func:`traverse` (dgla_traverse_workspace_bytes; host query)."""
    return int(LIB.dgla_traverse_workspace_bytes(_id_bits(idtype), int(num_nodes)))


def traverse(mode, csr, opposite=None, sources=None, workspace=None):
    """The frontiers of a BFS or of the topological order over the square CSR `csr` (dgla_traverse; the rule:
    include/dgl_amd.h "Graph traversal"): returns ``(ids, sections)``, `ids` in the csr's id type on its device holding
    the frontiers one after the other and `sections` the Python list of their sizes.  `mode` is TRAVERSE_BFS_NODES
    (node ids, the sources first), TRAVERSE_BFS_EDGES (tree-edge ids) or TRAVERSE_TOPO_NODES (node ids; `opposite` is
    the CSR of the other direction, whose row lengths are the counts).  Only sizes come back to the host: 24 bytes per
    level.  `workspace` (uint8, :func:`traverse_workspace_bytes`) is optional."""
    args, ids, num_ids, num_sections, sections = _traverse_args("traverse", mode, csr, opposite, sources, True)
    check_call(LIB.dgla_traverse(*args, *_ws(workspace), _stream(csr._keep[0])))
    return ids[:num_ids.value], list(sections[:num_sections.value])


def traverse_host(mode, csr, opposite=None, sources=None):
    """:func:`traverse` run by the CPU on CPU tensors (dgla_traverse_host; CSRs built with :func:`host_csr`): the same
    rule compiled for the host, bit for bit what the kernels write.  Needs no GPU."""
    args, ids, num_ids, num_sections, sections = _traverse_args("traverse_host", mode, csr, opposite, sources, False)
    check_call(LIB.dgla_traverse_host(*args))
    return ids[:num_ids.value], list(sections[:num_sections.value])


_TOPK_DTYPES = dict(_DTYPES)       # the weight types of dgla_select_topk: dgla_dtype, DGLA_TOPK_I32, DGLA_TOPK_I64
_TOPK_DTYPES.update({torch.int32: 4, torch.int64: 5})


def select_topk_max_picks():
    """The largest number of picks one row may yield (dgla_select_topk_max_picks; host query)."""
    return int(LIB.dgla_select_topk_max_picks())


def select_topk_workspace_bytes(idtype, num_seeds):
    """The bytes of the optional workspace of :func:`select_topk` (dgla_select_topk_workspace_bytes; host query)."""
    return int(LIB.dgla_select_topk_workspace_bytes(_id_bits(idtype), int(num_seeds)))


def _topk_args(who, csr, weight, seeds, k, ascending, gpu):
    """The checks the two top-k entry points share, and their leading arguments."""
    indptr = csr._keep[0]
    _all_on(gpu, who, indptr, weight, seeds)
    if weight.dtype not in _TOPK_DTYPES:
        raise _lib.DGLAMDError("%s: unsupported weight dtype %s (fp32, fp64, fp16, bf16, int32 and int64 are accepted)"
                               % (who, weight.dtype))
    if weight.dim() != 1 or not weight.is_contiguous() or weight.shape[0] != csr.nnz or weight.device != indptr.device:
        raise _lib.DGLAMDError("%s: weight must be a contiguous 1-D tensor with one value per edge on the csr's device" % who)
    _id_tensor_ok(who, "seeds", seeds, indptr)
    return [ctypes.byref(csr), _ptr(weight), _TOPK_DTYPES[weight.dtype], _ptr(seeds), seeds.shape[0], int(k),
            1 if ascending else 0]


def select_topk(csr, weight, seeds, k, ascending=False, workspace=None):
    """For every seed row of `csr` the ``min(k, deg)`` entries with the largest (``ascending``: smallest) weight, best
    first (dgla_select_topk; the rule: include/dgl_amd.h "Top-k neighbour selection").  `weight` has one value per EDGE
    ID.  Returns ``(indptr, nbr, eids)``, a CSR over the seeds.  For ``0 <= k <= 1024`` the outputs are allocated at
    ``num_seeds * k``, the first ``indptr[-1]`` entries are the result and nothing is read back; for ``k = -1`` or
    ``k > 1024`` the sizes come first and the outputs have the result's length.  `workspace` (uint8,
    :func:`select_topk_workspace_bytes`) is optional."""
    args = _topk_args("select_topk", csr, weight, seeds, k, ascending, True)
    n, dev, dt = seeds.shape[0], seeds.device, seeds.dtype
    indptr = torch.empty(n + 1, dtype=dt, device=dev)
    wp, wb = _ws(workspace)
    st = _stream(seeds)
    if 0 <= k <= select_topk_max_picks():
        cap = n * int(k)
    else:
        check_call(LIB.dgla_select_topk(*args, indptr.data_ptr(), None, None, wp, wb, st))
        cap = int(indptr[-1])
    nbr = torch.empty(cap, dtype=dt, device=dev)
    eids = torch.empty(cap, dtype=dt, device=dev)
    check_call(LIB.dgla_select_topk(*args, indptr.data_ptr(), nbr.data_ptr(), eids.data_ptr(), wp, wb, st))
    return indptr, nbr, eids


def select_topk_host(csr, weight, seeds, k, ascending=False):
    """:func:`select_topk` run by the CPU on CPU tensors (dgla_select_topk_host; CSRs built with :func:`host_csr`): the
    same rule compiled for the host, bit for bit what the kernels write.  The outputs have the result's length.  Needs
    no GPU."""
    args = _topk_args("select_topk_host", csr, weight, seeds, k, ascending, False)
    n, dt = seeds.shape[0], seeds.dtype
    indptr = torch.empty(n + 1, dtype=dt)
    check_call(LIB.dgla_select_topk_host(*args, indptr.data_ptr(), None, None))
    total = int(indptr[-1])
    nbr, eids = torch.empty(total, dtype=dt), torch.empty(total, dtype=dt)
    check_call(LIB.dgla_select_topk_host(*args, indptr.data_ptr(), nbr.data_ptr(), eids.data_ptr()))
    return indptr, nbr, eids


def pinsage_max_samples(idtype=torch.int64):
    """The largest ``num_samples_per_node`` the selection kernel accepts for ids of `idtype` (host query)."""
    return int(LIB.dgla_pinsage_max_samples(_id_bits(idtype)))


def pinsage_size_classes():
    """The largest ``num_samples_per_node`` of every size class of the selection kernel, ascending (host query)."""
    buf = (ctypes.c_int64 * 8)()
    n = LIB.dgla_pinsage_size_classes(buf, 8)
    return [int(buf[i]) for i in range(n)]


def _pinsage_args(who, src, dst, num_samples_per_node, k, device):
    """The argument errors the three selection entry points share, raised before any launch and before the device check
    (so they can be met without a GPU).  Returns ``(id width, num_dst, S, k, min(k, S))``."""
    if src.dtype != dst.dtype or src.dtype not in (torch.int32, torch.int64):
        raise _lib.DGLAMDError("%s: src and dst must both be int32 or both int64, got %s and %s" % (who, src.dtype, dst.dtype))
    if src.dim() != 1 or dst.shape != src.shape or not src.is_contiguous() or not dst.is_contiguous():
        raise _lib.DGLAMDError("%s: src and dst must be contiguous 1-D tensors of one length" % who)
    S, k = int(num_samples_per_node), int(k)
    if S < 1:
        raise _lib.DGLAMDError("%s: num_samples_per_node must be at least 1, got %d" % (who, S))
    if k < 1:
        raise _lib.DGLAMDError("%s: k must be at least 1, got %d" % (who, k))
    if src.shape[0] % S:
        raise _lib.DGLAMDError("%s: the length of src (%d) is not a multiple of num_samples_per_node (%d)"
                               % (who, src.shape[0], S))
    if device and S > pinsage_max_samples(src.dtype):
        raise _lib.DGLAMDError("%s: num_samples_per_node = %d is above the largest segment the kernel holds in LDS (%d); "
                               "there is no CPU fallback" % (who, S, pinsage_max_samples(src.dtype)))
    return _idbits(src), src.shape[0] // S, S, k, min(k, S)


def select_pinsage_neighbors_padded(src, dst, num_samples_per_node, k):
    """The visit-count top-k of every segment of ``num_samples_per_node`` entries of `src` in its static shape
    (dgla_pinsage_select_padded; the rule: include/dgl_amd.h).  Returns ``(src [n, k'], counts [n, k'], num [n])`` with
    k' = min(k, num_samples_per_node), -1 / 0 in the unused slots.  Nothing is read back."""
    bits, n, S, k, kp = _pinsage_args("select_pinsage_neighbors_padded", src, dst, num_samples_per_node, k, True)
    _require_gpu(src)
    _require_gpu(dst)
    out_src = torch.empty((n, kp), dtype=src.dtype, device=src.device)
    out_cnt = torch.empty((n, kp), dtype=src.dtype, device=src.device)
    out_num = torch.empty(n, dtype=src.dtype, device=src.device)
    check_call(LIB.dgla_pinsage_select_padded(bits, _ptr(src), _ptr(dst), n, S, k, _ptr(out_src), _ptr(out_cnt),
                                              _ptr(out_num), None, _stream(src)))
    return out_src, out_cnt, out_num


def select_pinsage_neighbors(src, dst, num_samples_per_node, k):
    """``_select_pinsage_neighbors`` of python/dgl/sampling/pinsage.py on the device (dgla_pinsage_select_count + _fill):
    ``(src, dst, counts)`` of the kept neighbours, segments in input order, ranked by (count, id) descending inside a
    segment.  Reading the total is the one host synchronisation."""
    bits, n, S, k, kp = _pinsage_args("select_pinsage_neighbors", src, dst, num_samples_per_node, k, True)
    _require_gpu(src)
    _require_gpu(dst)
    need = LIB.dgla_pinsage_select_workspace_bytes(bits, n, S, k)
    ws = _workspace(need, src.device)
    total = ctypes.c_int64(0)
    st = _stream(src)
    check_call(LIB.dgla_pinsage_select_count(bits, _ptr(src), _ptr(dst), n, S, k, ctypes.byref(total), _ptr(ws), need, st))
    res = [torch.empty(total.value, dtype=src.dtype, device=src.device) for _ in range(3)]
    check_call(LIB.dgla_pinsage_select_fill(bits, n, S, k, _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(ws), need, st))
    return tuple(res)


def select_pinsage_neighbors_host(src, dst, num_samples_per_node, k):
    """:func:`select_pinsage_neighbors` run by the CPU on CPU tensors (dgla_pinsage_select_host): a plain restatement
    of the rule, what the kernel is tested against.  Needs no GPU and accepts any ``num_samples_per_node``."""
    bits, n, S, k, kp = _pinsage_args("select_pinsage_neighbors_host", src, dst, num_samples_per_node, k, False)
    _all_on(False, "select_pinsage_neighbors_host", src, dst)
    res = [torch.empty(n * kp, dtype=src.dtype) for _ in range(3)]
    total = ctypes.c_int64(0)
    check_call(LIB.dgla_pinsage_select_host(bits, _ptr(src), _ptr(dst), n, S, k, _ptr(res[0]), _ptr(res[1]), _ptr(res[2]),
                                            ctypes.byref(total)))
    return tuple(r[:total.value].clone() for r in res)


def to_block(seeds, src, node_map):
    """Block-local renumbering of `src` (dgla_to_block).  Returns ``(local_src, src_nodes,
    num_src)``; reading ``num_src`` back is the one host synchronisation of block building
    (the reference synchronises at the same place, cuda_to_block.cu).  The node count is known here
    (``node_map`` has one entry per node), so the sort inside looks at the used key bits only
    (dgla_to_block_padded with every seed valid: 3 radix passes instead of 8 for int64 ids)."""
    _require_gpu(src)
    n, nnz = seeds.shape[0], src.shape[0]
    dev, dt = seeds.device, seeds.dtype
    local = torch.empty(nnz, dtype=dt, device=dev)
    src_nodes = torch.empty(n + nnz, dtype=dt, device=dev)
    num = torch.empty(1, dtype=torch.int64, device=dev)
    if n > 0:
        ws = _workspace(max(1, LIB.dgla_to_block_workspace_bytes(_idbits(seeds), nnz)), dev)
        check_call(LIB.dgla_to_block_padded(_idbits(seeds), seeds.data_ptr(), n, None, _ptr(src), nnz,
                                            int(node_map.shape[0]), node_map.data_ptr(), _ptr(local),
                                            src_nodes.data_ptr(), num.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _stream(seeds)))
    else:
        check_call(LIB.dgla_to_block(_idbits(seeds), seeds.data_ptr(), n, _ptr(src), nnz, node_map.data_ptr(),
                                     _ptr(local), src_nodes.data_ptr(), num.data_ptr(), None, 0, _stream(seeds)))
    k = int(num.item())
    return local, src_nodes[:k], k


SINK_ROWS = 64  # sink rows of a padded block (dgla_sample_neighbors_padded)


def sample_neighbors_padded(csr, seeds, num_valid, fanout, replace=False, rng_seed=0, rng_counter=None,
                            sink_rows=SINK_ROWS, prob=None):
    """Static-shape form of :func:`sample_neighbors` (dgla_sample_neighbors_padded): nothing is read
    back.  ``seeds`` has ``n`` slots of which the first ``num_valid`` (int64 device tensor of one
    element, or None = all) are real.  Returns ``(indptr[n + 1 + sink_rows], src[n * fanout],
    eids[n * fanout])``: the real rows' picks first, then the edges of ``sink_rows`` extra SINK rows
    (rows ``n ..``) pointing at the real seeds in turn.  ``rng_counter`` (int64 device tensor) is added to the draw counter on the device,
    so a captured call samples afresh on every replay once the caller bumps it."""
    _require_gpu(seeds)
    n = seeds.shape[0]
    dev, dt = seeds.device, seeds.dtype
    cap = n * int(fanout)
    indptr = torch.empty(n + 1 + int(sink_rows), dtype=dt, device=dev)
    src = torch.empty(cap, dtype=dt, device=dev)
    eids = torch.empty(cap, dtype=dt, device=dev)
    ws = _workspace(max(1, LIB.dgla_sample_neighbors_workspace_bytes(_idbits(seeds), n)), dev)
    if prob is not None:
        _require_gpu(prob)
        _prob_ok(prob)
    check_call(LIB.dgla_sample_neighbors_padded(
        ctypes.byref(csr), _ptr(prob), _DTYPES[prob.dtype] if prob is not None else 0, seeds.data_ptr(), n,
        _ptr(num_valid), int(fanout), 1 if replace else 0,
        _u64(rng_seed), _ptr(rng_counter), int(sink_rows), indptr.data_ptr(), src.data_ptr(),
        eids.data_ptr(),
        ws.data_ptr(), ws.numel(), _stream(seeds)))
    return indptr, src, eids


def to_block_padded(seeds, num_valid, src, node_map, fill=0, num_nodes=0):
    """Static-shape form of :func:`to_block` (dgla_to_block_padded).  Returns ``(local_src,
    src_nodes[n + nnz], num_src)`` with ``num_src`` an int64 DEVICE tensor; entries of ``src_nodes``
    past it hold ``fill`` (a valid node id).  Only the first ``num_valid`` seeds claim a local id."""
    _require_gpu(src)
    n, nnz = seeds.shape[0], src.shape[0]
    dev, dt = seeds.device, seeds.dtype
    local = torch.empty(nnz, dtype=dt, device=dev)
    src_nodes = torch.full((n + nnz,), int(fill), dtype=dt, device=dev)
    num = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(max(1, LIB.dgla_to_block_workspace_bytes(_idbits(seeds), nnz)), dev)
    check_call(LIB.dgla_to_block_padded(_idbits(seeds), seeds.data_ptr(), n, _ptr(num_valid), _ptr(src), nnz,
                                        int(num_nodes), node_map.data_ptr(), _ptr(local), src_nodes.data_ptr(), num.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream(seeds)))
    return local, src_nodes, num


def gather_rows(src, idx, out=None):
    """out[i] = src[idx[i]] along dim 0 (dgla_gather_rows): the pack kernel of the halo exchange."""
    _require_gpu(src)
    _require_gpu(idx)
    if not src.is_contiguous():
        raise _lib.DGLAMDError("gather_rows: src must be contiguous")
    idx = idx.contiguous()
    if out is None:
        out = torch.empty((idx.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    elif not out.is_contiguous() or out.shape[0] != idx.shape[0] or out.shape[1:] != src.shape[1:] \
            or out.dtype != src.dtype:
        raise _lib.DGLAMDError("gather_rows: out must be contiguous with one row per index")
    row_bytes = src.element_size()
    for d in src.shape[1:]:
        row_bytes *= int(d)
    check_call(LIB.dgla_gather_rows(_idbits(idx), src.data_ptr(), idx.data_ptr(), idx.shape[0],
                                    row_bytes, out.data_ptr(), _stream(out)))
    return out


def partition_map(mode, num_parts, part_range, idx, want_part=True, want_local=True):
    """(part, local) ids of the global ids `idx` under a remainder (mode 0) or range (mode 1)
    partition (dgla_partition_map)."""
    _require_gpu(idx)
    idx = idx.contiguous()
    part = torch.empty_like(idx) if want_part else None
    local = torch.empty_like(idx) if want_local else None
    check_call(LIB.dgla_partition_map(_idbits(idx), int(mode), int(num_parts), _ptr(part_range),
                                      idx.data_ptr(), idx.shape[0], _ptr(part), _ptr(local),
                                      _stream(idx)))
    return part, local


def partition_to_global(mode, num_parts, part_range, local_idx, part_id):
    _require_gpu(local_idx)
    local_idx = local_idx.contiguous()
    out = torch.empty_like(local_idx)
    check_call(LIB.dgla_partition_to_global(_idbits(local_idx), int(mode), int(num_parts),
                                            _ptr(part_range), local_idx.data_ptr(),
                                            local_idx.shape[0], int(part_id), out.data_ptr(),
                                            _stream(out)))
    return out


def scatter_rows(src, idx, out):
    """out[idx[i]] = src[i] along dim 0 (dgla_scatter_rows)."""
    _require_gpu(src)
    _require_gpu(idx)
    if not (src.is_contiguous() and out.is_contiguous() and idx.is_contiguous()):
        raise _lib.DGLAMDError("scatter_rows: tensors must be contiguous")
    row_bytes = src.element_size()
    for d in src.shape[1:]:
        row_bytes *= int(d)
    check_call(LIB.dgla_scatter_rows(_idbits(idx), src.data_ptr(), idx.data_ptr(), idx.shape[0],
                                     row_bytes, out.data_ptr(), _stream(out)))
    return out
