"""Host-side checks of the sparse x sparse entry points (csrc/csr_mm.hip): registry names, argument errors across the
C ABI, the row-class query, the workspace bound, the Python names, and the refusal of CPU tensors.  No GPU needed: every
call here fails (or answers) before anything is launched."""
import ctypes

import pytest
import torch

import dgl_amd
from dgl_amd import DGLAMDError, _capi, _ffi, _lib, sparse_kernels

LIB = _lib.LIB
FAKE = 0x1000   # a non-null "device pointer" for descriptors that are rejected before anything reads through them


def _csr(rows, cols, nnz, bits=64, ptr=FAKE):
    return _lib.CSR(rows, cols, nnz, bits, ptr, ptr, None)


def _err():
    return LIB.dgla_last_error().decode()


def test_registry_lists_the_five_names():
    names = set(_ffi.list_global_func_names())
    for n in ("dgl_amd._CAPI_CSRMMCount", "dgl_amd._CAPI_CSRMMFill", "dgl_amd._CAPI_CSRSumCount",
              "dgl_amd._CAPI_CSRSumFill", "dgl_amd._CAPI_CSRMask"):
        assert n in names


def test_null_and_mismatched_arguments_fail_with_a_message():
    nnz = ctypes.c_int64(-7)
    a, b = _csr(3, 4, 5), _csr(4, 6, 5)
    assert LIB.dgla_csr_mm_count(None, ctypes.byref(b), FAKE, ctypes.byref(nnz), None, 0, None) == -1 and "null" in _err()
    assert LIB.dgla_csr_mm_count(ctypes.byref(a), None, FAKE, ctypes.byref(nnz), None, 0, None) == -1 and "null" in _err()
    assert LIB.dgla_csr_mm_count(ctypes.byref(a), ctypes.byref(b), None, ctypes.byref(nnz), None, 0, None) == -1
    assert "null" in _err()
    assert LIB.dgla_csr_mm_count(ctypes.byref(a), ctypes.byref(b), FAKE, None, None, 0, None) == -1 and "null" in _err()
    bad = _csr(5, 6, 5)   # a.num_cols != b.num_rows
    assert LIB.dgla_csr_mm_count(ctypes.byref(a), ctypes.byref(bad), FAKE, ctypes.byref(nnz), None, 0, None) == -1
    assert "4 columns" in _err() and "5 rows" in _err()
    b32 = _csr(4, 6, 5, bits=32)   # mixed id widths
    assert LIB.dgla_csr_mm_count(ctypes.byref(a), ctypes.byref(b32), FAKE, ctypes.byref(nnz), None, 0, None) == -1
    assert "id types" in _err()
    assert LIB.dgla_csr_mm_fill(ctypes.byref(a), 0, FAKE, ctypes.byref(bad), FAKE, FAKE, FAKE, FAKE, None, 0, None) == -1
    assert LIB.dgla_csr_mm_fill(ctypes.byref(a), 0, None, ctypes.byref(b), FAKE, FAKE, FAKE, FAKE, None, 0, None) == -1
    assert "weights" in _err()
    assert nnz.value == -7   # untouched by failed calls
    # the sum: no operands, NULL table, different shapes
    ops = (ctypes.POINTER(_lib.CSR) * 2)(ctypes.pointer(a), ctypes.pointer(_csr(3, 5, 2)))
    assert LIB.dgla_csr_sum_count(None, 2, FAKE, ctypes.byref(nnz), None, 0, None) == -1 and "operand" in _err()
    assert LIB.dgla_csr_sum_count(ops, 0, FAKE, ctypes.byref(nnz), None, 0, None) == -1 and "operand" in _err()
    assert LIB.dgla_csr_sum_count(ops, 2, FAKE, ctypes.byref(nnz), None, 0, None) == -1 and "shapes" in _err()
    assert LIB.dgla_csr_sum_fill(ops, 2, 0, None, FAKE, FAKE, FAKE, None, 0, None) == -1
    # the mask: NULL operands, different shapes, mixed id widths
    coo = _lib.COO(3, 4, 2, 64, FAKE, FAKE, None)
    assert LIB.dgla_csr_mask(None, 0, FAKE, ctypes.byref(coo), FAKE, None) == -1 and "null" in _err()
    assert LIB.dgla_csr_mask(ctypes.byref(a), 0, FAKE, None, FAKE, None) == -1 and "null" in _err()
    assert LIB.dgla_csr_mask(ctypes.byref(a), 0, FAKE, ctypes.byref(_lib.COO(3, 5, 2, 64, FAKE, FAKE, None)), FAKE, None) == -1
    assert "shapes" in _err()
    assert LIB.dgla_csr_mask(ctypes.byref(a), 0, FAKE, ctypes.byref(_lib.COO(3, 4, 2, 32, FAKE, FAKE, None)), FAKE, None) == -1
    assert "id types" in _err()
    assert LIB.dgla_csr_mask(ctypes.byref(a), 0, FAKE, ctypes.byref(coo), None, None) == -1 and "out" in _err()


def test_row_classes_ascend():
    b = _capi.csr_mm_row_classes()
    assert len(b) == 2 and 0 < b[0] < b[1]
    one = (ctypes.c_int64 * 1)(-1)
    assert LIB.dgla_csr_mm_row_classes(one, 1) == 2 and one[0] == b[0]   # `max` is honoured, the count is still returned
    assert LIB.dgla_csr_mm_row_classes(None, 0) == 2


def test_workspace_bound_is_monotone():
    def need(rows, nnz):
        a, b = _csr(rows, 50, nnz), _csr(50, 60, nnz)
        return LIB.dgla_csr_mm_workspace_bytes(ctypes.byref(a), ctypes.byref(b))

    by_nnz = [need(1000, n) for n in (0, 1, 10, 1000, 10 ** 6, 10 ** 9)]
    assert all(x <= y for x, y in zip(by_nnz, by_nnz[1:])) and by_nnz[0] > 0
    by_rows = [need(r, 100) for r in (0, 1, 1000, 10 ** 6)]
    assert all(x <= y for x, y in zip(by_rows, by_rows[1:])) and by_rows[-1] >= 2 * 8 * 10 ** 6
    assert by_rows[-1] < 64 * 10 ** 6   # a few words per row: terms are never expanded into global memory
    ops = (ctypes.POINTER(_lib.CSR) * 1)(ctypes.pointer(_csr(1000, 50, 10)))
    assert LIB.dgla_csr_sum_workspace_bytes(ops, 1) >= need(1000, 10)


def test_python_names_exist():
    for mod, names in ((dgl_amd, ("adj_product_graph", "adj_sum_graph")),
                       (sparse_kernels, ("_csrmm", "_csrsum", "_csrmask"))):
        for n in names:
            assert callable(getattr(mod, n))
    from dgl_amd import autograd
    for n in ("CSRMM", "CSRSum", "CSRMask", "csrmm", "csrsum", "csrmask"):
        assert hasattr(autograd, n)


def test_empty_list_raises_value_error():
    with pytest.raises(ValueError):
        dgl_amd.adj_sum_graph([], "w")


def _cpu_graph():
    g = dgl_amd.heterograph({("A", "AB", "B"): (torch.tensor([0, 1, 2]), torch.tensor([1, 0, 3]))},
                            num_nodes_dict={"A": 3, "B": 4})
    g.edata["w"] = torch.ones(3)
    return g


def test_cpu_tensors_are_refused():
    g = _cpu_graph()
    h = dgl_amd.heterograph({("B", "BA", "A"): (torch.tensor([0, 3]), torch.tensor([1, 2]))}, num_nodes_dict={"A": 3, "B": 4})
    h.edata["w"] = torch.ones(2)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        sparse_kernels._csrmm(g._graph, g.edata["w"], h._graph, h.edata["w"], 1)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        sparse_kernels._csrsum([g._graph], [g.edata["w"]])
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        sparse_kernels._csrmask(g._graph, g.edata["w"], g._graph)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        dgl_amd.adj_product_graph(g, h, "w")
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        dgl_amd.adj_sum_graph([g], "w")
