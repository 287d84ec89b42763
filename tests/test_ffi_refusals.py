"""Every refusal of the FFI registry (dgl_amd/csrc/ffi_registry.hip), by its exact message.

TABLE holds (registered name, arguments, expected message).  Each row is a call the registry refuses
before it reaches a ``dgla_*`` launch, so nothing runs on a device and the test needs none: with a GPU
the arrays are tiny device tensors, without one they are host tensors whose ``ctx.device_type`` says
ROCm (a call that slipped through would end in HIP's "no device" error, not in a kernel).

Arguments are written as small specs (``A`` an array, ``G`` a unit graph, ``H`` a heterograph, ``LH`` a
``_List`` handle) that are made fresh for each call and released after it.
"""
import copy
import ctypes

import pytest
import torch

from dgl_amd import _ffi, _lib

_GPU = torch.cuda.is_available()
_TORCH = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64, "u8": torch.uint8}
S, D = "sparse._CAPI_DGLKernel", "dgl_amd._CAPI_"


class _Arr(_ffi.NDArray):
    __slots__ = ("_strides",)


class A:
    """A zero-filled array of at most a few dozen elements."""

    def __init__(self, *shape, dt="f32"):
        self.shape, self.dtype, self.on_host, self.is_strided = shape, dt, False, False

    def _but(self, **kw):
        c = copy.copy(self)
        c.__dict__.update(kw)
        return c

    def host(self):
        return self._but(on_host=True)

    def strided(self):
        return self._but(is_strided=True)

    def dt(self, dt):
        return self._but(dtype=dt)

    def make(self, cleanup):
        numel = 1
        for s in self.shape:
            numel *= s
        t = torch.zeros(2 * numel, dtype=_TORCH[self.dtype], device="cuda" if _GPU and not self.on_host else "cpu")
        a = _Arr.__new__(_Arr)
        a.tensor = t
        nd = len(self.shape)
        a._shape = (ctypes.c_int64 * nd)(*self.shape)
        a._strides = None
        if self.is_strided:  # twice the contiguous strides: never contiguous, and inside the 2 * numel buffer
            st, run = [], 1
            for s in reversed(self.shape):
                st.insert(0, 2 * run)
                run *= s
            a._strides = (ctypes.c_int64 * nd)(*st)
        code, bits = _ffi._DT[t.dtype]
        ctx = _ffi.DGLContext(_ffi.kDGLCPU, 0) if self.on_host else _ffi.DGLContext(_ffi.kDGLROCM, 0)
        a.arr = _ffi.DGLArray(t.data_ptr() if numel else None, ctx, nd, _ffi.DGLDataType(code, bits, 1), a._shape,
                              a._strides, 0)
        return a


def F(name):
    return _ffi.get_global_func(name)


class G:
    """A unit graph of 4 source nodes, 3 destination nodes and 5 edges with the named formats set."""

    def __init__(self, *fmts, bits=32):
        self.fmts, self.bits = fmts, bits

    def make(self, cleanup):
        h = F(D + "UnitGraphCreate")(4, 3, self.bits)
        cleanup.append(lambda: F(D + "UnitGraphFree")(h))
        ids = "i%d" % self.bits
        for f in self.fmts:
            x = A({"coo": 5, "csr": 5, "csc": 4}[f], dt=ids).make(cleanup)
            y = A(5, dt=ids).make(cleanup)
            cleanup.append(lambda x=x, y=y: None)  # the graph borrows them
            F(D + "UnitGraphSet" + f.upper())(h, x, y, None)
        return h


class H:
    """A heterograph of two node types with one relation 0 -> 1 over `g`."""

    def __init__(self, g):
        self.g = g

    def make(self, cleanup):
        g = self.g.make(cleanup)
        h = F(D + "HeteroGraphCreate")(2, g, 0, 1)
        cleanup.append(lambda: _lib.LIB.DGLObjectFree(ctypes.c_void_p(h.handle)))
        return h


class LH:
    """The handle of an empty `_List`."""

    def make(self, cleanup):
        h = F("_List")()
        cleanup.append(lambda: _lib.LIB.DGLObjectFree(ctypes.c_void_p(h.handle)))
        return h


def _make(x, cleanup):
    if isinstance(x, (A, G, H, LH)):
        return x.make(cleanup)
    if isinstance(x, list):
        return [_make(y, cleanup) for y in x]
    return x


def _refused(name, args):
    cleanup = []
    try:
        with pytest.raises(_lib.DGLAMDError) as ei:
            F(name)(*[_make(x, cleanup) for x in args])
        return str(ei.value)
    finally:
        for c in reversed(cleanup):  # handles before the arrays they borrow
            c()


TABLE = []
WRONG_HANDLE = []


def row(name, args, msg):
    TABLE.append((name, tuple(args), msg))


def sub(base, i, x):
    return base[:i] + (x,) + base[i + 1:]


_WRONG = {"i": ("x", "expected an integer"), "f": ("x", "expected a number"), "s": (1, "expected a string"),
          "h": (1, "expected an object handle"), "a": (1, "expected an NDArray"), "l": (1, "expected a list (see _List)")}


def reader(name, kinds, base, optional=0):
    """A wrong type code and a missing argument at every position of `name`; `kinds` has one letter per position
    (i integer, f number, s string, h handle, a NDArray, l list); the last `optional` positions may be left out."""
    assert len(kinds) == len(base)
    for i, k in enumerate(kinds):
        bad, what = _WRONG[k]
        row(name, sub(base, i, bad), "argument %d: %s" % (i, what))
        if i < len(kinds) - optional:
            row(name, base[:i], "argument %d is missing" % i if k == "a" else "argument %d: %s" % (i, what))


def array_check(name, base, nouns, not_gpu):
    """A host array and a strided array at every position in `nouns` ({position: noun of the message}); `not_gpu` is
    the site's wording for the former, with or without the noun in it."""
    for i, noun in nouns.items():
        row(name, sub(base, i, base[i].host()), not_gpu % noun if "%s" in not_gpu else not_gpu)
        row(name, sub(base, i, base[i].strided()), noun + " must be contiguous")


FLOAT = "feature arrays must be float16 / bfloat16 / float32 / float64"
INDEX = "index arrays must be int32 or int64"
DIFFER = "operand and output dtypes differ"
ON_GRAPH = "%s is not on the GPU device of the graph"
ON_GPU = "array is not on a GPU device"
NOT_UNIT = "argument %d: not a unit graph"
NOT_HETERO = "argument 0: expected a heterograph handle"

g_none, g_csc, g_csr, g_coo, g_all = G(), G("csc"), G("csr"), G("coo"), G("csc", "csr", "coo")
U, E, V, ARG = A(4, 3), A(5, 1), A(3, 3), A(3, 3, dt="i32")
WS = A(16, dt="u8")

# ---- unit-graph handle ---------------------------------------------------------------------------------------------
reader(D + "UnitGraphCreate", "iii", (4, 3, 32))
row(D + "UnitGraphCreate", (4, 3, 16), "idtype bits must be 32 or 64")
reader(D + "UnitGraphFree", "h", (g_none,))
for fmt, n_x in (("COO", 5), ("CSR", 5), ("CSC", 4)):
    name = D + "UnitGraphSet" + fmt
    x, y = A(n_x, dt="i32"), A(5, dt="i32")
    base = (g_none, x, y, A(5, dt="i32"))
    reader(name, "haaa", base)
    row(name, sub(base, 1, None), "index arrays are required")
    row(name, sub(base, 2, None), "index arrays are required")
    row(name, sub(base, 1, x.dt("f32")), INDEX)
    row(name, sub(base, 2, y.dt("u8")), INDEX)
    row(name, sub(base, 1, x.dt("i64")), "index dtype does not match the graph")
    row(name, sub(base, 2, y.dt("i64")), "index dtype does not match the graph")
    row(name, sub(base, 3, A(5, dt="f32")), INDEX)
    row(name, sub(base, 3, A(5, dt="i64")), "edge-id dtype does not match the graph")
    row(name, sub(base, 1, x.strided()), "indptr/row must be contiguous")
    row(name, sub(base, 2, y.strided()), "indices/col must be contiguous")
    row(name, sub(base, 1, A(n_x - 1, dt="i32")),
        "row and col must have the same length" if fmt == "COO" else "indptr must have num_rows + 1 entries")
reader(D + "UnitGraphSetWorkspace", "ha", (g_none, WS))
reader(D + "UnitGraphSetSoftmaxWorkspace", "ha", (g_none, WS))
reader(D + "UnitGraphStaticOperand", "hii", (g_none, 1, 2), optional=1)
reader(D + "SetAutoEdgeOperandMinEdges", "i", (1,))

# ---- g-SpMM --------------------------------------------------------------------------------------------------------
for n in ("SpMM", "SpMMMean", "SpMMAccumulate", "SpMMWorkspaceBytes"):
    name = S + n
    base = (g_csc, "mul", "sum", U, E, V, ARG, ARG)
    reader(name, "hssaaaaa", base, optional=2)
    row(name, base[:5] + (None,), "out array is empty")
    row(name, base[:5] + (A(0, 3),), "out array is empty")
    array_check(name, base, {3: "U_data", 4: "E_data", 5: "out", 6: "Arg_U", 7: "Arg_E"}, ON_GRAPH)
    for i in (3, 4, 5):
        row(name, sub(base, i, base[i].dt("i32")), FLOAT)
    row(name, sub(base, 3, U.dt("f64")), DIFFER)
    row(name, sub(base, 4, E.dt("f64")), DIFFER)
    row(name, sub(base, 5, V.dt("f64")), DIFFER)
row(S + "SpMM", (g_none, "mul", "sum", U, E, V), "SpMM only supports CSC and COO formats")
row(S + "SpMM", (g_csr, "mul", "sum", U, E, V), "SpMM only supports CSC and COO formats")
row(S + "SpMMMean", (g_coo, "mul", "sum", U, E, V), "SpMMMean needs the CSC format")
row(S + "SpMMAccumulate", (g_coo, "mul", "sum", U, E, V), "SpMMAccumulate needs the CSC format")

TAB, REL = A(2, dt="i64"), A(5, dt="u8")
TYPES = A(2, 2, dt="i32").host()
for n in ("SpMMStacked", "SpMMStackedWorkspaceBytes", "SpMMStackedCmp", "SpMMStackedCmpWorkspaceBytes"):
    name, cmp_ = S + n, "Cmp" in n
    if cmp_:
        base = (g_csc, "mul", "max", U, E, TAB, TAB, V, REL, TYPES, ARG, ARG, ARG, ARG)
        reader(name, "hssaaaaaaaaaaa", base)
        u, v, rel = 3, 7, 8
    else:
        base = (g_csc, "mul", U, E, TAB, TAB, V, REL)
        reader(name, "hsaaaaaa", base)
        u, v, rel = 2, 6, 7
    row(name, sub(base, 0, g_coo), "stacked SpMM needs the CSC format")
    row(name, sub(base, v, None), "out array is empty")
    row(name, sub(base, v, V.dt("i32")), FLOAT)
    array_check(name, base, {u: "operand", u + 1: "operand"}, ON_GRAPH)
    for i in (u, u + 1):
        row(name, sub(base, i, base[i].dt("i32")), FLOAT)
        row(name, sub(base, i, base[i].dt("f64")), DIFFER)
    if "Workspace" in n:
        continue
    row(name, sub(base, rel, None), "rel must be a uint8 array")
    row(name, sub(base, rel, A(5, dt="i32")), "rel must be a uint8 array")
    if cmp_:
        for bad in (None, A(2, 2, dt="i32"), TYPES.dt("i64"), A(4, dt="i32").host(), A(3, 2, dt="i32").host()):
            row(name, sub(base, 9, bad), "types must be a host int32 array of shape [2, num_rel]")
        array_check(name, base, {10: "arg array", 11: "arg array", 12: "arg array", 13: "arg array"}, ON_GRAPH)
        for i in (10, 11, 12, 13):
            row(name, sub(base, i, ARG.dt("i64")), "arg arrays must have the graph's id type")

# ---- g-SDDMM, edge softmax -----------------------------------------------------------------------------------------
LHS, RHS, OUT = A(4, 3), A(3, 3), A(5, 1)
base = (g_coo, "dot", LHS, RHS, OUT, 0, 2)
reader(S + "SDDMM", "hsaaaii", base)
row(S + "SDDMM", sub(base, 4, None), "out array is empty")
array_check(S + "SDDMM", base, {2: "array", 3: "array", 4: "array"}, ON_GRAPH)
for i in (2, 3, 4):
    row(S + "SDDMM", sub(base, i, base[i].dt("i32")), FLOAT)
    row(S + "SDDMM", sub(base, i, base[i].dt("f64")), DIFFER)
row(S + "SDDMM", sub(base, 0, g_csc), "SDDMM only supports CSR and COO formats")

reader(S + "Edge_softmaxWorkspaceBytes", "hii", (g_csc, 1, 32))
reader(S + "Edge_softmax_forward", "hsaaa", (g_csc, "copy_rhs", None, E, E))
row(S + "Edge_softmax_forward", (g_coo, "copy_rhs", None, E, E), "edge_softmax needs the CSC format")
row(S + "Edge_softmax_forward", (g_csc, "copy_rhs", None, None, E), "score / out missing")
row(S + "Edge_softmax_forward", (g_csc, "copy_rhs", None, E, None), "score / out missing")
row(S + "Edge_softmax_forward", (g_csc, "copy_rhs", None, E.dt("i32"), E), FLOAT)
reader(S + "Edge_softmax_backward", "hsaaa", (g_csc, "copy_rhs", E, E, E))
row(S + "Edge_softmax_backward", (g_coo, "copy_rhs", E, E, E), "edge_softmax needs the CSC format")
for i in (2, 3, 4):
    row(S + "Edge_softmax_backward", sub((g_csc, "copy_rhs", E, E, E), i, None), "out / sds / back missing")
row(S + "Edge_softmax_backward", (g_csc, "copy_rhs", E.dt("i32"), E, E), FLOAT)

# ---- fused GAT attention -------------------------------------------------------------------------------------------
FT, EL, ER, GOUT, MZ = A(4, 2, 3), A(4, 2, 1), A(3, 2, 1), A(3, 2, 3), A(3, 2, 2)
MIXED = "gat_attention: mixed dtypes (ft, el, er, out, dout and the gradients share one element type)"
reader(D + "GATAttentionWorkspaceBytes", "hii", (g_csc, 2, 3))
row(D + "GATAttentionWorkspaceBytes", (g_coo, 2, 3), "gat_attention needs the CSC format")


def gat(name, kinds, base, mz, no_format, required):
    """kinds: the reader's letters; every 'a' but the last (the workspace) is a required tensor, position 1 gives
    the element type and `mz` is the float32 statistics array."""
    reader(name, kinds, base)
    row(name, sub(base, 0, g_coo), no_format)
    arrays = [i for i, k in enumerate(kinds) if k == "a"]
    tensors = arrays[:-1] if base[arrays[-1]] is WS else arrays
    for i in tensors:
        row(name, sub(base, i, None), required)
    array_check(name, base, {i: "array" for i in arrays}, ON_GPU)
    row(name, sub(base, 1, base[1].dt("i32")), FLOAT)
    for i in tensors[1:]:
        row(name, sub(base, i, base[i].dt("f64")), "gat_attention: mz must be float32" if i == mz else MIXED)


gat(D + "GATAttentionForward", "haaafaaa", (g_csc, FT, EL, ER, 0.2, GOUT, MZ, WS), 6,
    "gat_attention needs the CSC format", "gat_attention: ft / el / er / out / mz are required")
gat(D + "GATAttentionTrainForward", "haaaffiaaa", (g_csc, FT, EL, ER, 0.2, 0.5, 7, GOUT, MZ, WS), 8,
    "gat_attention needs the CSC format", "gat_attention: ft / el / er / out / mz are required")
gat(D + "GATAttentionBackward", "haaaaaafaaaa", (g_all, FT, EL, ER, GOUT, MZ, GOUT, 0.2, FT, EL, ER, WS), 5,
    "gat_attention backward needs the CSC and the CSR format", "gat_attention backward: every tensor is required")
gat(D + "GATAttentionTrainBackward", "haaaaaffiaaaa", (g_all, FT, EL, ER, MZ, GOUT, 0.2, 0.5, 7, FT, EL, ER, WS), 4,
    "gat_attention backward needs the CSC and the CSR format", "gat_attention backward: every tensor is required")
gat(D + "GATAttentionWeights", "haaaffia", (g_csc, EL, ER, MZ, 0.2, 0.5, 7, A(5, 2, 1)), 3,
    "gat_attention needs the CSC format", "gat_attention_weights: el / er / mz / attn are required")
row(D + "GATAttentionBackward", sub((g_all, FT, EL, ER, GOUT, MZ, GOUT, 0.2, FT, EL, ER, WS), 0, g_csc),
    "gat_attention backward needs the CSC and the CSR format")

# ---- sparse x sparse -----------------------------------------------------------------------------------------------
NEED_CSR = "csr_mm / csr_sum / csr_mask need the CSR format of their operands"
IP, IX, W5, W7 = A(5, dt="i32"), A(7, dt="i32"), A(5), A(7)


def ids(name, base, i, noun, num_rows=True):
    row(name, sub(base, i, None), noun + " is required")
    row(name, sub(base, i, base[i].host()), ON_GPU)
    row(name, sub(base, i, base[i].strided()), noun + " must be contiguous")
    row(name, sub(base, i, base[i].dt("f32")), INDEX)
    row(name, sub(base, i, base[i].dt("i64")), noun + " must have the id type of the operands")
    if num_rows:
        row(name, sub(base, i, A(4, dt="i32")), "c_indptr must have num_rows + 1 entries")


def weights(name, base, i, noun, n):
    row(name, sub(base, i, None), noun + " is required")
    row(name, sub(base, i, base[i].host()), ON_GPU)
    row(name, sub(base, i, base[i].strided()), noun + " must be contiguous")
    row(name, sub(base, i, base[i].dt("i32")), FLOAT)
    row(name, sub(base, i, A(n, 2)), noun + " must be one scalar per edge (1-D)")
    row(name, sub(base, i, A(n, 1, 1)), noun + " must be one scalar per edge (1-D)")
    row(name, sub(base, i, A(n - 1)), "%s has %d entries for %d edges" % (noun, n - 1, n))


base = (g_csr, g_csr, IP, WS)
reader(D + "CSRMMCount", "hhaa", base)
row(D + "CSRMMCount", sub(base, 0, LH()), NOT_UNIT % 0)
row(D + "CSRMMCount", sub(base, 1, H(g_csr)), NOT_UNIT % 1)
row(D + "CSRMMCount", sub(base, 0, g_csc), NEED_CSR)
row(D + "CSRMMCount", sub(base, 1, g_coo), NEED_CSR)
ids(D + "CSRMMCount", base, 2, "c_indptr")

base = (g_csr, W5, g_csr, W5, IP, IX, W7, WS)
reader(D + "CSRMMFill", "hahaaaaa", base)
row(D + "CSRMMFill", sub(base, 0, H(g_csr)), NOT_UNIT % 0)
row(D + "CSRMMFill", sub(base, 2, LH()), NOT_UNIT % 2)
row(D + "CSRMMFill", sub(base, 2, g_csc), NEED_CSR)
weights(D + "CSRMMFill", base, 1, "a_weights", 5)
weights(D + "CSRMMFill", base, 3, "b_weights", 5)
weights(D + "CSRMMFill", base, 6, "c_weights", 7)
ids(D + "CSRMMFill", base, 4, "c_indptr")
ids(D + "CSRMMFill", base, 5, "c_indices", num_rows=False)
for i in (1, 3, 6):
    row(D + "CSRMMFill", sub(base, i, base[i].dt("f64")), "csr_mm: the weights of a, b and c must share one element type")

COUNT = "csr_sum: the number of operands must be in [1, 4096]"
for name, base in ((D + "CSRSumCount", (1, g_csr, IP, WS)), (D + "CSRSumFill", (1, g_csr, W5, IP, IX, W7, WS))):
    row(name, (), "argument 0: expected an integer")
    row(name, sub(base, 0, "x"), "argument 0: expected an integer")
    row(name, sub(base, 0, 0), COUNT)
    row(name, sub(base, 0, 4097), COUNT)
    row(name, sub(base, 0, -1), COUNT)
    row(name, sub(base, 1, 1), "argument 1: expected an object handle")
    row(name, base[:1], "argument 1: expected an object handle")
    row(name, sub(base, 1, LH()), NOT_UNIT % 1)
    row(name, sub(base, 1, g_csc), NEED_CSR)
    for i in range(2, len(base)):
        row(name, sub(base, i, 1), "argument %d: expected an NDArray" % i)
        row(name, base[:i], "argument %d is missing" % i)
row(D + "CSRSumCount", (2, g_csr, H(g_csr), IP, WS), NOT_UNIT % 2)
row(D + "CSRSumCount", (2, g_csr, g_coo, IP, WS), NEED_CSR)
row(D + "CSRSumCount", (2, g_csr, g_csr, IP), "argument 4 is missing")
ids(D + "CSRSumCount", (1, g_csr, IP, WS), 2, "c_indptr")
base = (1, g_csr, W5, IP, IX, W7, WS)
weights(D + "CSRSumFill", base, 2, "weights", 5)
weights(D + "CSRSumFill", base, 5, "c_weights", 7)
ids(D + "CSRSumFill", base, 3, "c_indptr")
ids(D + "CSRSumFill", base, 4, "c_indices", num_rows=False)
row(D + "CSRSumFill", sub(base, 5, W7.dt("f64")), "csr_sum: the weights must share one element type")
row(D + "CSRSumFill", (2, g_csr, g_csr, W5, W5.dt("f64"), IP, IX, W7, WS), "csr_sum: the weights must share one element type")
row(D + "CSRSumFill", (2, g_csr, g_csr, W5, A(4), IP, IX, W7, WS), "weights has 4 entries for 5 edges")
row(D + "CSRSumFill", (2, g_csr, g_csr, W5, W5, IP, IX, W7), "argument 8 is missing")
row(D + "CSRSumFill", (2, g_csr, LH(), W5, W5, IP, IX, W7, WS), NOT_UNIT % 2)

base = (g_csr, W5, g_coo, W5)
reader(D + "CSRMask", "haha", base)
row(D + "CSRMask", sub(base, 0, LH()), NOT_UNIT % 0)
row(D + "CSRMask", sub(base, 2, H(g_coo)), NOT_UNIT % 2)
row(D + "CSRMask", sub(base, 0, g_coo), NEED_CSR)
row(D + "CSRMask", sub(base, 2, g_csr), "csr_mask needs the COO format of its second operand")
weights(D + "CSRMask", base, 1, "a_weights", 5)
weights(D + "CSRMask", base, 3, "out", 5)
row(D + "CSRMask", sub(base, 3, W5.dt("f64")), "csr_mask: a_weights and out must share one element type")

# ---- segment reduce family -----------------------------------------------------------------------------------------
FEAT, OFF, SOUT = A(6, 3), A(4, dt="i32"), A(3, 3)
base = ("max", FEAT, OFF, SOUT, ARG)
reader(S + "SegmentReduce", "saaaa", base)
for i in (1, 2, 3):
    row(S + "SegmentReduce", sub(base, i, None), "feat / offsets / out is required")
array_check(S + "SegmentReduce", base, {1: "array", 2: "array", 3: "array", 4: "array"}, ON_GPU)
row(S + "SegmentReduce", sub(base, 1, FEAT.dt("i32")), FLOAT)
row(S + "SegmentReduce", sub(base, 3, SOUT.dt("i32")), FLOAT)
row(S + "SegmentReduce", sub(base, 2, OFF.dt("f32")), INDEX)
row(S + "SegmentReduce", sub(base, 1, FEAT.dt("f64")), "feat and out dtypes differ")
row(S + "SegmentReduce", sub(base, 2, A(5, dt="i32")), "offsets must have out.shape[0] + 1 entries")
row(S + "SegmentReduce", sub(base, 2, A(4, 1, dt="i32")), "offsets must have out.shape[0] + 1 entries")
row(S + "SegmentReduce", sub(base, 4, None), "arg is required for max/min")
row(S + "SegmentReduce", sub(sub(base, 0, "min"), 4, None), "arg is required for max/min")
row(S + "SegmentReduce", sub(base, 4, ARG.dt("i64")), "arg dtype must equal the offsets dtype")
row(S + "SegmentReduce", sub(base, 4, ARG.dt("f32")), "arg dtype must equal the offsets dtype")

base = (FEAT, A(6, dt="i32"), SOUT)
reader(S + "ScatterAdd", "aaa", base)
for i in (0, 1, 2):
    row(S + "ScatterAdd", sub(base, i, None), "feat / idx / out is required")
row(S + "ScatterAdd", sub(base, 2, A(0, 3)), "out is empty but feat is not")
array_check(S + "ScatterAdd", base, {0: "array", 1: "array", 2: "array"}, ON_GPU)
row(S + "ScatterAdd", sub(base, 0, FEAT.dt("i32")), FLOAT)
row(S + "ScatterAdd", sub(base, 2, SOUT.dt("i32")), FLOAT)
row(S + "ScatterAdd", sub(base, 1, A(6, dt="f32")), INDEX)
row(S + "ScatterAdd", sub(base, 0, FEAT.dt("f64")), "feat and out dtypes differ")
row(S + "ScatterAdd", sub(base, 1, A(5, dt="i32")), "idx must have one entry per row of feat")
row(S + "ScatterAdd", sub(base, 1, A(6, 1, dt="i32")), "idx must have one entry per row of feat")

base = (SOUT, ARG, FEAT)
reader(S + "BwdSegmentCmp", "aaa", base)
for i in (0, 1, 2):
    row(S + "BwdSegmentCmp", sub(base, i, None), "feat / arg / out is required")
array_check(S + "BwdSegmentCmp", base, {0: "array", 1: "array", 2: "array"}, ON_GPU)
row(S + "BwdSegmentCmp", sub(base, 0, SOUT.dt("i32")), FLOAT)
row(S + "BwdSegmentCmp", sub(base, 2, FEAT.dt("i32")), FLOAT)
row(S + "BwdSegmentCmp", sub(base, 1, ARG.dt("f32")), INDEX)
row(S + "BwdSegmentCmp", sub(base, 2, FEAT.dt("f64")), "feat and out dtypes differ")

# ---- segment / gather mm -------------------------------------------------------------------------------------------
MA, MB, MC, SEG = A(6, 3), A(2, 3, 4), A(6, 4), A(2, dt="i64").host()


def mm_dims(name, base, nouns):
    for i, (noun, nd) in nouns.items():
        for bad in (None, A(*((6, 3, 4, 2)[:nd + 1])), A(*((6, 3, 4)[:nd - 1]))):
            row(name, sub(base, i, bad), "%s must be a %d-D array" % (noun, nd))
        row(name, sub(base, i, base[i].host()), noun + " is not on a GPU device")
        row(name, sub(base, i, base[i].strided()), noun + " must be contiguous")
        row(name, sub(base, i, base[i].dt("i32")), FLOAT)


base = (MA, MB, MC, SEG, 0, 0)
reader(S + "SEGMENTMM", "aaaaii", base)
mm_dims(S + "SEGMENTMM", base, {0: ("A", 2), 1: ("B", 3), 2: ("C", 2)})
row(S + "SEGMENTMM", sub(base, 3, None), "seglen_A must be a 1-D array")
row(S + "SEGMENTMM", sub(base, 3, A(2, 1, dt="i64").host()), "seglen_A must be a 1-D array")
row(S + "SEGMENTMM", sub(base, 4, 1), "segment_mm: A_trans is not supported (the reference never sets it)")
row(S + "SEGMENTMM", sub(base, 3, A(2, dt="f32").host()), INDEX)
for i in (0, 1, 2):
    row(S + "SEGMENTMM", sub(base, i, base[i].dt("f64")), "A, B and C dtypes differ")
row(S + "SEGMENTMM", sub(base, 3, A(3, dt="i64").host()), "segment_mm expects len(seglen_A) == B.shape[0]")
row(S + "SEGMENTMM", sub(base, 2, A(5, 4)), "segment_mm expects C.shape[0] == A.shape[0]")
SHAPES = "segment_mm expects A.shape[1] == B.shape[1] (B.shape[2] with B_trans) and C to match"
row(S + "SEGMENTMM", sub(base, 1, A(2, 5, 4)), SHAPES)
row(S + "SEGMENTMM", sub(base, 1, A(2, 3, 5)), SHAPES)
row(S + "SEGMENTMM", sub(base, 5, 1), SHAPES)

DC, DB = A(6, 4), A(2, 3, 4)
base = (MA, DC, DB, SEG)
reader(S + "SEGMENTMMBackwardB", "aaaa", base)
mm_dims(S + "SEGMENTMMBackwardB", base, {0: ("A", 2), 1: ("dC", 2), 2: ("dB", 3)})
row(S + "SEGMENTMMBackwardB", sub(base, 3, None), "seglen must be a 1-D array")
row(S + "SEGMENTMMBackwardB", sub(base, 3, A(2, 1, dt="i64").host()), "seglen must be a 1-D array")
row(S + "SEGMENTMMBackwardB", sub(base, 3, A(2, dt="f32").host()), INDEX)
for i in (0, 1, 2):
    row(S + "SEGMENTMMBackwardB", sub(base, i, base[i].dt("f64")), "A, dC and dB dtypes differ")
row(S + "SEGMENTMMBackwardB", sub(base, 1, A(5, 4)), "segment_mm backward expects A and dC to have the same rows")
DB_SHAPE = "segment_mm backward expects dB of shape (len(seglen), A.shape[1], dC.shape[1])"
row(S + "SEGMENTMMBackwardB", sub(base, 3, A(3, dt="i64").host()), DB_SHAPE)
row(S + "SEGMENTMMBackwardB", sub(base, 2, A(2, 2, 4)), DB_SHAPE)
row(S + "SEGMENTMMBackwardB", sub(base, 2, A(2, 3, 5)), DB_SHAPE)

IDX = A(6, dt="i32")
for name, base in ((S + "GATHERMM", (MA, MB, MC, IDX, IDX)), (S + "GATHERMMSCATTER", (MA, MB, MC, IDX, IDX, IDX))):
    reader(name, "a" * len(base), base)
    mm_dims(name, base, {0: ("A", 2), 1: ("B", 3), 2: ("C", 2)})
    for i in (0, 1, 2):
        row(name, sub(base, i, base[i].dt("f64")), "A, B and C dtypes differ")
    for i in range(3, len(base)):
        row(name, sub(base, i, IDX.host()), "index arrays must be on the GPU")
        row(name, sub(base, i, IDX.dt("f32")), INDEX)
    for i in range(4, len(base)):
        row(name, sub(base, i, IDX.dt("i64")), "index arrays must share one dtype")
        row(name, sub(base, i, A(5, dt="i32")), "index arrays must have the same length")
    row(name, base[:3] + (None,) * (len(base) - 3), "gather_mm needs at least one index array")
    row(name, sub(base, 0, A(6, 2)), "gather_mm expects A.shape[1] == B.shape[1]")
    row(name, sub(base, 2, A(6, 5)), "gather_mm expects C.shape[1] == B.shape[2]")

# ---- lists and the heterograph handle ------------------------------------------------------------------------------
row("_Value", (), "_Value takes one argument")
row("_Value", (1, 2), "_Value takes one argument")
HG = "expected (num_ntypes, [unit graph, src ntype, dst ntype] ...)"
row(D + "HeteroGraphCreate", (), "argument 0: expected an integer")
row(D + "HeteroGraphCreate", ("x", g_csc, 0, 1), "argument 0: expected an integer")
row(D + "HeteroGraphCreate", (2, g_csc), HG)
row(D + "HeteroGraphCreate", (2, g_csc, 0), HG)
row(D + "HeteroGraphCreate", (2, g_csc, 0, 1, g_csc), HG)
for bad in ((LH(), 0, 1), (H(g_csc), 0, 1), (1, 0, 1), (g_csc, "x", 1), (g_csc, 0, 1.5), (g_csc, 2, 1), (g_csc, 0, 2),
            (g_csc, -1, 1), (g_csc, 0, -1)):
    row(D + "HeteroGraphCreate", (2,) + bad, "bad relation 0")
    row(D + "HeteroGraphCreate", (2, g_csc, 0, 1) + bad, "bad relation 1")

hg, hg_coo = H(g_csc), H(g_coo)
ENTRY = "list entry %d is not an NDArray"
base = (hg, "mul", "sum", [U], [E], [None, V], [None, ARG], [None, ARG], [], [])
reader(S + "SpMMHetero", "hsslllllll", base)
row(S + "SpMMHetero", sub(base, 0, g_csc), NOT_HETERO)
row(S + "SpMMHetero", sub(base, 0, LH()), NOT_HETERO)
row(S + "SpMMHetero", sub(base, 2, "prod"), "Unsupported SpMM reducer: prod")
row(S + "SpMMHetero", sub(base, 3, [1]), ENTRY % 0)
row(S + "SpMMHetero", sub(base, 5, [None, "x"]), ENTRY % 1)
row(S + "SpMMHetero", sub(base, 5, [None, V.dt("i32")]), FLOAT)
for i, l in ((3, [U]), (4, [E]), (5, [None, V]), (6, [None, ARG]), (7, [None, ARG])):
    row(S + "SpMMHetero", sub(base, i, l[:-1] + [l[-1].host()]), ON_GRAPH % "array")
    row(S + "SpMMHetero", sub(base, i, l[:-1] + [l[-1].strided()]), "array must be contiguous")

base = (hg_coo, "dot", [LHS], [None, RHS], [OUT], 0, 2)
reader(S + "SDDMMHetero", "hslllii", base)
row(S + "SDDMMHetero", sub(base, 0, g_coo), NOT_HETERO)
row(S + "SDDMMHetero", sub(base, 0, LH()), NOT_HETERO)
for i, t in ((5, 3), (5, -1), (6, 3), (6, -1)):
    row(S + "SDDMMHetero", sub(base, i, t), "targets must be 0 (u), 1 (e) or 2 (v)")
row(S + "SDDMMHetero", sub(base, 4, [1]), ENTRY % 0)
row(S + "SDDMMHetero", sub(base, 3, [None, 1]), ENTRY % 1)
row(S + "SDDMMHetero", sub(base, 4, [OUT.dt("i32")]), FLOAT)
for i, l in ((2, [LHS]), (3, [None, RHS]), (4, [OUT])):
    row(S + "SDDMMHetero", sub(base, i, l[:-1] + [l[-1].host()]), ON_GRAPH % "array")
    row(S + "SDDMMHetero", sub(base, i, l[:-1] + [l[-1].strided()]), "array must be contiguous")
row(S + "SDDMMHetero", sub(base, 0, hg), "SDDMM only supports CSR and COO formats")

# the graph is reversed: relation 0 -> 1 reads feat / idx / idx_type of type 0 and writes out of type 1
base = (hg, "copy_lhs", [SOUT], [ARG], [ARG], [None, U])
reader(S + "UpdateGradMinMaxHetero", "hsllll", base)
row(S + "UpdateGradMinMaxHetero", sub(base, 0, g_csc), NOT_HETERO)
row(S + "UpdateGradMinMaxHetero", sub(base, 0, LH()), NOT_HETERO)
row(S + "UpdateGradMinMaxHetero", sub(base, 2, [1]), ENTRY % 0)
row(S + "UpdateGradMinMaxHetero", sub(base, 2, [SOUT.dt("i32")]), FLOAT)
row(S + "UpdateGradMinMaxHetero", sub(base, 3, [ARG.dt("f32")]), INDEX)
row(S + "UpdateGradMinMaxHetero", sub(base, 4, [ARG.dt("u8")]), INDEX)
row(S + "UpdateGradMinMaxHetero", sub(base, 4, [ARG.dt("i64")]), "idx and idx_type must have the same integer type")
for i, l in ((2, [SOUT]), (3, [ARG]), (4, [ARG]), (5, [None, U])):
    row(S + "UpdateGradMinMaxHetero", sub(base, i, l[:-1] + [l[-1].host()]), ON_GRAPH % "array")
    row(S + "UpdateGradMinMaxHetero", sub(base, i, l[:-1] + [l[-1].strided()]), "array must be contiguous")

# ---- a handle of another kind where a unit graph is expected: one entry of each family -------------------------------
for name, args in ((D + "UnitGraphSetCSC", (A(4, dt="i32"), A(5, dt="i32"), None)),
                   (D + "UnitGraphSetWorkspace", (WS,)),
                   (D + "UnitGraphStaticOperand", (1,)),
                   (D + "UnitGraphFree", ()),
                   (S + "SpMM", ("mul", "sum", U, E, V)),
                   (S + "SpMMWorkspaceBytes", ("mul", "sum", U, E, V)),
                   (S + "SpMMStacked", ("mul", U, E, TAB, TAB, V, REL)),
                   (S + "SpMMStackedCmpWorkspaceBytes", ("mul", "max", U, E, TAB, TAB, V, REL, TYPES, ARG, ARG, ARG, ARG)),
                   (S + "SDDMM", ("dot", LHS, RHS, OUT, 0, 2)),
                   (S + "Edge_softmax_forward", ("copy_rhs", None, E, E)),
                   (S + "Edge_softmaxWorkspaceBytes", (1, 32)),
                   (D + "GATAttentionForward", (FT, EL, ER, 0.2, GOUT, MZ, WS)),
                   (D + "GATAttentionTrainBackward", (FT, EL, ER, MZ, GOUT, 0.2, 0.5, 7, FT, EL, ER, WS)),
                   (D + "GATAttentionWorkspaceBytes", (2, 3))):
    WRONG_HANDLE.append((name, (LH(),) + args, NOT_UNIT % 0))
    WRONG_HANDLE.append((name, (H(g_all),) + args, NOT_UNIT % 0))

# names whose body cannot refuse anything
EXEMPT = {"_List": "takes any number of values of any kind"}


def _ids(table):
    return ["%03d-%s" % (i, r[0].replace(S, "").replace(D, "")) for i, r in enumerate(table)]


@pytest.mark.parametrize("name,args,msg", TABLE, ids=_ids(TABLE))
def test_refusal(name, args, msg):
    assert _refused(name, args) == msg


def test_every_registered_name_has_a_case():
    names = set(_ffi.list_global_func_names())
    covered = {r[0] for r in TABLE}
    assert covered <= names and set(EXEMPT) <= names and not covered & set(EXEMPT)
    assert names - covered - set(EXEMPT) == set()


@pytest.mark.parametrize("name,args,msg", WRONG_HANDLE, ids=_ids(WRONG_HANDLE))
def test_wrong_kind_of_handle(name, args, msg):
    """A `_List` handle or a heterograph handle passed as the unit graph.  Until the typed argument reader checked
    the tag of every handle these calls were undefined (the handle was cast unchecked); they are the only cases of
    this file that are not refused by the code before that reader."""
    assert _refused(name, args) == msg
