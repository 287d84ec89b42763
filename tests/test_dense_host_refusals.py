"""What the dense Graphormer units refuse on the host, and what their workspaces take, pinned to recorded tables — runs
without a GPU.

The three dense units (biased_attention, spatial_encoder3d, graphormer_bias) take no ``dgla_csr``, so
tests/test_host_refusals.py does not reach them.  Here every entry point of theirs is called through ctypes with small
host buffers standing in for the pointers; nothing dereferences them, because every call is one of two kinds:

  * a call the entry refuses BEFORE any runtime call: it returns -1 and ``dgla_last_error()`` is ``"<who>: <message>"``,
    no HIP error text;
  * a call that returns 0 before any launch: ``B == 0`` (attention), ``B * N == 0`` (spatial encoder),
    ``num_pairs == 0`` (bias forward), nothing wanted (bias backward).

No accepted non-empty call is made: it would launch.  ``REFUSALS`` holds one defect per row, forward and backward where
both have it; ``DOUBLY_WRONG`` holds calls that are wrong in two ways, whose message shows the ORDER of the checks.
``WORKSPACE_BYTES`` holds rows ``(query, arguments, bytes)`` of the three ``*_workspace_bytes`` queries: sizes at 0, 1,
across a 32-pair tile and a 256-byte boundary, one large shape, and arguments the query answers with 0 because the
entry would refuse the shape:
  biased_attention (B, N, H)        spatial_encoder3d (B, N, K, H)
  graphormer_bias (num_pairs, path_len, max_len, num_edges, num_heads, spatial_rows)

All three tables were recorded from the library as it stood BEFORE the dense units moved to the shared tile header
(csrc/mfma_tile.h) and the dense part of the host scaffold (csrc/host_util.h), so a unit that starts to refuse more,
less, in another order or in other words, or whose workspace changes size, shows up here as a diff of one row."""
import numpy as np
import pytest

from dgl_amd._lib import LIB

F32, F64, F16, BF16 = 0, 1, 2, 3          # dtype codes of include/dgl_amd.h
BUF = np.zeros(1 << 12, np.uint8)         # stands in for every pointer, a too small workspace included
PTR = BUF.ctypes.data


def last_error():
    return LIB.dgla_last_error().decode()


def _pointers(null):
    return lambda name: None if name in null else PTR


# ---- the calls: every keyword is the undamaged value, a row of the tables overrides what it damages ------------------
def attention(direction, dtype=F32, B=1, N=32, H=4, D=32, drop=0.0, null=(), ws=None, ws_bytes=0):
    p = _pointers(null)
    head = (dtype, p("q"), p("k"), p("v"), p("bias"), p("mask"))
    if direction == "forward":
        return LIB.dgla_biased_attention_forward(*head, B, N, H, D, 1.0, drop, 7, p("out"), p("lse"), None)
    return LIB.dgla_biased_attention_backward(*head, p("out"), p("lse"), p("dout"), B, N, H, D, 1.0, drop, 7, p("dq"), p("dk"),
                                              p("dv"), p("dbias"), ws, ws_bytes, None)


def attention_mask(direction, drop=0.0, B=1, H=1, N=4, null=()):
    return LIB.dgla_biased_attention_dropout_mask_host(7, drop, B, H, N, _pointers(null)("keep"))


SE_OPERANDS = ("coord", "gamma_src", "gamma_tgt", "beta_src", "beta_tgt", "means", "stds", "w1", "b1", "w2", "b2")
SE_GRADIENTS = ("dw1", "db1", "dw2", "db2", "dmeans", "dstds", "dgamma_src", "dgamma_tgt", "dbeta_src", "dbeta_tgt")


def spatial(direction, dtype=F32, B=1, N=4, K=8, H=4, null=(), ws=None, ws_bytes=0):
    p = _pointers(null)
    head = (dtype,) + tuple(p(name) for name in SE_OPERANDS)
    if direction == "forward":
        return LIB.dgla_spatial_encoder3d_forward(*head, B, N, K, H, p("out"), None)
    return LIB.dgla_spatial_encoder3d_backward(*head, p("dout"), B, N, K, H, *(p(name) for name in SE_GRADIENTS), ws, ws_bytes,
                                               None)


def bias(direction, idtype_bits=64, dtype=F32, num_pairs=16, path_len=2, num_edges=8, max_len=4, H=4, spatial_rows=6,
         null=(), ws=None, ws_bytes=0):
    p = _pointers(null)
    if direction == "forward":
        return LIB.dgla_graphormer_bias_forward(idtype_bits, dtype, p("dist"), p("paths"), num_pairs, path_len, p("table"),
                                                num_edges, max_len, H, p("spatial"), spatial_rows, p("out"), None)
    return LIB.dgla_graphormer_bias_backward(idtype_bits, dtype, p("dist"), p("paths"), num_pairs, path_len, num_edges, max_len, H,
                                             spatial_rows, p("grad_out"), p("grad_table"), p("grad_spatial"), 0, ws, ws_bytes,
                                             None)


# unit -> (who, call, its workspace query with the undamaged sizes)
UNITS = {
    "attention": ("biased_attention", attention, lambda: LIB.dgla_biased_attention_workspace_bytes(1, 32, 4)),
    "attention_mask": ("biased_attention", attention_mask, None),
    "spatial": ("spatial_encoder_3d", spatial, lambda: LIB.dgla_spatial_encoder3d_workspace_bytes(1, 4, 8, 4)),
    "bias": ("graphormer_bias", bias, lambda: LIB.dgla_graphormer_bias_workspace_bytes(16, 2, 4, 8, 4, 6)),
}
BOTH = ("forward", "backward")
FWD, BWD = ("forward",), ("backward",)

_FLOATS = "operands must be float32, float16 or bfloat16"
_QKV = "q, k, v must be (B, N, H, D) with N >= 1 and H >= 1"
_DROP = "the dropout probability must lie in [0, 1)"
_MASK = "the mask is (B, H, N, N) with H >= 1 and N >= 1"
_BWD_NULL = "an operand or a gradient of q, k, v is null"
_COORD = "coord must be (B, N, 3) with B >= 0 and N >= 0"
_TWO_ROWS = "a spatial table has at least two rows (max_dist + 2)"

# (unit, directions, damage, the message behind "<who>: " or 0)
REFUSALS = [
    ("attention", BOTH, dict(dtype=F64), _FLOATS),
    ("attention", BOTH, dict(N=0), _QKV),
    ("attention", BOTH, dict(H=0), _QKV),
    ("attention", BOTH, dict(D=0), "head width 0: the kernels take 1 to 128"),
    ("attention", BOTH, dict(D=129), "head width 129: the kernels take 1 to 128"),
    ("attention", BOTH, dict(drop=1.0), _DROP),
    ("attention", BOTH, dict(drop=-0.1), _DROP),
    ("attention", BOTH, dict(N=1 << 30), "sizes overflow"),
    ("attention", BOTH, dict(B=1 << 31), "more workgroups than one launch takes"),
    ("attention", BOTH, dict(B=(1 << 29) + 1, N=33, H=5, D=128), "more workgroups than one launch takes"),
    ("attention", FWD, dict(null=("q",)), "q, k, v, out or lse is null"),
    ("attention", FWD, dict(null=("out",)), "q, k, v, out or lse is null"),
    ("attention", BWD, dict(null=("q",)), _BWD_NULL),
    ("attention", BWD, dict(null=("out",)), _BWD_NULL),
    ("attention", BWD, dict(null=("dq",)), _BWD_NULL),
    ("attention", BOTH, dict(B=0), 0),
    ("attention", BOTH, dict(B=0, null=("q", "out", "dq")), 0),
    ("attention_mask", FWD, dict(drop=1.0), _DROP),
    ("attention_mask", FWD, dict(H=0), _MASK),
    ("attention_mask", FWD, dict(null=("keep",)), _MASK),
    ("attention_mask", FWD, dict(B=0, null=("keep",)), 0),
    ("spatial", BOTH, dict(dtype=F64), "the weights must be float32, float16 or bfloat16"),
    ("spatial", BOTH, dict(B=-1), _COORD),
    ("spatial", BOTH, dict(N=-1), _COORD),
    ("spatial", BOTH, dict(K=0), "num_kernels 0: the kernels take 1 to 128"),
    ("spatial", BOTH, dict(K=129), "num_kernels 129: the kernels take 1 to 128"),
    ("spatial", BOTH, dict(H=0), "num_heads 0: the kernels take 1 to 64"),
    ("spatial", BOTH, dict(H=65), "num_heads 65: the kernels take 1 to 64"),
    ("spatial", BOTH, dict(N=1 << 31), "sizes overflow"),
    ("spatial", BOTH, dict(B=1 << 16, N=1 << 15), "sizes overflow"),              # B N = 2^31
    ("spatial", BOTH, dict(B=1 << 60, N=1), "sizes overflow"),
    ("spatial", FWD, dict(null=("coord",)), "an operand or out is null"),
    ("spatial", FWD, dict(null=("b2",)), "an operand or out is null"),
    ("spatial", FWD, dict(null=("out",)), "an operand or out is null"),
    ("spatial", BWD, dict(null=("coord",)), "an operand or dout is null"),
    ("spatial", BWD, dict(null=("b2",)), "an operand or dout is null"),
    ("spatial", BWD, dict(null=("dout",)), "an operand or dout is null"),
    ("spatial", BWD, dict(null=("dw1",)), "a gradient is null"),
    ("spatial", BWD, dict(null=("dbeta_tgt",)), "a gradient is null"),
    ("spatial", BOTH, dict(B=0), 0),
    ("spatial", BOTH, dict(N=0, null=("coord", "out", "dout", "dw1")), 0),
    ("bias", BOTH, dict(idtype_bits=16), "idtype must be int32 or int64"),
    ("bias", BOTH, dict(dtype=F64), _FLOATS),
    ("bias", BOTH, dict(num_pairs=-1), "negative size"),
    ("bias", BOTH, dict(path_len=-1), "negative size"),
    ("bias", BOTH, dict(H=0), "0 heads: the kernels take 1 to 256"),
    ("bias", BOTH, dict(H=257), "257 heads: the kernels take 1 to 256"),
    ("bias", BOTH, dict(max_len=0), "max_len 0: the kernels take 1 to 32"),
    ("bias", BOTH, dict(max_len=33), "max_len 33: the kernels take 1 to 32"),
    ("bias", BOTH, dict(spatial_rows=1), _TWO_ROWS),
    ("bias", BOTH, dict(num_pairs=1 << 56), "sizes overflow"),
    ("bias", FWD, dict(null=("dist",)), "dist or out is null"),
    ("bias", FWD, dict(null=("out",)), "dist or out is null"),
    ("bias", FWD, dict(null=("paths",)), "paths is null"),
    ("bias", FWD, dict(null=("table",)), "the projected table is null"),
    ("bias", FWD, dict(num_pairs=0), 0),
    ("bias", FWD, dict(num_pairs=0, null=("dist", "out", "paths", "table")), 0),
    ("bias", BWD, dict(spatial_rows=0), _TWO_ROWS),
    ("bias", BWD, dict(spatial_rows=1 << 30), "the spatial table is larger than one launch takes"),
    ("bias", BWD, dict(null=("dist",)), "dist or grad_out is null"),
    ("bias", BWD, dict(null=("grad_out",)), "dist or grad_out is null"),
    ("bias", BWD, dict(null=("paths",)), "paths is null"),
    ("bias", BWD, dict(null=("grad_table", "grad_spatial")), 0),
    ("bias", BWD, dict(num_edges=0, null=("grad_spatial",)), 0),                  # a table without rows is not wanted
    ("bias", BWD, dict(spatial_rows=1, null=("grad_table", "grad_spatial")), 0),  # a table nobody asks for has no rows
]

# Calls that are wrong in two ways: the order of the checks decides the message.  `SHORT` hands over a workspace of no
# bytes, which every backward refuses last.
SHORT = dict(ws=PTR, ws_bytes=0)
DOUBLY_WRONG = [
    ("attention", BOTH, dict(dtype=F64, N=0), _FLOATS),
    ("attention", BOTH, dict(N=0, D=0), _QKV),
    ("attention", BOTH, dict(D=129, drop=1.0), "head width 129: the kernels take 1 to 128"),
    ("attention", BOTH, dict(drop=1.0, N=1 << 30), _DROP),
    ("attention", BOTH, dict(N=1 << 30, B=1 << 31), "sizes overflow"),
    ("attention", BOTH, dict(B=1 << 31, null=("q",)), "more workgroups than one launch takes"),
    ("attention", BOTH, dict(B=0, D=0), "head width 0: the kernels take 1 to 128"),
    ("attention", BWD, dict(null=("dq",), **SHORT), _BWD_NULL),
    ("attention_mask", FWD, dict(drop=1.0, H=0), _DROP),
    ("spatial", BOTH, dict(dtype=F64, B=-1), "the weights must be float32, float16 or bfloat16"),
    ("spatial", BOTH, dict(B=-1, K=0), _COORD),
    ("spatial", BOTH, dict(K=0, H=0), "num_kernels 0: the kernels take 1 to 128"),
    ("spatial", BOTH, dict(H=65, N=1 << 31), "num_heads 65: the kernels take 1 to 64"),
    ("spatial", BOTH, dict(N=1 << 31, null=("coord",)), "sizes overflow"),
    ("spatial", BOTH, dict(B=0, K=129), "num_kernels 129: the kernels take 1 to 128"),
    ("spatial", BWD, dict(null=("dout", "dw1")), "an operand or dout is null"),
    ("spatial", BWD, dict(null=("dw1",), **SHORT), "a gradient is null"),
    ("bias", BOTH, dict(idtype_bits=16, dtype=F64), "idtype must be int32 or int64"),
    ("bias", BOTH, dict(dtype=F64, num_pairs=-1), _FLOATS),
    ("bias", BOTH, dict(num_pairs=-1, H=0), "negative size"),
    ("bias", BOTH, dict(H=257, max_len=0), "257 heads: the kernels take 1 to 256"),
    ("bias", BOTH, dict(max_len=33, spatial_rows=1), "max_len 33: the kernels take 1 to 32"),
    ("bias", BOTH, dict(spatial_rows=1, num_pairs=1 << 56), _TWO_ROWS),
    ("bias", FWD, dict(num_pairs=0, H=0), "0 heads: the kernels take 1 to 256"),
    ("bias", FWD, dict(null=("dist", "paths")), "dist or out is null"),
    ("bias", FWD, dict(null=("paths", "table")), "paths is null"),
    ("bias", BWD, dict(max_len=33, null=("grad_table", "grad_spatial")), "max_len 33: the kernels take 1 to 32"),
    ("bias", BWD, dict(spatial_rows=0, null=("dist",)), _TWO_ROWS),
    ("bias", BWD, dict(null=("dist", "paths")), "dist or grad_out is null"),
    ("bias", BWD, dict(null=("paths",), **SHORT), "paths is null"),
]


def _ids(table):
    return ["%s-%s" % (unit, ",".join("%s=%s" % (k, "+".join(v) if isinstance(v, tuple) else v) for k, v in sorted(damage.items())))
            for unit, _, damage, _ in table]


def _check(unit, directions, damage, expected):
    who, call, _ = UNITS[unit]
    for direction in directions:
        rc = call(direction, **damage)
        if expected == 0:
            assert rc == 0, (unit, direction, last_error())
        else:
            assert rc == -1, (unit, direction)
            assert last_error() == "%s: %s" % (who, expected), (unit, direction)   # (no HIP error text: no runtime call was made)


@pytest.mark.parametrize("unit,directions,damage,expected", REFUSALS, ids=_ids(REFUSALS))
def test_refusals_and_empty_calls_match_the_recorded_table(unit, directions, damage, expected):
    _check(unit, directions, damage, expected)


@pytest.mark.parametrize("unit,directions,damage,expected", DOUBLY_WRONG, ids=_ids(DOUBLY_WRONG))
def test_a_doubly_wrong_call_gets_the_first_check_s_message(unit, directions, damage, expected):
    _check(unit, directions, damage, expected)


@pytest.mark.parametrize("unit", ["attention", "spatial", "bias"])
def test_a_short_workspace_is_refused_in_the_one_wording(unit):
    who, call, query = UNITS[unit]
    need = query()
    assert need >= 256 and need % 256 == 0     # (with need == 0 the call below would be accepted, and launch)
    assert call("backward", ws=PTR, ws_bytes=need - 256) == -1
    assert last_error() == "%s: workspace of %d bytes required, got %d" % (who, need, need - 256)


def test_the_tables_cover_every_unit_in_both_directions():
    for unit, both in (("attention", True), ("attention_mask", False), ("spatial", True), ("bias", True)):
        seen = {d for u, ds, _, _ in REFUSALS + DOUBLY_WRONG if u == unit for d in ds}
        assert seen == (set(BOTH) if both else {"forward"}), unit
        assert any(e == 0 for u, _, _, e in REFUSALS if u == unit), unit


# ---- workspace sizes ------------------------------------------------------------------------------------------------
WORKSPACE_QUERIES = {
    "biased_attention": LIB.dgla_biased_attention_workspace_bytes,
    "spatial_encoder3d": LIB.dgla_spatial_encoder3d_workspace_bytes,
    "graphormer_bias": LIB.dgla_graphormer_bias_workspace_bytes,
}
WORKSPACE_BYTES = [
    ("biased_attention", (0, 1, 1), 0),
    ("biased_attention", (1, 1, 1), 256),
    ("biased_attention", (1, 63, 1), 256),
    ("biased_attention", (1, 64, 1), 256),
    ("biased_attention", (1, 65, 1), 512),
    ("biased_attention", (31, 1, 1), 256),
    ("biased_attention", (32, 1, 2), 256),
    ("biased_attention", (33, 1, 2), 512),
    ("biased_attention", (64, 512, 32), 4194304),
    ("biased_attention", (-1, 32, 4), 0),
    ("biased_attention", (1, 0, 4), 0),
    ("biased_attention", (1, 32, 0), 0),
    ("biased_attention", (1099511627776, 1048576, 8), 0),
    ("spatial_encoder3d", (0, 4, 8, 4), 0),
    ("spatial_encoder3d", (1, 0, 8, 4), 0),
    ("spatial_encoder3d", (1, 1, 1, 1), 512),
    ("spatial_encoder3d", (1, 4, 8, 4), 768),
    ("spatial_encoder3d", (31, 1, 128, 64), 100352),
    ("spatial_encoder3d", (32, 1, 128, 64), 100352),
    ("spatial_encoder3d", (33, 1, 128, 64), 200448),
    ("spatial_encoder3d", (2, 4, 33, 8), 6144),
    ("spatial_encoder3d", (16, 256, 128, 32), 25591808),
    ("spatial_encoder3d", (64, 512, 128, 64), 92733440),
    ("spatial_encoder3d", (-1, 4, 8, 4), 0),
    ("spatial_encoder3d", (1, 4, 0, 4), 0),
    ("spatial_encoder3d", (1, 4, 129, 4), 0),
    ("spatial_encoder3d", (1, 4, 8, 65), 0),
    ("spatial_encoder3d", (1, 2147483648, 8, 4), 0),
    ("graphormer_bias", (0, 0, 1, 0, 1, 0), 256),
    ("graphormer_bias", (0, 2, 4, 8, 4, 6), 256),
    ("graphormer_bias", (1, 1, 1, 1, 1, 2), 7168),
    ("graphormer_bias", (16, 2, 4, 8, 4, 6), 7168),
    ("graphormer_bias", (31, 5, 5, 64, 8, 22), 14848),
    ("graphormer_bias", (32, 5, 5, 64, 8, 22), 14848),
    ("graphormer_bias", (33, 5, 5, 64, 8, 22), 14848),
    ("graphormer_bias", (33, 5, 5, 64, 8, 0), 14080),
    ("graphormer_bias", (33, 0, 5, 64, 8, 22), 1024),
    ("graphormer_bias", (33, 8, 5, 0, 8, 22), 1024),
    ("graphormer_bias", (16777216, 32, 5, 1048576, 32, 512), 4194476032),
    ("graphormer_bias", (-1, 2, 4, 8, 4, 6), 0),
    ("graphormer_bias", (16, 2, 4, 8, 0, 6), 0),
    ("graphormer_bias", (16, 2, 4, 8, 257, 6), 0),
    ("graphormer_bias", (16, 2, 33, 8, 4, 6), 0),
    ("graphormer_bias", (16, 2, 4, 8, 4, 1), 0),
    ("graphormer_bias", (16, 2, 4, 8, 256, 16777216), 0),
]


@pytest.mark.parametrize("query,args,nbytes", WORKSPACE_BYTES, ids=["%s-%s" % (q, "x".join(map(str, a))) for q, a, _ in WORKSPACE_BYTES])
def test_workspace_bytes_match_the_recorded_table(query, args, nbytes):
    assert WORKSPACE_QUERIES[query](*args) == nbytes
    assert nbytes % 256 == 0


def test_the_workspace_table_covers_every_query_and_its_refusals():
    for query in WORKSPACE_QUERIES:
        sizes = [b for q, _, b in WORKSPACE_BYTES if q == query]
        assert len(sizes) >= 12 and 0 in sizes and max(sizes) >= 1 << 22, query
