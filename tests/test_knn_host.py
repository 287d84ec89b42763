"""The rule of the point-cloud entry points (csrc/knn_step.h) run by the CPU: dgla_knn_host and dgla_fps_host against
the numpy model of tests/knn_cases.py, the refusals by their messages and the workspace sizes.  No GPU.

Exact part: lattice coordinates (multiples of 1/4 in [-4, 4], D <= 257) make every difference, square and sum exact in
fp32 (a sum stays below 2^15 with four fraction bits), so host == model for ids AND distance bits, massive ties
included.  Generic part: randn inputs; every returned distance within (D + 2) * eps relative of the wider model (the
bound of a chain of D fused steps: one rounding per subtraction, entering squared, and one per step), and no excluded
point closer than the k-th returned one by more than twice that margin."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import knn_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = [np.float32, np.float64]
IDS = [torch.int32, torch.int64]
EPS = {np.float32: 2.0 ** -23, np.float64: 2.0 ** -52}
WIDE = {np.float32: np.float64, np.float64: np.longdouble}


def test_constants_match_the_library():
    from dgl_amd import _capi

    assert _capi.knn_tile_sizes() == (kc.QUERY_TILE, kc.DATA_TILE)
    assert _capi.knn_max_k() == kc.MAX_K >= 64


# ---- k-NN: exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.exact_cases() + [kc.special_case()], ids=lambda c: c["name"])
@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_host_equals_model_exactly(case, dtype):
    want_ids, want_dist = kc.model_knn(case, dtype)
    for idtype in IDS:
        ids, dist = kc.run_knn(case, dtype, idtype)
        assert ids.dtype == (np.int32 if idtype == torch.int32 else np.int64) and dist.dtype == dtype
        assert np.array_equal(ids.astype(np.int64), want_ids), case["name"]
        assert np.array_equal(dist, want_dist.astype(dtype)), case["name"]       # bits: no NaN is ever written
        assert not np.isnan(dist).any()


def test_coincident_points_come_in_ascending_id():
    case = next(c for c in kc.exact_cases() if c["name"] == "coincident")
    ids, dist = kc.run_knn(case, np.float32, torch.int64)
    assert np.array_equal(ids[1].reshape(100, 20), np.tile(np.arange(20), (100, 1)))
    assert (dist == 0).all()


def test_duplicates_across_a_tile_boundary_rank_by_id():
    T = kc.DATA_TILE
    case = next(c for c in kc.exact_cases() if c["name"] == "dup_tile_boundary_xy")
    ids, dist = kc.run_knn(case, np.float32, torch.int64)
    assert list(ids[1][:6]) == [T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T] and (dist[:6] == 0).all()
    assert list(ids[1][6:12]) == [T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T] and (dist[6:12] == 0.0625).all()


def test_short_and_empty_segments_leave_minus_one():
    case = next(c for c in kc.exact_cases() if c["name"] == "xy_k20_d5")
    ids, dist = kc.run_knn(case, np.float64, torch.int32)
    k = case["k"]
    yo = kc.offsets(case["y_segs"])
    q = yo[2]                                   # a query of the segment with 7 data rows
    assert (ids[1][q * k:q * k + 7] >= 0).all() and (ids[1][q * k + 7:(q + 1) * k] == -1).all()
    assert np.isinf(dist[q * k + 7:(q + 1) * k]).all()
    q = yo[4]                                   # a query of the segment without data rows
    assert (ids[1][q * k:(q + 1) * k] == -1).all() and (ids[0][q * k:(q + 1) * k] == q).all()


def test_nan_distances_order_as_infinity():
    case = kc.special_case()
    ids, dist = kc.run_knn(case, np.float32, torch.int64)
    k = case["k"]
    row = lambda q: (ids[1][q * k:(q + 1) * k], dist[q * k:(q + 1) * k])
    nbr, d = row(1)                             # a NaN query: every distance is +inf, the ids ascend
    assert np.array_equal(nbr, np.arange(k)) and np.isinf(d).all()
    nbr, d = row(0)                             # a finite query: the four special rows come last, by id
    bad = [3, 9, 17, 33]
    assert np.isfinite(d[:k - 2]).all() and not set(nbr[:36]) & set(bad)
    assert list(nbr[36:]) == bad[:2] and np.isinf(d[36:]).all()


# ---- k-NN: generic -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.generic_cases(), ids=lambda c: c["name"])
@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_generic_inputs_stay_within_the_chain_bound(case, dtype):
    ids, dist = kc.run_knn(case, dtype, torch.int64)
    k, D = case["k"], case["D"]
    rel = (D + 2) * EPS[dtype]
    segs = kc.model_distances(case, dtype, WIDE[dtype])
    for q0, x0, M in segs:
        for i in range(M.shape[0]):
            q = q0 + i
            nbr = ids[1][q * k:(q + 1) * k] - x0
            got = dist[q * k:(q + 1) * k].astype(WIDE[dtype])
            exact = M[i][nbr]
            assert (np.abs(got - exact) <= rel * exact).all(), (case["name"], q)
            assert (np.diff(got) >= 0).all() and len(set(nbr)) == k
            left_out = np.delete(M[i], nbr)
            assert (left_out >= exact[-1] * (1 - 2 * rel)).all(), (case["name"], q)


# ---- farthest points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.fps_clouds()))
@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_fps_host_equals_model(name, dtype):
    pos, starts = kc.fps_clouds()[name]
    B, N, _ = pos.shape
    for s in starts:
        for npoints in (1, 2, N // 2 + 1, N):
            start = [s] * B
            got = kc.run_fps(pos, npoints, start, dtype)
            assert np.array_equal(got, kc.model_fps(pos, npoints, start)), (name, s, npoints)
            assert (got[:, 0] == s).all()
            if npoints == N:                    # every row exactly once
                assert (np.sort(got, axis=1) == np.arange(N)).all()


def test_fps_coincident_points_and_square_corners():
    pos, _ = kc.fps_clouds()["coincident"]
    got = kc.run_fps(pos, 9, [4, 0], np.float32)
    assert list(got[0]) == [4, 0, 1, 2, 3, 5, 6, 7, 8] and list(got[1]) == list(range(9))
    pos, _ = kc.fps_clouds()["square"]
    # from corner 0: the opposite corner 3 (distance 2), then corners 1 and 2 tie at 1 (the smaller first), the centre last
    assert list(kc.run_fps(pos, 5, [0], np.float64)[0]) == [0, 3, 1, 2, 4]
    # from the centre every corner ties at 1/2: corner 0 first; the other corners stay at 1/2 (their distance to the
    # centre is below the one to corner 0), so they follow in ascending order
    assert list(kc.run_fps(pos, 5, [4], np.float32)[0]) == [4, 0, 1, 2, 3]


def test_fps_different_starts_per_cloud():
    pos, _ = kc.fps_clouds()["lattice_b3_n50"]
    start = [49, 0, 23]
    assert np.array_equal(kc.run_fps(pos, 12, start, np.float32), kc.model_fps(pos, 12, start))


# ---- the C ABI -----------------------------------------------------------------------------------------
NEW = ["dgla_knn_max_k", "dgla_knn_tile_sizes", "dgla_knn_workspace_bytes", "dgla_knn", "dgla_knn_host",
       "dgla_fps_workspace_bytes", "dgla_fps", "dgla_fps_host"]


def test_header_declares_and_library_exports_the_entry_points():
    from dgl_amd._lib import LIB

    header = open(os.path.join(ROOT, "include", "dgl_amd.h")).read()
    assert "Point-cloud graphs" in header and "#define DGLA_ABI_VERSION 2" in header
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(LIB, name), name


def test_workspace_sizes():
    from dgl_amd._lib import LIB

    # the tile table: three int64 per segment boundary, on a 256-byte boundary
    for segs, want in {-1: 0, 0: 0, 1: 256, 9: 256, 10: 512, 31: 768, 32: 1024}.items():
        assert LIB.dgla_knn_workspace_bytes(segs) == want, segs
    # farthest points: nothing while mind fits LDS, then one value per row
    R = kc.FPS_LDS_ROWS
    for (dt, B, N), want in {(0, 4, 0): 0, (0, 4, 1): 0, (0, 4, R): 0, (1, 4, R): 0, (0, 4, R + 1): 65792,
                             (1, 1, R + 1): 33024, (0, 0, R + 1): 0, (2, 4, R + 1): 0}.items():
        assert LIB.dgla_fps_workspace_bytes(dt, B, N) == want, (dt, B, N)


def test_bad_arguments_fail_with_a_message():
    from dgl_amd._lib import LIB

    x = torch.zeros(8, 3)
    ids = torch.zeros(2, 16, dtype=torch.int64)
    off = (ctypes.c_int64 * 2)(0, 8)
    X, I = x.data_ptr(), ids.data_ptr()

    def refused(rc, *words):
        assert rc == -1
        msg = LIB.dgla_last_error().decode()
        assert all(w in msg for w in words), msg

    host = lambda **kw: LIB.dgla_knn_host(*[kw.get(n, d) for n, d in (
        ("x", X), ("num_x", 8), ("y", None), ("num_y", 8), ("dtype", 0), ("dim", 3), ("xo", off), ("yo", off), ("segs", 1),
        ("k", 2), ("bits", 64), ("ids", I), ("dist", None))])
    assert host() == 0
    refused(host(k=kc.MAX_K + 1), "knn_host", "k = 65", "kKnnMaxK = 64")
    refused(host(k=0), "k must be at least 1")
    refused(host(dtype=2), "float16 / bfloat16")
    refused(host(dtype=3), "float16 / bfloat16")
    refused(host(dtype=7), "unknown dtype")
    refused(host(bits=16), "idtype must be int32 or int64")
    refused(host(dim=0), "dim must be at least 1")
    refused(host(x=None), "x is null")
    refused(host(num_y=5), "y is null")
    refused(host(xo=None), "x_offsets is null")
    refused(host(yo=None), "y_offsets is null")
    refused(host(ids=None), "out_ids is null")
    refused(host(xo=(ctypes.c_int64 * 2)(0, 7)), "x_offsets do not match", "end at 7", "8 rows")
    refused(host(yo=(ctypes.c_int64 * 2)(1, 8)), "y_offsets do not match", "start at 0")
    refused(host(segs=2, xo=(ctypes.c_int64 * 3)(0, 9, 8)), "x_offsets do not match", "descend")
    refused(host(num_x=2 ** 31, num_y=2 ** 31), "below 2^31 - 64")
    # the device entry point refuses the same things before any launch (no GPU is touched), and a missing workspace
    dev = lambda **kw: LIB.dgla_knn(*[kw.get(n, d) for n, d in (
        ("x", X), ("num_x", 8), ("y", None), ("num_y", 8), ("dtype", 0), ("dim", 3), ("xo", off), ("yo", off), ("segs", 1),
        ("k", 2), ("bits", 64), ("ids", I), ("dist", None), ("ws", None), ("ws_bytes", 0), ("stream", None))])
    refused(dev(k=kc.MAX_K + 1), "knn:", "kKnnMaxK")
    refused(dev(dtype=2), "float16 / bfloat16")
    refused(dev(), "workspace of 256 bytes required")

    pos, start, out = torch.zeros(2, 5, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64)
    fps = lambda **kw: LIB.dgla_fps_host(*[kw.get(n, d) for n, d in (
        ("pos", pos.data_ptr()), ("dtype", 0), ("B", 2), ("N", 5), ("dim", 3), ("n", 3), ("start", start.data_ptr()),
        ("out", out.data_ptr()))])
    assert fps() == 0
    refused(fps(dtype=3), "fps_host", "float16 / bfloat16")
    refused(fps(n=6), "npoints must be in [1, num_rows = 5]")
    refused(fps(n=0), "npoints must be in")
    refused(fps(dim=0), "dim must be at least 1")
    refused(fps(pos=None), "are null")
    refused(fps(start=None), "are null")
    refused(fps(out=None), "are null")
    rc = LIB.dgla_fps(pos.data_ptr(), 0, 2, kc.FPS_LDS_ROWS + 1, 3, 3, start.data_ptr(), out.data_ptr(), None, 0, None)
    refused(rc, "fps:", "workspace of", "bytes required")


def test_python_surface_refuses_by_name():
    import dgl_amd
    from dgl_amd import DGLError

    x = torch.zeros(8, 3)
    for algorithm in ("kd-tree", "nn-descent"):
        for call in (lambda: dgl_amd.knn(2, x, [8], algorithm=algorithm), lambda: dgl_amd.knn_graph(x, 2, algorithm=algorithm),
                     lambda: dgl_amd.segmented_knn_graph(x, 2, [3, 5], algorithm=algorithm)):
            with pytest.raises(DGLError, match=algorithm):
                call()
    with pytest.raises(DGLError, match="Invalid k value"):
        dgl_amd.knn_graph(x, 0)
    with pytest.raises(DGLError, match="Invalid k value"):
        dgl_amd.segmented_knn_graph(x, -1, [3, 5], exclude_self=True)
    with pytest.raises(DGLError, match="Find empty point set"):
        dgl_amd.knn_graph(torch.tensor([]), 3)
    with pytest.raises(DGLError, match="Find empty point set"):
        dgl_amd.segmented_knn_graph(torch.tensor([]), 3, [3, 5])
    with pytest.raises(DGLError, match="no CPU fallback"):          # a CPU tensor reaches no kernel
        dgl_amd.knn_graph(x, 2)
    with pytest.raises(DGLError, match="Invalid start_idx"):
        dgl_amd.geometry.farthest_point_sampler(torch.zeros(2, 5, 3), 2, start_idx=5)
    with pytest.raises(DGLError, match="no CPU fallback"):
        dgl_amd.geometry.farthest_point_sampler(torch.zeros(2, 5, 3), 2, start_idx=0)
