"""Point-cloud graphs on the device (csrc/knn.hip): device == host bit for bit (ids and distances) on every case of
tests/knn_cases.py, each run twice with identical bytes, the lattice cases and the generic ones alike because the fma
order is shared; then the Python surface as the reference's _test_knn_common, test_knn_sharedmem_large and test_fps
check it (tests/python/pytorch/geometry/test_geometry.py:15-210)."""
import warnings

import numpy as np
import pytest
import torch

from tests import knn_cases as kc

pytestmark = pytest.mark.gpu

FLOATS = [np.float32, np.float64]
ALL_CASES = kc.exact_cases() + kc.generic_cases() + [kc.special_case()]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_device_equals_host_bit_for_bit(dev, case, dtype):
    for idtype in (torch.int32, torch.int64):
        h_ids, h_dist = kc.run_knn(case, dtype, idtype)
        for _ in range(2):
            ids, dist = kc.run_knn(case, dtype, idtype, device=dev)
            assert same_bytes(ids, h_ids), (case["name"], idtype)
            assert same_bytes(dist, h_dist), (case["name"], idtype)


def test_ids_alone_and_a_side_stream(dev):
    from dgl_amd import _capi

    case = kc.exact_cases()[3]
    x = torch.from_numpy(case["x"].astype(np.float32)).to(dev)
    y = torch.from_numpy(case["y"].astype(np.float32)).to(dev)
    xo, yo = kc.offsets(case["x_segs"]), kc.offsets(case["y_segs"])
    want = kc.run_knn(case, np.float32, torch.int64)[0]
    assert np.array_equal(_capi.knn(x, xo, case["k"], y, yo).cpu().numpy(), want)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = _capi.knn(x, xo, case["k"], y, yo)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", sorted(kc.fps_clouds()))
@pytest.mark.parametrize("dtype", FLOATS, ids=["f32", "f64"])
def test_fps_device_equals_host(dev, name, dtype):
    pos, starts = kc.fps_clouds()[name]
    B, N, _ = pos.shape
    for s in starts:
        for npoints in (1, N // 2 + 1, N):
            want = kc.run_fps(pos, npoints, [s] * B, dtype)
            for _ in range(2):
                assert np.array_equal(kc.run_fps(pos, npoints, [s] * B, dtype, device=dev), want), (name, s, npoints)


def test_fps_workspace_path_equals_host(dev):
    """A cloud past the LDS limit keeps mind in the workspace: the same picks."""
    rng = np.random.default_rng(8)
    pos = rng.standard_normal((2, kc.FPS_LDS_ROWS + 3, 3))
    want = kc.run_fps(pos, 6, [5, kc.FPS_LDS_ROWS + 2], np.float32)
    assert np.array_equal(kc.run_fps(pos, 6, [5, kc.FPS_LDS_ROWS + 2], np.float32, device=dev), want)


# ---- the Python surface ----------------------------------------------------------------------------------
def in_sets(g):
    src, dst = (t.cpu().numpy() for t in g.edges())
    return [set(src[dst == v]) for v in range(g.num_nodes())], np.bincount(dst, minlength=g.num_nodes())


@pytest.mark.parametrize("algorithm", ["bruteforce-blas", "bruteforce", "bruteforce-sharemem"])
@pytest.mark.parametrize("dist", ["euclidean", "cosine"])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_knn_graph_as_the_reference_checks_it(dev, algorithm, dist, exclude_self):
    import dgl_amd
    from dgl_amd import DGLError
    from dgl_amd.transforms import DGLWarning

    torch.manual_seed(3)
    x = torch.randn(8, 3, device=dev)
    if dist == "euclidean":
        d = torch.cdist(x, x).cpu()
    else:
        x = x + torch.randn(1).item()
        tmp = x / (1e-5 + torch.sqrt(torch.sum(x * x, dim=1, keepdim=True)))
        d = (1 - tmp @ tmp.T).cpu()

    def check_knn(g, start, end, k, check_indices=True):
        assert g.device == x.device
        sets, deg = in_sets(g)
        for v in range(start, end):
            assert len(sets[v]) == k and deg[v] == k
            if check_indices:
                ans = set((torch.topk(d[start:end, start:end][v - start], k + (1 if exclude_self else 0),
                                      largest=False)[1] + start).tolist())
                if exclude_self:
                    ans.remove(v)
                assert sets[v] == ans

    def check_batch(g, k, info):
        assert torch.equal(g.batch_num_nodes().cpu(), torch.tensor(info))
        assert torch.equal(g.batch_num_edges().cpu(), k * torch.tensor(info))

    kw = dict(algorithm=algorithm, dist=dist, exclude_self=exclude_self)
    with warnings.catch_warnings():
        warnings.simplefilter("error", DGLWarning)          # none of these may warn
        g = dgl_amd.knn_graph(x, 3, **kw)
        check_knn(g, 0, 8, 3)
        check_batch(g, 3, [8])
        g = dgl_amd.knn_graph(x.view(2, 4, 3), 3, **kw)
        check_knn(g, 0, 4, 3)
        check_knn(g, 4, 8, 3)
        check_batch(g, 3, [4, 4])
        k = 3 - (1 if exclude_self else 0)
        g = dgl_amd.segmented_knn_graph(x, k, [3, 5], **kw)
        check_knn(g, 0, 3, k)
        check_knn(g, 3, 8, k)
        check_batch(g, k, [3, 5])

    # k above the number of points is clamped with a warning
    with pytest.warns(DGLWarning):
        g = dgl_amd.knn_graph(x, 10, **kw)
    k = 8 - (1 if exclude_self else 0)
    check_knn(g, 0, 8, k)
    check_batch(g, k, [8])
    with pytest.warns(DGLWarning):
        g = dgl_amd.knn_graph(x.view(2, 4, 3), 10, **kw)
    k = 4 - (1 if exclude_self else 0)
    check_knn(g, 0, 4, k)
    check_knn(g, 4, 8, k)
    check_batch(g, k, [4, 4])
    with pytest.warns(DGLWarning):
        g = dgl_amd.segmented_knn_graph(x, 5, [3, 5], **kw)
    k = 3 - (1 if exclude_self else 0)
    check_knn(g, 0, 3, k)
    check_knn(g, 3, 8, k)
    check_batch(g, k, [3, 5])

    # the error cases
    k = 0 - (1 if exclude_self else 0)
    with pytest.raises(DGLError):
        dgl_amd.knn_graph(x, k, **kw)
    with pytest.raises(DGLError):
        dgl_amd.segmented_knn_graph(x, k, [3, 5], **kw)
    empty = torch.tensor([], device=dev)
    with pytest.raises(DGLError):
        dgl_amd.knn_graph(empty, 3, **kw)
    with pytest.raises(DGLError):
        dgl_amd.segmented_knn_graph(empty, 3, [3, 5], **kw)

    # 20 coincident points: more than k of them, so exclude_self needs the repair
    z = torch.zeros((20, 3), device=dev)
    g = dgl_amd.knn_graph(z, 3, **kw)
    check_knn(g, 0, 20, 3, False)
    check_batch(g, 3, [20])
    g = dgl_amd.segmented_knn_graph(z, 3, [4, 7, 5, 4], **kw)
    for lo, hi in ((0, 4), (4, 11), (11, 16), (16, 20)):
        check_knn(g, lo, hi, 3, False)
    check_batch(g, 3, [4, 7, 5, 4])
    if exclude_self:
        src, dst = g.edges()
        assert not bool((src == dst).any())


@pytest.mark.parametrize("num_points", [8, 64, 256, 1024])
def test_knn_against_topk_of_the_gram_form(dev, num_points):
    import dgl_amd

    torch.manual_seed(num_points)
    x = torch.randn(num_points, 5, device=dev)
    y = torch.randn(num_points, 5, device=dev)
    k = 4
    d = torch.sum(x * x, dim=1) + torch.sum(y * y, dim=1).unsqueeze(-1) - 2 * torch.mm(y, x.T)
    want = torch.sort(torch.topk(d, k, dim=-1, largest=False)[1], dim=-1)[0]
    out = dgl_amd.knn(k, x, [num_points], y, [num_points], algorithm="bruteforce-sharemem")
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, k * num_points)
    assert torch.equal(out[0], torch.arange(num_points, device=dev).repeat_interleave(k))
    assert torch.equal(torch.sort(out[1].reshape(-1, k), -1)[0], want)


def test_knn_limit_is_refused_by_name(dev):
    import dgl_amd
    from dgl_amd import DGLError

    x = torch.randn(100, 3, device=dev)
    with pytest.raises(DGLError, match="kKnnMaxK"):
        dgl_amd.knn(kc.MAX_K + 1, x, [100])
    with pytest.raises(DGLError, match="float16 / bfloat16"):
        dgl_amd.knn(3, x.half(), [100])
    with pytest.raises(DGLError, match="do not match"):
        dgl_amd.knn(3, x, [60, 30])


def test_farthest_point_sampler(dev):
    from dgl_amd.geometry import farthest_point_sampler

    rng = np.random.default_rng(0)
    x = torch.tensor(rng.uniform(size=(5, 200, 3)), device=dev)          # fp64, as the reference's test
    res = farthest_point_sampler(x, 10)
    assert res.dtype == torch.int64 and tuple(res.shape) == (5, 10) and res.device == x.device
    assert int(res.min()) >= 0 and int(res.max()) < 200 and int(res.sum()) > 0
    assert all(len(set(r.tolist())) == 10 for r in res)
    res = farthest_point_sampler(x, 10, start_idx=0)
    assert bool((res[:, 0] == 0).all())
    assert np.array_equal(res.cpu().numpy(), kc.run_fps(x.cpu().numpy(), 10, [0] * 5, np.float64))
    res = farthest_point_sampler(x.float(), 10, start_idx=199)
    assert bool((res[:, 0] == 199).all())
    a, b = farthest_point_sampler(x, 7, seed=11), farthest_point_sampler(x, 7, seed=11)
    assert torch.equal(a, b)
    starts = torch.stack([farthest_point_sampler(x, 1, seed=s)[:, 0] for s in range(8)])
    assert len(torch.unique(starts)) > 1                                  # the seed moves the start
