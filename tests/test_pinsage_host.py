"""PinSAGE neighbour selection (include/dgl_amd.h "PinSAGE neighbour selection", csrc/pinsage.hip) through the HOST entry
point — runs without a GPU.

dgla_pinsage_select_host is the library's plain C++ statement of the rule; the checker below is an independent numpy
restatement written from the header's text (per segment np.unique with counts, then a lexsort).  All comparisons are
equality: the operator is integer-only.  tests/test_zzzzzzz_gpu_pinsage.py holds the kernel to both.  Also here: the
argument errors of the three _capi entry points that need no device, and the construction of RandomWalkNeighborSampler /
PinSAGESampler (errors, metapath, restart tensor).  Reference: python/dgl/sampling/pinsage.py,
src/graph/sampling/randomwalks/randomwalk_cpu.cc:41-102."""
import numpy as np
import pytest
import torch

NP = {torch.int32: np.int32, torch.int64: np.int64}
BIG = {torch.int32: [2 ** 31 - 1], torch.int64: [2 ** 31 - 1, 2 ** 40 + 3, 2 ** 62 + 1]}
KINDS = ("random", "all_none", "one_id", "distinct", "ties", "big", "sparse")


# ---- the numpy model of the rule -----------------------------------------------------------------
def model_select(src, dst, S, k):
    """(src, dst, counts) of the rule, and the padded form (src [n, k'], counts [n, k'], num [n])."""
    n = len(src) // S
    kp = min(k, S)
    p_src = np.full((n, kp), -1, dtype=src.dtype)
    p_cnt = np.zeros((n, kp), dtype=src.dtype)
    num = np.zeros(n, dtype=src.dtype)
    out = [[], [], []]
    for j in range(n):
        seg = src[j * S:(j + 1) * S]
        ids, cnt = np.unique(seg[seg != -1], return_counts=True)
        order = np.lexsort((ids, cnt))[::-1][:k]            # count, then id, both descending
        num[j] = len(order)
        p_src[j, :len(order)] = ids[order]
        p_cnt[j, :len(order)] = cnt[order]
        out[0].append(ids[order])
        out[1].append(np.full(len(order), dst[j * S], dtype=src.dtype))
        out[2].append(cnt[order].astype(src.dtype))
    return tuple(np.concatenate(o).astype(src.dtype) for o in out), (p_src, p_cnt, num)


# ---- inputs --------------------------------------------------------------------------------------
def segment(kind, S, idtype, rng):
    """One segment of S ids of the given kind (int64 values that fit `idtype`)."""
    big = BIG[idtype]
    if kind == "all_none":                      # no output
        return np.full(S, -1, dtype=np.int64)
    if kind == "one_id":                        # one output with count S
        return np.full(S, 12345, dtype=np.int64)
    if kind == "distinct":                      # pure id-descending order; id 0 present
        return rng.permutation(S).astype(np.int64) * 3
    if kind == "ties":                          # a few counts shared by many ids; id 0 present
        pool = np.arange(max(1, S // 3), dtype=np.int64) * 7
        return rng.permutation(np.resize(pool, S))
    if kind == "big":                           # the top of the id range next to 0, with ties between the large ids
        pool = np.array([0, 1] + big + [b - 1 for b in big], dtype=np.int64)
        return pool[rng.integers(0, len(pool), S)]
    if kind == "sparse":                        # mostly -1
        seg = rng.integers(0, 5, S).astype(np.int64)
        seg[rng.random(S) < 0.8] = -1
        return seg
    seg = np.minimum(np.floor(rng.random(S) ** 3 * 4 * S), 2 ** 20).astype(np.int64)   # skewed visit counts
    seg[rng.random(S) < 0.1] = -1
    return seg


def make_input(num_dst, S, idtype, seed, kinds=KINDS):
    """src / dst of num_dst segments whose kinds cycle through `kinds`; dst repeats one id per segment."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([segment(kinds[j % len(kinds)], S, idtype, rng) for j in range(num_dst)]).astype(NP[idtype])
    dst = np.repeat(rng.integers(0, 1000, num_dst), S).astype(NP[idtype])
    return src, dst


def host_select(src, dst, S, k):
    from dgl_amd import _capi

    got = _capi.select_pinsage_neighbors_host(torch.from_numpy(src), torch.from_numpy(dst), S, k)
    assert all(g.dtype == torch.from_numpy(src).dtype and g.dim() == 1 for g in got)
    return tuple(g.numpy() for g in got)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("src", "dst", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


# ---- host entry point == numpy model ---------------------------------------------------------------
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 600])
def test_host_equals_model(idtype, S):
    for num_dst in (1, 257):
        # one segment: every kind on its own; many segments: the kinds interleaved
        inputs = [make_input(1, S, idtype, 100 + i, (kind,)) for i, kind in enumerate(KINDS)] if num_dst == 1 \
            else [make_input(num_dst, S, idtype, 7 * S)]
        for src, dst in inputs:
            for k in (1, 3, S, S + 5):
                want, _ = model_select(src, dst, S, k)
                assert_same(host_select(src, dst, S, k), want, (S, num_dst, k))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_known_answers(idtype):
    dt = NP[idtype]
    big = BIG[idtype][-1]
    seg0 = [5, 9, 5, -1, 0, 9]                  # 5 x2, 9 x2, 0 x1: the tie puts 9 before 5
    seg1 = [-1] * 6                             # nothing
    seg2 = [0, -1, big, -1, big - 1, -1]        # three ids once each: id descending
    src = np.array(seg0 + seg1 + seg2, dtype=dt)
    dst = np.repeat(np.array([70, 80, 90], dtype=dt), 6)
    s, d, c = host_select(src, dst, 6, 2)
    assert s.tolist() == [9, 5, big, big - 1] and d.tolist() == [70, 70, 90, 90] and c.tolist() == [2, 2, 1, 1]
    s, d, c = host_select(src, dst, 6, 100)
    assert s.tolist() == [9, 5, 0, big, big - 1, 0] and d.tolist() == [70] * 3 + [90] * 3 and c.tolist() == [2, 2, 1, 1, 1, 1]
    s, d, c = host_select(src, dst, 18, 4)      # the same ids as ONE segment: dst is read at the segment's start
    assert s.tolist() == [9, 5, 0, big] and d.tolist() == [70] * 4 and c.tolist() == [2, 2, 2, 1]


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_every_segment_empty(idtype):
    src, dst = make_input(40, 7, idtype, 1, ("all_none",))
    got = host_select(src, dst, 7, 3)
    assert all(g.shape == (0,) and g.dtype == NP[idtype] for g in got)
    got = host_select(src[:0], dst[:0], 7, 3)   # no segment at all
    assert all(g.shape == (0,) and g.dtype == NP[idtype] for g in got)


# ---- argument errors -------------------------------------------------------------------------------
def test_argument_errors():
    from dgl_amd import _capi
    from dgl_amd._lib import DGLAMDError

    src = torch.arange(12, dtype=torch.int64)
    dst = torch.zeros(12, dtype=torch.int64)
    entries = (_capi.select_pinsage_neighbors, _capi.select_pinsage_neighbors_padded, _capi.select_pinsage_neighbors_host)
    for fn in entries:
        with pytest.raises(DGLAMDError, match="not a multiple"):
            fn(src, dst, 5, 2)
        with pytest.raises(DGLAMDError, match="both be int32 or both int64"):
            fn(src, dst.int(), 4, 2)
        with pytest.raises(DGLAMDError, match="both be int32 or both int64"):
            fn(src.short(), dst.short(), 4, 2)
        with pytest.raises(DGLAMDError, match="both be int32 or both int64"):
            fn(src.float(), dst.float(), 4, 2)
        with pytest.raises(DGLAMDError, match="k must be at least 1"):
            fn(src, dst, 4, 0)
        with pytest.raises(DGLAMDError, match="num_samples_per_node must be at least 1"):
            fn(src, dst, 0, 2)
    for idtype in (torch.int32, torch.int64):
        limit = _capi.pinsage_max_samples(idtype)
        assert limit >= 4096 and _capi.pinsage_size_classes()[-1] == limit
        big = torch.zeros(limit + 1, dtype=idtype)
        for fn in entries[:2]:                  # the device forms refuse S over the limit, and CPU tensors
            with pytest.raises(DGLAMDError, match="above the largest segment"):
                fn(big, big, limit + 1, 2)
            with pytest.raises(DGLAMDError, match="no CPU fallback"):
                fn(src.to(idtype), dst.to(idtype), 4, 2)
        s, d, c = entries[2](big, big, limit + 1, 2)        # the host form has no limit
        assert s.tolist() == [0] and c.tolist() == [limit + 1]
    assert _capi.pinsage_size_classes() == sorted(set(_capi.pinsage_size_classes()))


def test_c_entry_points_refuse_before_any_launch():
    """The C ABI checks S, k and the id width first: with null pointers and no device these calls return -1 and a
    message, so nothing was launched."""
    from dgl_amd import _lib

    L = _lib.LIB
    limit = L.dgla_pinsage_max_samples(64)
    assert L.dgla_pinsage_max_samples(32) == limit and L.dgla_pinsage_max_samples(16) == 0
    total = _lib.ctypes.c_int64(-1)
    for S, k, bits, msg in ((limit + 1, 2, 64, "above the largest segment"), (0, 2, 32, "num_samples_per_node must be"),
                            (4, 0, 64, "k must be"), (4, 2, 16, "idtype must be")):
        assert L.dgla_pinsage_select_padded(bits, None, None, 3, S, k, None, None, None, None, None) == -1
        assert msg in L.dgla_last_error().decode()
        assert L.dgla_pinsage_select_count(bits, None, None, 3, S, k, _lib.ctypes.byref(total), None, 0, None) == -1
        assert msg in L.dgla_last_error().decode()
        assert L.dgla_pinsage_select_fill(bits, 3, S, k, None, None, None, None, 0, None) == -1
        assert msg in L.dgla_last_error().decode()
        assert L.dgla_pinsage_select_workspace_bytes(bits, 3, S, k) == 0
    assert L.dgla_pinsage_select_workspace_bytes(64, 1000, 600, 10) >= 1000 * 10 * 8 * 2
    assert L.dgla_pinsage_select_count(64, None, None, 3, 4, 2, _lib.ctypes.byref(total), None, 0, None) == -1


# ---- sampler construction ----------------------------------------------------------------------------
def _bipartite():
    import dgl_amd

    u = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 0, 1, 2])
    return dgl_amd.heterograph({("item", "bought-by", "user"): u, ("user", "bought", "item"): (u[1], u[0]),
                                ("user", "follows", "user"): (torch.tensor([0, 1]), torch.tensor([1, 2]))},
                               {"item": 3, "user": 3})


def test_sampler_construction_errors():
    import dgl_amd
    from dgl_amd import sampling
    from dgl_amd._lib import DGLAMDError

    assert dgl_amd.RandomWalkNeighborSampler is sampling.RandomWalkNeighborSampler
    assert dgl_amd.PinSAGESampler is sampling.PinSAGESampler and issubclass(sampling.PinSAGESampler,
                                                                           sampling.RandomWalkNeighborSampler)
    g = _bipartite()
    with pytest.raises(ValueError, match="Metapath must be specified"):
        sampling.RandomWalkNeighborSampler(g, 3, 0.5, 10, 4)
    with pytest.raises(ValueError, match="start and end at the same node type"):
        sampling.RandomWalkNeighborSampler(g, 3, 0.5, 10, 4, metapath=["bought-by"])
    with pytest.raises(ValueError, match="start and end at the same node type"):
        sampling.RandomWalkNeighborSampler(g, 3, 0.5, 10, 4, metapath=["bought", "bought-by", "follows", "bought"])
    with pytest.raises(DGLAMDError, match="no edge type goes from"):
        sampling.PinSAGESampler(g, "item", "nobody", 3, 0.5, 10, 4)


def test_sampler_metapath_and_restart_tensor():
    import dgl_amd
    from dgl_amd import sampling

    g = _bipartite()
    s = sampling.RandomWalkNeighborSampler(g, 4, 0.25, 10, 3, metapath=["bought-by", "follows", "bought"],
                                           weight_column="visits")
    assert s.ntype == "item" and s.metapath_hops == 3 and s.full_metapath == ["bought-by", "follows", "bought"] * 4
    assert s.weight_column == "visits" and s.num_neighbors == 3 and s.num_random_walks == 10 and s.num_traversals == 4
    want = [0.0] * 12
    want[3] = want[6] = want[9] = 0.25          # every multiple of the metapath length except 0
    assert s.restart_prob.dtype == torch.float32 and s.restart_prob.tolist() == want
    p = sampling.PinSAGESampler(g, "user", "item", 2, 0.5, 5, 2)
    assert p.ntype == "user" and p.metapath == [("user", "bought", "item"), ("item", "bought-by", "user")]
    assert p.restart_prob.tolist() == [0.0, 0.0, 0.5, 0.0] and p.weight_column == "weights"
    h = dgl_amd.graph((torch.tensor([0, 1]), torch.tensor([1, 0])), num_nodes=2)
    one = sampling.RandomWalkNeighborSampler(h, 3, 0.5, 7, 2)      # homogeneous: one step over the only edge type
    assert one.metapath == [("_N", "_E", "_N")] and one.ntype == "_N" and one.restart_prob.tolist() == [0.0, 0.5, 0.5]
