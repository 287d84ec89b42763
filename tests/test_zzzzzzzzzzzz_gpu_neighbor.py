"""Neighbour sampling and block building on the device (csrc/sampling.hip: sample_pick_kernel, weighted_pick_kernel,
the block builder over csrc/sort.hip.h) against the Python model of the rule (tests/neighbor_cases.py; its law, its
known answers and the power of these cases are shown on the CPU by tests/test_neighbor_model.py).

EQUALITY only, nothing statistical: the picks, counts and edge ids of the device are the model's, byte for byte, over
the degree ladders around every dispatch boundary of the kernels (fanout 16|17, 32|33, 128; rows of 63 .. 129 and 1000
edges for the wavefront-per-row weighted kernels; 16 384 keys and 32 768 elements for the block builder's sort and
scan), int32 and int64 ids, with and without an edge-id map, call seeds 0, 42 and 2^64 - 1.  The one comparison that
involves rounding — the inverse-CDF picks on weights whose sums are inexact — is held to the exact prefix sums within
1e-12 of the row's total."""
import math

import numpy as np
import pytest
import torch

from dgl_amd import DGLAMDError, _capi
from tests import neighbor_cases as nc

pytestmark = pytest.mark.gpu

IDTYPES = [torch.int32, torch.int64]
_CSR = {}


def csr_on(dev, name, G, idtype, use_eids):
    key = (name, idtype, use_eids)
    if key not in _CSR:
        _CSR[key] = nc.device_csr(G, idtype, use_eids, dev)
    return _CSR[key]


def same(got, want, idtype):
    """Byte for byte: the id type of the call and the model's values."""
    return got.dtype == nc.NP_I[idtype] and np.array_equal(got, want.astype(nc.NP_I[idtype]))


def rows_of(indptr, a):
    return [a[indptr[i]:indptr[i + 1]].tolist() for i in range(len(indptr) - 1)]


# ---- 1. uniform ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("f", nc.FANOUTS)
def test_uniform_equals_the_model(dev, idtype, f):
    G = nc.uniform_graph(f)
    seeds, perm = nc.uniform_seeds(f)
    for use_eids in (False, True):
        csr = csr_on(dev, "uniform%d" % f, G, idtype, use_eids)
        for fanout, replace in nc.uniform_modes(f):
            for S in nc.CALL_SEEDS:
                indptr, gpos = nc.expected_uniform(f, fanout, replace, S)
                src, eids = nc.gather(G, gpos, use_eids)
                got = nc.run_uniform(csr, seeds, fanout, replace, S, idtype, dev)
                where = (f, fanout, replace, S, use_eids)
                assert same(got[0], indptr, idtype), where
                assert same(got[1], src, idtype) and same(got[2], eids, idtype), where
                again = nc.run_uniform(csr, seeds, fanout, replace, S, idtype, dev)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), where
            # keyed by the node id: the seeds permuted give the rows permuted (and the node listed twice the same row)
            moved = nc.run_uniform(csr, seeds[perm], fanout, replace, 42, idtype, dev)
            first = nc.run_uniform(csr, seeds, fanout, replace, 42, idtype, dev)
            for k in (1, 2):
                rows = rows_of(first[0], first[k])
                assert rows_of(moved[0], moved[k]) == [rows[p] for p in perm], (f, fanout, replace)


@pytest.mark.parametrize("idtype", IDTYPES)
def test_no_seeds_and_refused_fanouts(dev, idtype):
    G = nc.uniform_graph(2)
    csr = csr_on(dev, "uniform2", G, idtype, True)
    none = np.zeros(0, dtype=np.int64)
    for fanout, replace in ((2, False), (2, True), (-1, False)):
        indptr, src, eids = nc.run_uniform(csr, none, fanout, replace, 42, idtype, dev)
        assert indptr.tolist() == [0] and len(src) == 0 and len(eids) == 0
    Gw, w = nc.weighted_graph("dyadic")
    wcsr = csr_on(dev, "dyadic", Gw, idtype, False)
    for replace in (False, True):
        indptr, src, eids = nc.run_weighted(wcsr, w, none, 7, replace, 42, idtype, dev)
        assert indptr.tolist() == [0] and len(src) == 0 and len(eids) == 0
    seeds = np.arange(3)
    for fanout in (0, -2):
        with pytest.raises(DGLAMDError, match="fanout must be positive, or -1 for all neighbours"):
            nc.run_uniform(csr, seeds, fanout, False, 42, idtype, dev)
    with pytest.raises(DGLAMDError, match="fanout larger than 128 is not supported"):
        nc.run_uniform(csr, seeds, 129, False, 42, idtype, dev)


# ---- 2 - 4. weighted ---------------------------------------------------------------------------------------
def weighted_runs(dev, kind, dtype, idtype, replace):
    """Every (use_eids, fanout, call seed) of a table: (where, rows' weights, model, device)."""
    G, w_pos = nc.weighted_graph(kind)
    seeds = nc.weighted_seeds(G)
    for use_eids in (False, True):
        csr = csr_on(dev, kind, G, idtype, use_eids)
        prob = nc.prob_by_eid(G, w_pos, use_eids, dtype)
        for fanout in nc.W_FANOUTS:
            for S in nc.W_SEEDS:
                got = nc.run_weighted(csr, prob, seeds, fanout, replace, S, idtype, dev)
                yield (kind, fanout, replace, S, use_eids), G, seeds, use_eids, S, nc.expected_weighted(kind, dtype, fanout, replace, S), got


@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weighted_with_replacement_equals_the_model_on_exact_sums(dev, idtype, dtype):
    """Dyadic rows: every partial sum is exact whatever order the wavefront adds in, so total, targets and picks are
    the model's."""
    for where, G, seeds, use_eids, S, (indptr, gpos), got in weighted_runs(dev, "dyadic", dtype, idtype, True):
        src, eids = nc.gather(G, gpos, use_eids)
        assert same(got[0], indptr, idtype), where
        assert same(got[1], src, idtype) and same(got[2], eids, idtype), where


@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weighted_with_replacement_inverts_the_exact_prefix(dev, idtype, dtype):
    """Generic rows: the device adds the weights in another order than the model, so a target within rounding of a prefix
    may fall to the neighbouring positive edge.  Counts are exact; every pick c is positive and
    P[previous positive] - tol < target <= P[c] + tol with P the exact prefix and tol = 1e-12 * total; at most 1 pick in
    10 000 differs from the model's own."""
    picks = differ = 0
    G, w_pos = nc.weighted_graph("generic")
    w_pos = w_pos.astype(dtype)
    pos_of_eid = np.argsort(G["eids"])
    prefix = {}
    for where, G, seeds, use_eids, S, (indptr, gpos), got in weighted_runs(dev, "generic", dtype, idtype, True):
        assert same(got[0], indptr, idtype), where
        got_pos = pos_of_eid[got[2]] if use_eids else got[2].astype(np.int64)
        assert np.array_equal(got[1], G["indices"][got_pos]), where
        for i, r in enumerate(seeds):
            start, end = int(G["indptr"][r]), int(G["indptr"][r + 1])
            w = w_pos[start:end]
            if r not in prefix:
                pos = nc.positive_positions(w)
                running = 0.0                     # the model's total: the running fp64 sum
                for j in pos:
                    running += float(w[j])
                prefix[r] = ({j: q for q, j in enumerate(pos)}, nc.exact_prefix(w, pos), running)
            rank, P, model_total = prefix[r]
            tol = 1e-12 * P[-1] if P else 0.0
            assert not P or P[-1] == math.fsum(float(w[j]) for j in rank)
            for t in range(int(indptr[i]), int(indptr[i + 1])):
                c = int(got_pos[t]) - start
                assert c in rank, (where, r, t)            # a positive position of the seed's own row
                q = rank[c]
                target = nc.slot_target(S, int(r), t - int(indptr[i]), model_total)
                assert (P[q - 1] if q else 0.0) - tol < target <= P[q] + tol, (where, r, t)
                picks += 1
                differ += int(got_pos[t] != gpos[t])
    print("generic rows, %s: %d of %d picks differ from the model's" % (np.dtype(dtype).name, differ, picks))
    assert picks > 10000 and differ * 10000 <= picks


@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["dyadic", "generic"])
def test_weighted_without_replacement_equals_the_model(dev, idtype, dtype, kind):
    """The slots are the positive positions in ascending (key, position).  First, on the CPU: the model's keys (math.log,
    fp64) of the first picks + 1 of every row are more than 1e-9 apart relatively, so a device logarithm a few ulp off
    cannot reorder them — a wrong scan, tie rule or edge-id lookup does."""
    G, w_pos = nc.weighted_graph(kind)
    w_pos = w_pos.astype(dtype)
    for S in nc.W_SEEDS:
        gap = min(nc.min_key_gap(S, r, nc.row_weights(G, w_pos, r, False), nc.MAX_FANOUT) for r in range(G["num_rows"]))
        assert gap > 1e-9, (S, gap)
    for where, G, seeds, use_eids, S, (indptr, gpos), got in weighted_runs(dev, kind, dtype, idtype, False):
        src, eids = nc.gather(G, gpos, use_eids)
        assert same(got[0], indptr, idtype), where
        assert same(got[1], src, idtype) and same(got[2], eids, idtype), where


# ---- 5. the special row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_weights(dev, idtype, dtype):
    G, w = nc.special_graph(dtype)
    positive = len(nc.positive_positions(w))
    assert positive == 90 - len(nc.SPECIAL_NEVER)
    seeds = np.zeros(1, dtype=np.int64)
    for use_eids in (False, True):
        csr = csr_on(dev, "special" + np.dtype(dtype).name, G, idtype, use_eids)
        prob = nc.prob_by_eid(G, w, use_eids, dtype)
        never = [int(G["eids"][p]) if use_eids else p for p in nc.SPECIAL_NEVER]
        inf_eid = int(G["eids"][nc.SPECIAL_INF]) if use_eids else nc.SPECIAL_INF
        for fanout in nc.W_FANOUTS:
            for S in nc.W_SEEDS:
                indptr, src, eids = nc.run_weighted(csr, prob, seeds, fanout, False, S, idtype, dev)
                assert indptr.tolist() == [0, min(fanout, positive)]
                assert not set(eids.tolist()) & set(never) and len(set(eids.tolist())) == len(eids)
                assert eids[0] == inf_eid and src[0] == G["indices"][nc.SPECIAL_INF]
                indptr, src, eids = nc.run_weighted(csr, prob, seeds, fanout, True, S, idtype, dev)
                assert indptr.tolist() == [0, fanout]
                assert (eids == inf_eid).all() and (src == G["indices"][nc.SPECIAL_INF]).all()


# ---- 6. the block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", IDTYPES)
@pytest.mark.parametrize("num_nodes", nc.B_NODES)
def test_block_equals_the_model(dev, idtype, num_nodes):
    node_map = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
    for name, seeds, src in nc.block_cases(num_nodes):
        local, nodes = nc.model_block(seeds, src)
        results = []
        for padded in (False, True):
            got = nc.run_block(seeds, src, node_map, idtype, dev, padded)
            where = (num_nodes, name, "padded" if padded else "plain")
            assert got[2] == len(nodes), where
            assert same(got[0], local, idtype) and same(got[1], nodes, idtype), where
            assert bool((node_map == -1).all()), where
            results.append(got)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0][:2], results[1][:2])), (num_nodes, name)
