"""Graph construction helpers around the hot path, in torch index arithmetic on the caller's device.

``add_self_loop`` / ``remove_self_loop`` / ``remove_edges`` / ``reorder_graph`` / ``add_reverse_edges`` / ``to_simple`` /
``to_bidirected`` (python/dgl/transforms/functional.py), ``node_subgraph`` / ``edge_subgraph`` / ``in_subgraph``
(python/dgl/subgraph.py),
``batch`` (python/dgl/batch.py), ``from_scipy`` / ``bipartite_from_scipy`` (python/dgl/convert.py), ``adj_external``
(heterograph.py): the handful the reference's own layer tests
(tests/python/pytorch/nn/test_nn.py, tests/utils/graph_cases.py) build their graphs with — tools/ref_suite runs those
files unmodified.  None of this is a kernel and none of it is timed; every graph these return builds its CSR / CSC with
the library's COO -> CSR kernel the first time an operator asks for it, like any other graph.

``knn`` / ``knn_graph`` / ``segmented_knn_graph`` (python/dgl/transforms/functional.py:111-278, 337-488, 641-785) are the
exception: graph construction from coordinates is a hot path (EdgeConv rebuilds the graph in every layer) and runs the
k-NN kernel of csrc/knn.hip.
"""
import warnings

import torch

from . import function as fn
from ._lib import DGLAMDError
from .graph_index import GraphIndex, Relation
from .heterograph import DGLGraph, _Frame, graph, heterograph

EID = NID = "_ID"


def _single(g, what):
    if len(g.canonical_etypes) != 1:
        raise DGLAMDError("%s: an edge type must be given on a graph with several edge types" % what)


def _with_edges(g, etid, u, v, edge_frame):
    """Copy of ``g`` whose relation ``etid`` has the edges (u, v) and the given edge frame; everything else shared."""
    rels = list(g._graph.relations)
    old = rels[etid]
    rels[etid] = Relation(old.num_src, old.num_dst, u.contiguous(), v.contiguous(), idtype=g.idtype, device=g.device)
    gidx = GraphIndex([g._graph.num_nodes(i) for i in range(len(g._ntypes))], list(g._graph.metagraph.edges), rels)
    eframes = [g._copy_frame(f) for f in g._edge_frames]
    eframes[etid] = edge_frame
    return DGLGraph(gidx, g._ntypes, g._canonical_etypes, [g._copy_frame(f) for f in g._node_frames], eframes,
                    g._src_ntype_ids, g._dst_ntype_ids)


def add_self_loop(g, edge_feat_names=None, fill_data=1.0, etype=None):
    """One edge i -> i per node, appended behind the existing edges; their features are ``fill_data`` — a number, or
    'sum' / 'mean' / 'max' / 'min' of the node's incoming edges' features (transforms/functional.py add_self_loop)."""
    etid = g.get_etype_id(etype)
    s, d = g._graph.metagraph.find_edge(etid)
    if s != d:
        raise DGLAMDError("add_self_loop does not support unidirectional bipartite graphs: {}. Please make sure the types "
                          "of head node and tail node are identical.".format(g.canonical_etypes[etid]))
    n = g._graph.num_nodes(s)
    u, v = g.edges(etype=g.canonical_etypes[etid])
    loop = torch.arange(n, dtype=g.idtype, device=g.device)
    old = g._edge_frames[etid]
    frame = _Frame(int(u.shape[0]) + n)
    for k, col in old.items():
        shape = (n,) + tuple(col.shape[1:])
        if edge_feat_names is not None and k not in edge_feat_names:
            # not named: the feature stays, the new self-loop rows are zero (the reference goes through add_edges(data=...))
            dict.__setitem__(frame, k, torch.cat([col, torch.zeros(shape, dtype=col.dtype, device=col.device)], 0))
            continue
        if isinstance(fill_data, str):
            if fill_data not in ("sum", "mean", "max", "min"):
                raise DGLAMDError("Unsupported aggregation: {}".format(fill_data))
            idx = v.long().view((-1,) + (1,) * (col.dim() - 1)).expand_as(col)
            op = {"sum": "sum", "mean": "mean", "max": "amax", "min": "amin"}[fill_data]
            add = torch.zeros(shape, dtype=col.dtype, device=col.device).scatter_reduce(0, idx, col, op, include_self=False)
        else:
            add = torch.full(shape, fill_data, dtype=col.dtype, device=col.device)
        dict.__setitem__(frame, k, torch.cat([col, add], 0))
    return _with_edges(g, etid, torch.cat([u, loop]), torch.cat([v, loop]), frame)


def remove_edges(g, eids, etype=None, store_ids=False):
    """Copy of ``g`` without the given edges of one type; the others keep their relative order (functional.py)."""
    etid = g.get_etype_id(etype)
    u, v = g.edges(etype=g.canonical_etypes[etid])
    keep = torch.ones(u.shape[0], dtype=torch.bool, device=g.device)
    keep[torch.as_tensor(eids, device=g.device).long()] = False
    sel = torch.nonzero(keep).reshape(-1)
    frame = _Frame(int(sel.shape[0]))
    for k, col in g._edge_frames[etid].items():
        dict.__setitem__(frame, k, col[sel])
    if store_ids:
        dict.__setitem__(frame, EID, sel.to(g.idtype))
    out = _with_edges(g, etid, u[sel], v[sel], frame)
    if store_ids:
        for i in range(len(out._ntypes)):
            out._node_frames[i][NID] = torch.arange(out._graph.num_nodes(i), dtype=g.idtype, device=g.device)
    return out


def remove_self_loop(g, etype=None):
    etid = g.get_etype_id(etype)
    u, v = g.edges(etype=g.canonical_etypes[etid])
    return remove_edges(g, torch.nonzero(u == v).reshape(-1), etype=etype)


def reorder_graph(g, node_permute_algo=None, edge_permute_algo="src", store_ids=True, permute_config=None):
    """Edges re-ordered by source / destination id or by a given permutation (functional.py reorder_graph; node
    re-ordering — rcmk / metis — is the reference's graph-partitioning tool chain and is not offered)."""
    if node_permute_algo is not None:
        raise DGLAMDError("reorder_graph: node_permute_algo is not supported (only edges are re-ordered)")
    _single(g, "reorder_graph")
    u, v = g.edges()
    if edge_permute_algo == "src":
        perm = torch.argsort(u, stable=True)
    elif edge_permute_algo == "dst":
        perm = torch.argsort(v, stable=True)
    elif edge_permute_algo == "custom":
        if not permute_config or "edges_perm" not in permute_config:
            raise DGLAMDError("edge_permute_algo='custom' needs permute_config['edges_perm']")
        perm = torch.as_tensor(permute_config["edges_perm"], device=g.device)
        if perm.shape[0] != u.shape[0]:
            raise DGLAMDError("edges_perm must hold one entry per edge")
    else:
        raise DGLAMDError("Unexpected edge_permute_algo is specified: {}. Expected algos: ['src', 'dst', 'custom']"
                          .format(edge_permute_algo))
    perm = perm.long()
    frame = _Frame(int(u.shape[0]))
    for k, col in g._edge_frames[0].items():
        dict.__setitem__(frame, k, col[perm])
    if store_ids:
        dict.__setitem__(frame, EID, perm.to(g.idtype))
    return _with_edges(g, 0, u[perm], v[perm], frame)


def batch(graphs, ndata="__ALL__", edata="__ALL__"):
    """Disjoint union with node / edge ids shifted graph by graph (python/dgl/batch.py); ``batch_num_nodes()`` /
    ``batch_num_edges()`` give the pieces."""
    if len(graphs) == 0:
        raise DGLAMDError("The input list of graphs cannot be empty.")
    g0 = graphs[0]
    for g in graphs[1:]:
        if g.ntypes != g0.ntypes or g.canonical_etypes != g0.canonical_etypes:
            raise DGLAMDError("All graphs should have the same node types and edge types to be batched.")
    nts, cets = g0.ntypes, g0.canonical_etypes
    counts = {n: [g.num_nodes(n) for g in graphs] for n in nts}
    offs = {n: [sum(counts[n][:i]) for i in range(len(graphs))] for n in nts}
    data = {}
    for c in cets:
        us, vs = [], []
        for i, g in enumerate(graphs):
            u, v = g.edges(etype=c)
            us.append(u + offs[c[0]][i])
            vs.append(v + offs[c[2]][i])
        data[c] = (torch.cat(us), torch.cat(vs))
    total = {n: sum(counts[n]) for n in nts}
    if len(cets) == 1 and len(nts) == 1:
        out = graph(data[cets[0]], num_nodes=total[nts[0]], idtype=g0.idtype, device=g0.device)
    else:
        out = heterograph(data, total, idtype=g0.idtype, device=g0.device)
    def merge(frames, keys):
        merged = {}
        names = list(frames[0].keys()) if keys == "__ALL__" else (keys or [])
        for k in names:
            if all(k in f for f in frames):
                merged[k] = torch.cat([f[k] for f in frames], 0)
        return merged
    for i, n in enumerate(out._ntypes):
        for k, val in merge([g._node_frames[g.get_ntype_id(n)] for g in graphs], ndata).items():
            out._node_frames[i][k] = val
    for i, c in enumerate(out._canonical_etypes):
        for k, val in merge([g._edge_frames[g.get_etype_id(c)] for g in graphs], edata).items():
            out._edge_frames[i][k] = val
    out._batch_num_nodes = {n: torch.tensor(counts[n], dtype=g0.idtype, device=g0.device) for n in nts}
    out._batch_num_edges = {c: torch.tensor([g.num_edges(c) for g in graphs], dtype=g0.idtype, device=g0.device) for c in cets}
    out.batch_size = len(graphs)
    return out


def unbatch(g, node_split=None, edge_split=None):
    """The graphs a batch was made of, with their slices of the features (python/dgl/batch.py unbatch)."""
    nts, cets = g.ntypes, g.canonical_etypes
    nsplit = {n: (g.batch_num_nodes(n) if node_split is None else torch.as_tensor(
        node_split[n] if isinstance(node_split, dict) else node_split)).tolist() for n in nts}
    esplit = {c: (g.batch_num_edges(c) if edge_split is None else torch.as_tensor(
        edge_split[c] if isinstance(edge_split, dict) else edge_split)).tolist() for c in cets}
    k = len(nsplit[nts[0]])
    noff = {n: [sum(nsplit[n][:i]) for i in range(k + 1)] for n in nts}
    eoff = {c: [sum(esplit[c][:i]) for i in range(k + 1)] for c in cets}
    out = []
    for i in range(k):
        data = {}
        for c in cets:
            u, v = g.edges(etype=c)
            a, b = eoff[c][i], eoff[c][i + 1]
            data[c] = (u[a:b] - noff[c[0]][i], v[a:b] - noff[c[2]][i])
        counts = {n: nsplit[n][i] for n in nts}
        if len(cets) == 1 and len(nts) == 1:
            sg = graph(data[cets[0]], num_nodes=counts[nts[0]], idtype=g.idtype, device=g.device)
        else:
            sg = heterograph(data, counts, idtype=g.idtype, device=g.device)
        for n in nts:
            fr = g._node_frames[g.get_ntype_id(n)]
            for key, val in fr.items():
                sg._node_frames[sg.get_ntype_id(n)][key] = val[noff[n][i]:noff[n][i + 1]]
        for c in cets:
            fr = g._edge_frames[g.get_etype_id(c)]
            for key, val in fr.items():
                sg._edge_frames[sg.get_etype_id(c)][key] = val[eoff[c][i]:eoff[c][i + 1]]
        out.append(sg)
    return out


def from_scipy(sp_mat, eweight_name=None, idtype=None, device=None):
    """Graph with an edge row -> column per nonzero of a square scipy sparse matrix (convert.py from_scipy)."""
    if sp_mat.shape[0] != sp_mat.shape[1]:
        raise DGLAMDError("Expect the number of rows to be the same as the number of columns for sp_mat, got {:d} and {:d}."
                          .format(sp_mat.shape[0], sp_mat.shape[1]))
    coo = sp_mat.tocoo()
    g = graph((torch.as_tensor(coo.row).long(), torch.as_tensor(coo.col).long()), num_nodes=sp_mat.shape[0],
              idtype=idtype or torch.int64, device=device or torch.device("cpu"))
    if eweight_name is not None:
        g.edata[eweight_name] = torch.as_tensor(coo.data).to(g.device)
    return g


def bipartite_from_scipy(sp_mat, utype, etype, vtype, eweight_name=None, idtype=None, device=None):
    coo = sp_mat.tocoo()
    g = heterograph({(utype, etype, vtype): (torch.as_tensor(coo.row).long(), torch.as_tensor(coo.col).long())},
                    {utype: sp_mat.shape[0], vtype: sp_mat.shape[1]}, idtype=idtype or torch.int64,
                    device=device or torch.device("cpu"))
    if eweight_name is not None:
        g.edata[eweight_name] = torch.as_tensor(coo.data).to(g.device)
    return g


def adj_external(g, transpose=False, ctx=None, scipy_fmt=None, etype=None):
    """Adjacency matrix as a torch sparse COO tensor — rows = source nodes unless ``transpose`` — or a scipy matrix
    (heterograph.py adj_external)."""
    c = g.to_canonical_etype(etype)
    u, v = g.edges(etype=c)
    n_src, n_dst = g.num_src_nodes(c[0]) if g.is_unibipartite else g.num_nodes(c[0]), \
        g.num_dst_nodes(c[2]) if g.is_unibipartite else g.num_nodes(c[2])
    if scipy_fmt is not None:
        import numpy as np
        import scipy.sparse as sp

        rows, cols, shape = (v, u, (n_dst, n_src)) if transpose else (u, v, (n_src, n_dst))
        mat = sp.coo_matrix((np.ones(int(u.shape[0])), (rows.cpu().numpy(), cols.cpu().numpy())), shape=shape)
        return mat.asformat(scipy_fmt)
    idx = torch.stack([v, u] if transpose else [u, v]).long()
    shape = (n_dst, n_src) if transpose else (n_src, n_dst)
    out = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], device=idx.device), shape)
    return out.to(ctx) if ctx is not None else out


def _homogeneous(g, what):
    if len(g.ntypes) != 1 or len(g.canonical_etypes) != 1:
        raise DGLAMDError("%s only supports homogeneous graphs; convert with to_homogeneous first" % what)


def add_reverse_edges(g, readonly=None, copy_ndata=True, copy_edata=False, ignore_bipartite=False, exclude_self=True):  # noqa: ARG001
    """Every edge (u, v) followed by its reverse (v, u), appended behind the existing edges — self-loops are not doubled
    when ``exclude_self`` (transforms/functional.py add_reverse_edges); reverse edges get a copy of their edge's features
    when ``copy_edata``."""
    _homogeneous(g, "add_reverse_edges")
    u, v = g.edges()
    keep = (u != v) if exclude_self else torch.ones_like(u, dtype=torch.bool)
    ru, rv = v[keep], u[keep]
    out = graph((torch.cat([u, ru]), torch.cat([v, rv])), num_nodes=g.num_nodes(), idtype=g.idtype, device=g.device)
    if copy_ndata:
        for k, val in g._node_frames[0].items():
            out._node_frames[0][k] = val
    if copy_edata:
        for k, val in g._edge_frames[0].items():
            out._edge_frames[0][k] = torch.cat([val, val[keep]], 0)
    return out


def to_simple(g, return_counts="count", writeback_mapping=False, copy_ndata=True, copy_edata=False):  # noqa: ARG001
    """Parallel edges merged into one, edges ordered by (source, destination); ``edata[return_counts]`` = multiplicity
    (functional.py to_simple).  With ``writeback_mapping`` also returns, per original edge, the id of its merged edge."""
    _homogeneous(g, "to_simple")
    u, v = g.edges()
    n = max(g.num_nodes(), 1)
    key = u.long() * n + v.long()
    uniq, inverse, counts = torch.unique(key, sorted=True, return_inverse=True, return_counts=True)
    out = graph(((uniq // n).to(g.idtype), (uniq % n).to(g.idtype)), num_nodes=g.num_nodes(), idtype=g.idtype, device=g.device)
    if return_counts is not None:
        out.edata[return_counts] = counts
    if copy_ndata:
        for k, val in g._node_frames[0].items():
            out._node_frames[0][k] = val
    return (out, inverse.to(g.idtype)) if writeback_mapping else out


def to_bidirected(g, copy_ndata=False, readonly=None):  # noqa: ARG001
    """A simple graph with both directions of every edge (functional.py to_bidirected): reverse edges added, parallel edges
    merged; edge features are not carried (there is no single value for a merged edge)."""
    _homogeneous(g, "to_bidirected")
    both = add_reverse_edges(g, copy_ndata=copy_ndata, copy_edata=False, exclude_self=True)
    return to_simple(both, return_counts=None, copy_ndata=copy_ndata)


def _induced(g, node_ids_per_type, edge_ids_per_etype, relabel_nodes, store_ids):
    """Subgraph from per-etype edge ids (and, when relabelling, per-type node ids in their new order)."""
    nts, cets = g.ntypes, g.canonical_etypes
    dev, idt = g.device, g.idtype
    if relabel_nodes:
        maps = {}
        for n in nts:
            ids = node_ids_per_type[n].long()
            m = torch.full((max(g.num_nodes(n), 1),), -1, dtype=torch.long, device=dev)
            m[ids] = torch.arange(ids.shape[0], device=dev)
            maps[n] = m
        counts = {n: int(node_ids_per_type[n].shape[0]) for n in nts}
    else:
        counts = {n: g.num_nodes(n) for n in nts}
    data = {}
    for c in cets:
        u, v = g.edges(etype=c)
        e = edge_ids_per_etype[c].long()
        uu, vv = u[e].long(), v[e].long()
        if relabel_nodes:
            uu, vv = maps[c[0]][uu], maps[c[2]][vv]
        data[c] = (uu.to(idt), vv.to(idt))
    return _assemble(g, data, counts, node_ids_per_type, edge_ids_per_etype, relabel_nodes, store_ids)


def _assemble(g, data, counts, node_ids_per_type, edge_ids_per_etype, relabel_nodes, store_ids):
    """The subgraph with edges ``data`` and node counts ``counts``, the features of ``g`` following its nodes and edges."""
    nts, cets = g.ntypes, g.canonical_etypes
    dev, idt = g.device, g.idtype
    if len(cets) == 1 and len(nts) == 1:
        out = graph(data[cets[0]], num_nodes=counts[nts[0]], idtype=idt, device=dev)
    else:
        out = heterograph(data, counts, idtype=idt, device=dev)
    for n in nts:
        fr = g._node_frames[g.get_ntype_id(n)]
        of = out._node_frames[out.get_ntype_id(n)]
        for k, val in fr.items():
            of[k] = val[node_ids_per_type[n].long()] if relabel_nodes else val
        if store_ids and relabel_nodes:
            of[NID] = node_ids_per_type[n].to(idt)
    for c in cets:
        fr = g._edge_frames[g.get_etype_id(c)]
        of = out._edge_frames[out.get_etype_id(c)]
        for k, val in fr.items():
            of[k] = val[edge_ids_per_etype[c].long()]
        if store_ids:
            of[EID] = edge_ids_per_etype[c].to(idt)
    return out


def _per_type(g, x, names, what):
    if isinstance(x, dict):
        return {k: torch.as_tensor(v, device=g.device) for k, v in x.items()}
    if len(names) != 1:
        raise DGLAMDError("%s: a dict keyed by type is needed on a graph with several types" % what)
    return {names[0]: torch.as_tensor(x, device=g.device)}


def _ids_of(t, n):
    return torch.nonzero(t).reshape(-1) if t.dtype == torch.bool else t.reshape(-1)


def node_subgraph(g, nodes, relabel_nodes=True, store_ids=True, output_device=None):
    """Subgraph induced on the given nodes (ids or a boolean mask; a dict per node type on heterographs): every edge whose
    two ends are kept, in edge-id order (python/dgl/subgraph.py node_subgraph)."""
    nodes = _per_type(g, nodes, g.ntypes, "node_subgraph")
    ids = {n: _ids_of(nodes[n], g.num_nodes(n)) if n in nodes else torch.empty(0, dtype=torch.long, device=g.device) for n in g.ntypes}
    inside = {}
    for n in g.ntypes:
        m = torch.zeros(max(g.num_nodes(n), 1), dtype=torch.bool, device=g.device)
        m[ids[n].long()] = True
        inside[n] = m
    eids = {}
    for c in g.canonical_etypes:
        u, v = g.edges(etype=c)
        eids[c] = torch.nonzero(inside[c[0]][u.long()] & inside[c[2]][v.long()]).reshape(-1)
    out = _induced(g, ids, eids, relabel_nodes, store_ids)
    return out.to(output_device) if output_device is not None else out


def edge_subgraph(g, edges, relabel_nodes=True, store_ids=True, output_device=None):
    """Subgraph of the given edges (ids or a boolean mask; a dict per edge type), its nodes the edges' end points in
    ascending id order when relabelled (subgraph.py edge_subgraph)."""
    edges = _per_type(g, edges, g.canonical_etypes if len(g.canonical_etypes) == 1 else g.etypes, "edge_subgraph")
    eids = {}
    for c in g.canonical_etypes:
        t = edges.get(c, edges.get(c[1]))
        eids[c] = _ids_of(t, g.num_edges(c)) if t is not None else torch.empty(0, dtype=torch.long, device=g.device)
    ids = {}
    for n in g.ntypes:
        parts = []
        for c in g.canonical_etypes:
            u, v = g.edges(etype=c)
            e = eids[c].long()
            if c[0] == n:
                parts.append(u[e].long())
            if c[2] == n:
                parts.append(v[e].long())
        ids[n] = torch.unique(torch.cat(parts)) if parts else torch.empty(0, dtype=torch.long, device=g.device)
    out = _induced(g, ids, eids, relabel_nodes, store_ids)
    return out.to(output_device) if output_device is not None else out


def in_subgraph(g, nodes, relabel_nodes=False, store_ids=True, output_device=None):
    """Every inbound edge of the given nodes, all nodes kept unless ``relabel_nodes`` (subgraph.py in_subgraph)."""
    nodes = _per_type(g, nodes, g.ntypes, "in_subgraph")
    eids = {}
    for c in g.canonical_etypes:
        u, v = g.edges(etype=c)
        if c[2] in nodes:
            m = torch.zeros(max(g.num_nodes(c[2]), 1), dtype=torch.bool, device=g.device)
            m[_ids_of(nodes[c[2]], 0).long()] = True
            eids[c] = torch.nonzero(m[v.long()]).reshape(-1)
        else:
            eids[c] = torch.empty(0, dtype=torch.long, device=g.device)
    if not relabel_nodes:
        out = _induced(g, None, eids, False, store_ids)
    else:
        ids = {}
        for n in g.ntypes:
            parts = [_ids_of(nodes[n], 0).long()] if n in nodes else []
            for c in g.canonical_etypes:
                u, v = g.edges(etype=c)
                e = eids[c].long()
                if c[0] == n:
                    parts.append(u[e].long())
                if c[2] == n:
                    parts.append(v[e].long())
            ids[n] = torch.unique(torch.cat(parts)) if parts else torch.empty(0, dtype=torch.long, device=g.device)
        out = _induced(g, ids, eids, True, store_ids)
    return out.to(output_device) if output_device is not None else out


def out_subgraph(g, nodes, relabel_nodes=False, store_ids=True, output_device=None):
    """Every outbound edge of the given nodes, all nodes kept unless ``relabel_nodes`` (subgraph.py out_subgraph): the
    mirror image of :func:`in_subgraph`."""
    nodes = _per_type(g, nodes, g.ntypes, "out_subgraph")
    eids = {}
    for c in g.canonical_etypes:
        u, v = g.edges(etype=c)
        if c[0] in nodes:
            m = torch.zeros(max(g.num_nodes(c[0]), 1), dtype=torch.bool, device=g.device)
            m[_ids_of(nodes[c[0]], 0).long()] = True
            eids[c] = torch.nonzero(m[u.long()]).reshape(-1)
        else:
            eids[c] = torch.empty(0, dtype=torch.long, device=g.device)
    if not relabel_nodes:
        out = _induced(g, None, eids, False, store_ids)
    else:
        ids = {}
        for n in g.ntypes:
            parts = [_ids_of(nodes[n], 0).long()] if n in nodes else []
            for c in g.canonical_etypes:
                u, v = g.edges(etype=c)
                e = eids[c].long()
                if c[0] == n:
                    parts.append(u[e].long())
                if c[2] == n:
                    parts.append(v[e].long())
            ids[n] = torch.unique(torch.cat(parts)) if parts else torch.empty(0, dtype=torch.long, device=g.device)
        out = _induced(g, ids, eids, True, store_ids)
    return out.to(output_device) if output_device is not None else out


def _induced_rows(g, ids_per_type, relabel_nodes=True, store_ids=True):
    """The node-induced subgraph of a GPU graph in O(sum of the selected nodes' in-degrees): what :func:`node_subgraph`
    returns for the id lists ``ids_per_type`` ({node type: ids}, local ids in list order), cut by the kernels of
    csrc/subgraph.hip.  Every node type's map is marked once, every relation is swept over its in-edge CSR (count, ONE
    read-back of (total, flags), fill in edge-id order), and the maps are cleared again whatever happens.  A duplicate or
    out-of-range id raises ``DGLAMDError``."""
    from . import _capi
    from .sampling import _node_map

    if g.device.type != "cuda":
        raise DGLAMDError("_induced_rows runs on a GPU graph; use node_subgraph on %s" % g.device)
    nts, cets = g.ntypes, g.canonical_etypes
    dev, idt = g.device, g.idtype
    ids = {n: (torch.as_tensor(ids_per_type[n]).reshape(-1).to(device=dev, dtype=idt).contiguous() if n in ids_per_type
               else torch.empty(0, dtype=idt, device=dev)) for n in nts}
    maps = {n: _node_map(g, dev, None if len(nts) == 1 else i) for i, n in enumerate(nts)}
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    data, eids, checked = {}, {}, False
    try:
        for n in nts:
            _capi.node_map_mark(ids[n], maps[n], flags)
        for etid, c in enumerate(cets):
            rel = g._graph.relations[etid]
            if rel.num_edges == 0 or ids[c[2]].shape[0] == 0:
                row = col = eid = torch.empty(0, dtype=idt, device=dev)
            else:
                indptr, indices, emap = rel.csc()
                csr = _capi.make_csr(indptr, indices, emap, rel.num_src)
                _, row, col, eid = _capi.induced_subgraph(csr, ids[c[2]], maps[c[0]], eid_order=True, flags=flags)
                checked = True
            data[c], eids[c] = (col, row), eid          # (rows of the in-edge CSR are destinations)
        if not checked:
            _capi._flag_error("induced_subgraph", int(flags.item()))
    finally:
        for n in nts:
            _capi.node_map_clear(ids[n], maps[n])
    if relabel_nodes:
        counts = {n: int(ids[n].shape[0]) for n in nts}
    else:
        counts = {n: g.num_nodes(n) for n in nts}
        data = {c: (ids[c[0]][u.long()], ids[c[2]][v.long()]) for c, (u, v) in data.items()}
    return _assemble(g, data, counts, ids, eids, relabel_nodes, store_ids)


def _compact_nodes_torch(preserve, ends, num_nodes):
    """The compaction rule of include/dgl_amd.h ("Edge exclusion and compaction") in torch index arithmetic, for a CPU
    graph: ``preserve`` in the order given (a repeated id at its first position), then the other ids of ``ends``
    ascending.  Returns ``(local ids of ends, nodes)``."""
    dev = ends.device
    p, e = preserve.long(), ends.long()
    if p.numel() and (int(p.min()) < 0 or int(p.max()) >= num_nodes):
        raise DGLAMDError("compact_graphs: node id out of range in always_preserve")
    if p.numel():
        uniq, inv = torch.unique(p, return_inverse=True)
        at = torch.arange(p.shape[0], device=dev)
        first = torch.full((uniq.shape[0],), p.shape[0], dtype=torch.long, device=dev).scatter_reduce(0, inv, at, "amin")
        p = p[first[inv] == at]
    mark = torch.full((max(1, num_nodes),), -1, dtype=torch.long, device=dev)
    mark[p] = torch.arange(p.shape[0], device=dev)
    new = torch.unique(e[mark[e] < 0])
    mark[new] = p.shape[0] + torch.arange(new.shape[0], device=dev)
    return mark[e].to(ends.dtype), torch.cat([p, new]).to(ends.dtype)


def compact_graphs(graphs, always_preserve=None, copy_ndata=True, copy_edata=True):
    """``dgl.compact_graphs`` (python/dgl/transforms/functional.py compact_graphs): the graphs (one, or a list over the
    same node space) with every node dropped that is not an end point of an edge of ANY of them, except the ids of
    ``always_preserve`` (ids, or a dict per node type).  All returned graphs share one node space, stored as
    ``ndata[dgl.NID]``; edge order and edge features are the input's.

    The node order is the block rule of ``to_block``, per node type: the ``always_preserve`` ids in the order given (a
    repeated id keeps its first position), then every other end point ascending.  (The reference's CPU order is first
    appearance and its GPU order is unspecified.)  A GPU graph runs csrc/exclude.hip (dgla_compact_nodes) with ONE
    read-back per node type; a CPU graph follows the same rule in torch.  Blocks are refused."""
    as_list = isinstance(graphs, (list, tuple))
    graphs = list(graphs) if as_list else [graphs]
    if not graphs:
        return []
    g0 = graphs[0]
    nts, dev, idt = g0.ntypes, g0.device, g0.idtype
    for g in graphs:
        if g.is_block:
            raise DGLAMDError("compact_graphs: a block is refused (its source and destination nodes are two node spaces)")
        if g.ntypes != nts:
            raise DGLAMDError("compact_graphs: all graphs must have the same node types in the same order")
        if g.idtype != idt or g.device != dev:
            raise DGLAMDError("compact_graphs: all graphs must have the same idtype and device, got %s / %s and %s / %s"
                              % (idt, dev, g.idtype, g.device))
        for n in nts:
            if g.num_nodes(n) != g0.num_nodes(n):
                raise DGLAMDError("compact_graphs: the graphs disagree on the number of nodes of type %s (%d and %d)"
                                  % (n, g0.num_nodes(n), g.num_nodes(n)))
    if always_preserve is None:
        always_preserve = {}
    elif not isinstance(always_preserve, dict):
        if len(nts) != 1:
            raise DGLAMDError("compact_graphs: always_preserve must be a dict of node type -> ids on a graph with "
                              "several node types")
        always_preserve = {nts[0]: always_preserve}
    for n in always_preserve:
        if n not in nts:
            raise DGLAMDError('Node type "{}" does not exist.'.format(n))
    edges = [{c: g.edges(etype=c) for c in g.canonical_etypes} for g in graphs]
    local, nodes = {}, {}       # local: (graph, canonical etype, end) -> ids in the compact space
    for ntid, n in enumerate(nts):
        keys, parts = [], []
        for gi, g in enumerate(graphs):
            for c in g.canonical_etypes:
                for end in (0, 2):
                    if c[end] == n:
                        keys.append((gi, c, end))
                        parts.append(edges[gi][c][end // 2].to(idt))
        ends = torch.cat(parts).contiguous() if parts else torch.empty(0, dtype=idt, device=dev)
        keep = torch.as_tensor(always_preserve.get(n, [])).reshape(-1).to(device=dev, dtype=idt).contiguous()
        if dev.type == "cuda":
            from . import _capi
            from .sampling import _node_map

            try:
                loc, nodes[n] = _capi.compact_nodes(keep, ends, _node_map(g0, dev, None if len(nts) == 1 else ntid))
            except DGLAMDError as err:
                if "node id out of range" in str(err):
                    raise DGLAMDError("compact_graphs: node id out of range in always_preserve") from None
                raise
        else:
            loc, nodes[n] = _compact_nodes_torch(keep, ends, g0.num_nodes(n))
        at = 0
        for key, part in zip(keys, parts):
            local[key] = loc[at:at + part.shape[0]]
            at += part.shape[0]
    counts = {n: int(nodes[n].shape[0]) for n in nts}
    out = []
    for gi, g in enumerate(graphs):
        cets = g.canonical_etypes
        data = {c: (local[(gi, c, 0)], local[(gi, c, 2)]) for c in cets}
        if len(cets) == 1 and len(nts) == 1:
            new = graph(data[cets[0]], num_nodes=counts[nts[0]], idtype=idt, device=dev)
        else:
            new = heterograph(data, counts, idtype=idt, device=dev)
        for n in nts:
            of = new._node_frames[new.get_ntype_id(n)]
            if copy_ndata:
                for k, val in g._node_frames[g.get_ntype_id(n)].items():
                    of[k] = val[nodes[n].long()]
            of[NID] = nodes[n]
        if copy_edata:
            for c in cets:
                of = new._edge_frames[new.get_etype_id(c)]
                for k, val in g._edge_frames[g.get_etype_id(c)].items():
                    of[k] = val
        out.append(new)
    return out if as_list else out[0]


def _all_neighbors(rel, frontier, direction):
    """The predecessors (``"in"``) or successors (``"out"``) of ``frontier`` over relation ``rel``, with repeats: the
    device's all-neighbour pick on a GPU graph, the same rows of the CSC / CSR in index arithmetic on a CPU graph."""
    indptr, indices, emap = rel.csc() if direction == "in" else rel.csr()
    if rel.device.type == "cuda":
        from . import _capi

        csr = _capi.make_csr(indptr, indices, emap, rel.num_src if direction == "in" else rel.num_dst)
        return _capi.sample_neighbors(csr, frontier.contiguous(), -1)[1]
    f = frontier.long()
    deg = (indptr[f + 1] - indptr[f]).long()
    total = int(deg.sum())
    first = torch.cumsum(deg, 0) - deg
    pos = torch.repeat_interleave(indptr[f].long() - first, deg, output_size=total) + torch.arange(total)
    return indices[pos]


def _khop_subgraph(g, nodes, k, direction, relabel_nodes, store_ids, output_device):
    who = "khop_%s_subgraph" % direction
    if g.is_block:
        raise DGLAMDError("Extracting subgraph of a block graph is not allowed.")
    is_mapping = isinstance(nodes, dict)
    if not is_mapping:
        if len(g.ntypes) != 1:
            raise DGLAMDError("%s: need a dict of node type and IDs for graph with multiple node types" % who)
        nodes = {g.ntypes[0]: nodes}
    dev, idt = g.device, g.idtype
    seeds = {}
    for n, v in nodes.items():
        if n not in g.ntypes:
            raise DGLAMDError('Node type "{}" does not exist.'.format(n))
        t = torch.as_tensor(v).reshape(-1).to(device=dev, dtype=idt)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= g.num_nodes(n)):
            raise DGLAMDError("%s: node id out of range for node type %s" % (who, n))
        seeds[n] = t
    empty = torch.empty(0, dtype=idt, device=dev)
    last, hops = seeds, [seeds]
    for _ in range(int(k)):
        cur = {n: [] for n in g.ntypes}
        for etid, (s_t, _, d_t) in enumerate(g.canonical_etypes):
            here, there = (d_t, s_t) if direction == "in" else (s_t, d_t)
            frontier = last.get(here, empty)
            rel = g._graph.relations[etid]
            if frontier.numel() and rel.num_edges:
                cur[there].append(_all_neighbors(rel, frontier, direction))
        last = {n: (torch.unique(torch.cat(v)) if v else empty) for n, v in cur.items()}
        hops.append(last)
    khop, inverse = {}, {}
    for n in g.ntypes:
        khop[n], inverse[n] = torch.unique(torch.cat([h.get(n, empty) for h in hops]), return_inverse=True)
    if dev.type == "cuda":
        sg = _induced_rows(g, khop, relabel_nodes, store_ids)
    else:
        sg = node_subgraph(g, khop, relabel_nodes=relabel_nodes, store_ids=store_ids)
    if output_device is not None:
        sg = sg.to(output_device)
    if not relabel_nodes:
        return sg
    inv = {n: inverse[n][:seeds[n].shape[0]] for n in seeds}
    if output_device is not None:
        inv = {n: t.to(output_device) for n, t in inv.items()}
    return sg, (inv if is_mapping else inv[g.ntypes[0]])


def khop_in_subgraph(g, nodes, k, *, relabel_nodes=True, store_ids=True, output_device=None):
    """``dgl.khop_in_subgraph`` (python/dgl/subgraph.py:618-800): the subgraph induced on the ``k``-hop in-neighbourhood
    of ``nodes`` (ids, or a dict per node type on a heterograph), i.e. the nodes themselves and everything that reaches
    them in at most ``k`` steps: per type the ascending distinct ids.  With ``relabel_nodes`` returns
    ``(subgraph, inverse_indices)``, the new ids of ``nodes`` in the form they were given.  On a GPU graph every hop is
    the device's all-neighbour pick and the subgraph is cut by csrc/subgraph.hip; on a CPU graph both steps are torch
    index arithmetic.  Blocks are refused."""
    return _khop_subgraph(g, nodes, k, "in", relabel_nodes, store_ids, output_device)


def khop_out_subgraph(g, nodes, k, *, relabel_nodes=True, store_ids=True, output_device=None):
    """``dgl.khop_out_subgraph`` (python/dgl/subgraph.py:803-985): :func:`khop_in_subgraph` along the out-edges, the nodes
    reached from ``nodes`` in at most ``k`` steps."""
    return _khop_subgraph(g, nodes, k, "out", relabel_nodes, store_ids, output_device)


DGLGraph.subgraph = node_subgraph
DGLGraph.edge_subgraph = edge_subgraph
DGLGraph.in_subgraph = in_subgraph
DGLGraph.out_subgraph = out_subgraph
DGLGraph.khop_in_subgraph = khop_in_subgraph
DGLGraph.khop_out_subgraph = khop_out_subgraph


def adj_product_graph(A, B, weight_name, etype="_E"):
    """Weighted graph whose adjacency matrix is ``adj(A) x adj(B)`` (rows = source nodes, columns = destination nodes;
    transforms/functional.py:2564-2714).  Both graphs must be simple graphs (call :func:`to_simple` first otherwise) with
    one edge type, on the GPU; the number of destination nodes of ``A`` must equal the number of source nodes of ``B``;
    ``edata[weight_name]`` of both is one scalar per edge.  The result goes from ``A``'s source node type to ``B``'s
    destination node type and is homogeneous when the two are the same; its edge type is ``etype`` and its weights are
    in ``edata[weight_name]``, differentiable w.r.t. both inputs.  Unlike scipy, an edge whose weight sums to zero is
    kept.  Edges are listed row by row with ascending destination ids.  If the formats are restricted both graphs must
    allow CSR.  No int32 size limit applies (the reference's cuSPARSE restriction)."""
    from .autograd import csrmm

    _single(A, "adj_product_graph")
    _single(B, "adj_product_graph")
    srctype, _, _ = A.canonical_etypes[0]
    _, _, dsttype = B.canonical_etypes[0]
    num_vtypes = 1 if srctype == dsttype else 2
    ntypes = [srctype] if num_vtypes == 1 else [srctype, dsttype]
    C_gidx, C_weights = csrmm(A._graph, A.edata[weight_name], B._graph, B.edata[weight_name], num_vtypes)
    C = DGLGraph(C_gidx, ntypes, [(srctype, etype, dsttype)])
    C.edata[weight_name] = C_weights
    return C


def adj_sum_graph(graphs, weight_name):
    """Weighted graph whose adjacency matrix is the sum of those of ``graphs`` (transforms/functional.py:2717-2821): simple
    graphs with one edge type, the same node types and the same numbers of nodes, on the GPU.  The result has the
    metagraph of the inputs and its weights in ``edata[weight_name]``, differentiable w.r.t. every input; an edge whose
    weight sums to zero is kept.  If the formats are restricted every graph must allow CSR."""
    from .autograd import csrsum

    if len(graphs) == 0:
        raise ValueError("The list of graphs must not be empty.")
    for g in graphs:
        _single(g, "adj_sum_graph")
    C_gidx, C_weights = csrsum([g._graph for g in graphs], [g.edata[weight_name] for g in graphs])
    C = DGLGraph(C_gidx, graphs[0].ntypes, graphs[0].canonical_etypes)
    C.edata[weight_name] = C_weights
    return C


class DGLWarning(UserWarning):
    """The reference's ``dgl.base.DGLWarning``."""


_KNN_ALGORITHMS = ("bruteforce", "bruteforce-blas", "bruteforce-sharemem")


def _segment_list(segs):
    return [int(v) for v in (segs.tolist() if isinstance(segs, torch.Tensor) else segs)]


def _offsets(segs):
    off = [0]
    for n in segs:
        off.append(off[-1] + n)
    return off


def knn(k, x, x_segs, y=None, y_segs=None, algorithm="bruteforce", dist="euclidean"):
    """``dgl.functional.knn`` (python/dgl/transforms/functional.py:641-785): for every row of ``y`` the ``k`` nearest
    rows of ``x`` inside the same segment; ``y=None`` is the self-query.  Returns the reference's ``(2, k * len(y))``
    int64 tensor: row 0 the query ids, row 1 the ids in ``x``, the ``k`` slots of a query next to each other in
    ascending (distance, id) order.

    ``"bruteforce"``, ``"bruteforce-blas"`` and ``"bruteforce-sharemem"`` all run the one device kernel (csrc/knn.hip;
    the rule: include/dgl_amd.h "Point-cloud graphs"): exact, one total order, the same bytes on every run, nothing of
    size N x N.  ``"kd-tree"`` and ``"nn-descent"`` are refused.  ``dist="cosine"`` normalises the rows with the
    reference's ``v / (|v| + 1e-5)`` and uses the same kernel.  ``k`` above the smallest segment of ``x`` is clamped
    with a warning; ``k`` above ``kKnnMaxK`` (64) is refused by the library.  There is no CPU path."""
    from . import _capi

    if algorithm in ("kd-tree", "nn-descent"):
        raise DGLAMDError("knn: algorithm '%s' is not supported: only the exact brute-force kernel runs here (%s)"
                          % (algorithm, ", ".join(_KNN_ALGORITHMS)))
    if algorithm not in _KNN_ALGORITHMS:
        raise DGLAMDError("knn: unknown algorithm %r; expected one of %s" % (algorithm, ", ".join(_KNN_ALGORITHMS)))
    self_query = y is None
    if self_query:
        y, y_segs = x, x_segs
    if x.device != y.device:
        raise DGLAMDError("knn: x and y must be on the same device")
    x_segs, y_segs = _segment_list(x_segs), _segment_list(y_segs)
    min_num_points = min(x_segs) if x_segs else 0
    if k > min_num_points:
        warnings.warn("'k' should be less than or equal to the number of points in 'x'"
                      "expect k <= {0}, got k = {1}, use k = {0}".format(min_num_points, k), DGLWarning, stacklevel=2)
        k = min_num_points
    if k <= 0:
        raise DGLAMDError("Invalid k value. expect k > 0, got k = {}".format(k))
    if x.shape[0] == 0 or y.shape[0] == 0:
        raise DGLAMDError("Find empty point set")
    dist = dist.lower()
    if dist not in ("euclidean", "cosine"):
        raise DGLAMDError("Only ['euclidean', 'cosine'] are supported for distance computation, got {}".format(dist))
    if x.dim() != 2 or y.dim() != 2:
        raise DGLAMDError("knn: x and y must be 2-D")
    if len(x_segs) != len(y_segs):
        raise DGLAMDError("knn: x_segs and y_segs do not match: %d and %d segments" % (len(x_segs), len(y_segs)))
    if dist == "cosine":
        def l2_normalised(v):
            return v / (torch.sqrt(torch.sum(v * v, dim=1, keepdim=True)) + 1e-5)
        x = l2_normalised(x)
        y = None if self_query else l2_normalised(y)
    elif self_query:
        y = None
    return _capi.knn(x.contiguous(), _offsets(x_segs), k, None if y is None else y.contiguous(), _offsets(y_segs))


def _knn_graph_of(x, k, segs, algorithm, dist, exclude_self, batched):
    """The graph of a self-query over the segments ``segs`` of the 2-D ``x`` (``k`` already includes the self edge when
    ``exclude_self``), with the batch information of the reference when ``batched``."""
    out = knn(k, x, segs, algorithm=algorithm, dist=dist)
    n = x.shape[0]
    kk = out.shape[1] // n            # k after clamping
    nbr, qry = out[1].view(n, kk), out[0].view(n, kk)
    if exclude_self:
        # drop the self edge of every node; a node among more than k coincident points may not hold one, and then
        # loses its last (equally distant) neighbour instead: every node keeps kk - 1 (functional.py:257-276)
        is_self = nbr == qry
        drop = torch.where(is_self.any(1), is_self.int().argmax(1), torch.full_like(nbr[:, 0], kk - 1))
        keep = torch.ones_like(is_self).scatter_(1, drop.unsqueeze(1), False)
        nbr, qry, kk = nbr[keep], qry[keep], kk - 1
    g = graph((nbr.reshape(-1), qry.reshape(-1)), num_nodes=n, idtype=torch.int64, device=x.device)
    if batched:
        num_nodes = torch.tensor(segs, dtype=torch.int64, device=x.device)
        g._batch_num_nodes = {g.ntypes[0]: num_nodes}
        g._batch_num_edges = {g.canonical_etypes[0]: kk * num_nodes}
        g.batch_size = len(segs)
    return g


def knn_graph(x, k, algorithm="bruteforce-blas", dist="euclidean", exclude_self=False):
    """``dgl.knn_graph`` (python/dgl/transforms/functional.py:111-278): the graph whose node ``i`` has the ``k`` nearest
    points of ``x[i]`` as predecessors.  A 3-D ``x`` gives one graph per ``x[b]``, batched.  Every algorithm name of
    :func:`knn` runs the device kernel, the default ``"bruteforce-blas"`` included; the neighbour sets are those of
    ``cdist`` + ``topk`` away from ties, ties go to the smaller id.  ``exclude_self`` searches ``k + 1`` and removes the
    self edge, with the reference's repair for more than ``k`` coincident points."""
    if exclude_self:
        k = k + 1
    if k <= 0:
        raise DGLAMDError("Invalid k value. expect k > 0, got k = {}".format(k))
    if x.shape[0] == 0:
        raise DGLAMDError("Find empty point set")
    if x.dim() == 3:
        segs = x.shape[0] * [x.shape[1]]
        return _knn_graph_of(x.reshape(-1, x.shape[2]), k, segs, algorithm, dist, exclude_self, True)
    return _knn_graph_of(x, k, [x.shape[0]], algorithm, dist, exclude_self, False)


def segmented_knn_graph(x, k, segs, algorithm="bruteforce-blas", dist="euclidean", exclude_self=False):
    """``dgl.segmented_knn_graph`` (python/dgl/transforms/functional.py:337-488): :func:`knn_graph` over point sets of
    different sizes stored one after the other in the 2-D ``x``; ``segs`` are their sizes.  The result is batched."""
    if exclude_self:
        k = k + 1
    if k <= 0:
        raise DGLAMDError("Invalid k value. expect k > 0, got k = {}".format(k))
    if x.shape[0] == 0:
        raise DGLAMDError("Find empty point set")
    return _knn_graph_of(x, k, _segment_list(segs), algorithm, dist, exclude_self, True)


__all__ = ["adj_product_graph", "adj_sum_graph", "add_self_loop", "remove_self_loop", "remove_edges", "reorder_graph", "add_reverse_edges", "to_simple", "to_bidirected",
           "node_subgraph", "edge_subgraph", "in_subgraph", "out_subgraph", "khop_in_subgraph", "khop_out_subgraph", "batch", "unbatch", "from_scipy", "bipartite_from_scipy",
           "adj_external", "knn", "knn_graph", "segmented_knn_graph", "DGLWarning"]
