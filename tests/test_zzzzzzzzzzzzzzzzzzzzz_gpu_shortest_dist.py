"""Shortest distances and paths on the device (csrc/shortest_dist.hip): device == host twin == the numpy model of
tests/test_shortest_dist_host.py, element for element, on every graph there: both id types, with and without an edge-id
map, all pairs and single roots, with and without a caller's workspace, the masks in LDS and (max_lds_nodes=32) in the
workspace; every path is a path; the refusals, and a workspace whose guard bands stay clean."""
import pytest
import torch

from tests import test_shortest_dist_host as sd
from tests.guarded import POISON_INDEX, guarded

pytestmark = pytest.mark.gpu

CASES = [(name, True) for name in sorted(sd.GRAPHS)] + [("loops_doubles65", False), ("random129", False)]


def csr_pair(name, edge_ids, idtype, dev):
    """(host dgla_csr, device dgla_csr) of the in-edge CSR of a graph, with its edge-id map or without."""
    from dgl_amd import _capi

    n = sd.GRAPHS[name][0]
    host = [torch.from_numpy(a).to(idtype) for a in sd.in_csr(*sd.GRAPHS[name])]
    if not edge_ids:
        host[2] = None
    return _capi.host_csr(*host, n), _capi.make_csr(*[None if t is None else t.to(dev) for t in host], n)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("name,edge_ids", CASES)
def test_device_equals_the_host_twin_and_the_model(dev, name, edge_ids, idtype):
    from dgl_amd import _capi

    n = sd.GRAPHS[name][0]
    h_csr, d_csr = csr_pair(name, edge_ids, idtype, dev)
    model = sd.expected(name, edge_ids)
    own = torch.empty(_capi.shortest_dist_workspace_bytes(idtype, n, n), dtype=torch.uint8, device=dev)
    for root in (None, 0, n - 1):
        src = None if root is None else torch.tensor([root], dtype=idtype)
        want = _capi.shortest_dist_host(h_csr, src, True)
        exact = model if root is None else tuple(t[None] for t in sd.of_root(model, root))
        assert torch.equal(want[0], exact[0]) and torch.equal(want[1], exact[1]), (name, root)
        for ws in (None, own):
            for lds in (None, 32):
                what = (name, root, ws is not None, lds)
                got = _capi.shortest_dist(d_csr, None if src is None else src.to(dev), True, ws=ws, max_lds_nodes=lds)
                assert got[0].is_cuda and got[0].dtype == got[1].dtype == torch.int64, what
                assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), what
                only = _capi.shortest_dist(d_csr, None if src is None else src.to(dev), False, ws=ws, max_lds_nodes=lds)
                assert torch.equal(only.cpu(), want[0]), what


def test_every_path_is_a_path_of_its_length(dev):
    import dgl_amd as dgl

    n, src, dst = (torch.as_tensor(a, device=dev) for a in sd.GRAPHS["random129"])
    dist, paths = dgl.shortest_dist(dgl.graph((src, dst), num_nodes=int(n), device=dev), return_paths=True)
    k = torch.arange(paths.shape[2], device=dev)
    on = k < dist[:, :, None]                                               # the steps of every path; the rest is padding
    e = paths.clamp(min=0)
    s, v = torch.meshgrid(torch.arange(int(n), device=dev), torch.arange(int(n), device=dev), indexing="ij")
    leaves = torch.where(k == 0, s[:, :, None], dst[e].roll(1, dims=2))     # step k leaves where step k - 1 arrived
    arrives = torch.where(k == dist[:, :, None] - 1, v[:, :, None], dst[e])
    assert paths.shape[2] == dist.max() and torch.equal(paths >= 0, on) and torch.equal(paths[~on], -torch.ones_like(paths[~on])) \
        and torch.equal(src[e][on], leaves[on]) and torch.equal(dst[e][on], arrives[on])


def test_refusals_and_a_guarded_call_afterwards(dev):
    import dgl_amd as dgl
    from dgl_amd import _capi

    n, src, dst = sd.GRAPHS["random65"]
    g = dgl.graph((torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)), num_nodes=n, device=dev)
    d_csr = csr_pair("random65", True, torch.int64, dev)[1]
    with pytest.raises(dgl.DGLAMDError, match=r"shortest_dist: the root 65 lies outside \[0, 65\)"):
        dgl.shortest_dist(g, root=65)
    with pytest.raises(dgl.DGLAMDError, match=r"shortest_dist: a source lies outside \[0, 65\)"):
        _capi.shortest_dist(d_csr, torch.tensor([3, -2], device=dev), True)
    need = _capi.shortest_dist_workspace_bytes(torch.int64, n, n)
    with pytest.raises(dgl.DGLAMDError, match="shortest_dist: workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.shortest_dist(d_csr, None, True, ws=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    with pytest.raises(dgl.DGLAMDError, match="shortest_dist: takes a homogeneous graph"):
        dgl.shortest_dist(dgl.heterograph({("a", "x", "b"): ([0], [0])}, device=dev))
    ws = guarded(dev, need, torch.uint8, poison=POISON_INDEX)               # exactly the bytes the query reports
    for lds in (None, 32):
        got = _capi.shortest_dist(d_csr, None, True, ws=ws.t, max_lds_nodes=lds)
        ws.check("the workspace of shortest_dist, max_lds_nodes=%s" % lds)
        assert torch.equal(got[0].cpu(), sd.expected("random65")[0]) and torch.equal(got[1].cpu(), sd.expected("random65")[1])
    both = dgl.shortest_dist(g, root=64, return_paths=True)
    assert both[0].device == g.device and torch.equal(both[1].cpu(), sd.of_root(sd.expected("random65"), 64)[1])
