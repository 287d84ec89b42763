"""The keep rule of attention dropout in the fused GAT operator (csrc/gat_dropout.h, include/dgl_amd.h "Training
form") through its host entry point dgla_gat_dropout_mask_host, and the new keywords of the public API — runs without a
GPU.

Statistics.  A keep bit is Bernoulli(1 - p); over n independent bits the keep rate has standard deviation
sqrt(p (1 - p) / n), and two independent masks agree on a bit with probability q = p^2 + (1 - p)^2, so their agreement
rate has standard deviation sqrt(q (1 - q) / n).  Every bar is 5 of those standard deviations (a fair generator misses
it once in 1.7 million draws).  n = 2^20 (eid, head) pairs.  Every figure is printed before it is asserted."""
import inspect
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = [0.1, 0.5, 0.6, 0.9]
HEADS = 8
EDGES = (1 << 20) // HEADS
NEW = ("dgla_gat_attention_train_forward", "dgla_gat_attention_train_backward", "dgla_gat_attention_weights",
       "dgla_gat_dropout_mask_host")


def _mask(seed, p, eids, heads=HEADS):
    from dgl_amd import _capi

    return _capi.gat_dropout_mask_host(seed, p, eids, heads)


def _agreement(a, b, p, what):
    n = a.numel()
    q = p * p + (1 - p) * (1 - p)
    rate = float((a == b).double().mean())
    bar = 5 * math.sqrt(q * (1 - q) / n)
    print("%s p=%.1f: agreement %.5f, expected %.5f, bar +-%.5f" % (what, p, rate, q, bar))
    assert abs(rate - q) <= bar, (what, p, rate, q, bar)


def test_header_declares_and_library_exports_the_new_functions():
    from dgl_amd import _lib

    with open(os.path.join(ROOT, "include", "dgl_amd.h")) as fh:
        text = fh.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert getattr(_lib.LIB, name) is not None          # AttributeError on a library without the symbol
    assert "Philox4x32-10" in text and "threshold = (uint32_t)(p * 16777216.0)" in text
    assert "data ? data[pos] : pos" in text and "WITHOUT dropout" in text


def test_registry_carries_the_new_names():
    from dgl_amd import _ffi

    names = set(_ffi.list_global_func_names())
    for n in ("GATAttentionTrainForward", "GATAttentionTrainBackward", "GATAttentionWeights"):
        assert "dgl_amd._CAPI_" + n in names, n


def test_mask_is_deterministic_and_p0_keeps_everything():
    eids = torch.arange(EDGES)
    a, b = _mask(1234, 0.6, eids), _mask(1234, 0.6, eids)
    assert a.dtype == torch.uint8 and a.shape == (EDGES, HEADS)
    assert a.numpy().tobytes() == b.numpy().tobytes()
    assert set(a.unique().tolist()) == {0, 1}
    assert bool((_mask(1234, 0.0, eids) == 1).all())


def test_mask_does_not_depend_on_the_order_or_the_batch_of_the_edge_ids():
    """The bit is a function of (seed, eid, head) alone: a permuted / strided / 64-bit id list gives the same bits."""
    g = torch.Generator().manual_seed(3)
    eids = torch.randperm(5000, generator=g)
    full = _mask(77, 0.5, torch.arange(5000), heads=5)
    assert torch.equal(_mask(77, 0.5, eids, heads=5), full[eids])
    big = torch.tensor([0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 7, (1 << 62) + 1])
    one = torch.cat([_mask(5, 0.5, big[i:i + 1], heads=9) for i in range(big.numel())])
    assert torch.equal(_mask(5, 0.5, big, heads=9), one)
    # heads 0-3 come from one Philox block, 4-7 from the next: a mask of 3 heads is the prefix of a mask of 9
    assert torch.equal(_mask(5, 0.5, big, heads=3), one[:, :3])


def test_the_generator_is_philox4x32_10():
    """Known answer of Philox4x32-10 (Random123's kat_vectors): key = 0, counter = 0 gives 6627e8d5 e169c58d bc57ac4c
    9b00dbd8.  The mask shows the top 24 bits of a word: head h of edge 0 under seed 0 is kept iff (word[h] >> 8) >= t
    with t = p * 2^24, and every t below 2^24 is a float p exactly — so the largest kept t, found by bisection, is
    word[h] >> 8.  A second vector pins the key and the counter order: seed = 2^32 + 1 bumps both key words, edge id
    2^32 + 2 both counter words, heads 4-7 the block word."""
    # the Python reference used for the second vector reproduces the published vectors itself
    assert _philox4x32_10((0, 0), (0, 0, 0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    zero = torch.zeros(1, dtype=torch.int64)

    def top24(seed, eid, head):
        lo, hi = 0, (1 << 24) - 1                              # invariant: kept at lo (t = 0 keeps everything)
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if int(_mask(seed, mid / 16777216.0, eid, heads=head + 1)[0, head]):
                lo = mid
            else:
                hi = mid - 1
        return lo

    got = [top24(0, zero, h) for h in range(4)]
    print("Philox4x32-10(0, 0) >> 8:", ["%06x" % w for w in got])
    assert got == [0x6627E8, 0xE169C5, 0xBC57AC, 0x9B00DB]
    ref = _philox4x32_10((1, 1), (2, 1, 1, 0))
    got = [top24((1 << 32) + 1, zero + (1 << 32) + 2, 4 + h) for h in range(4)]
    print("second vector:", ["%06x" % w for w in got], "reference", ["%06x" % (w >> 8) for w in ref])
    assert got == [w >> 8 for w in ref]


def _philox4x32_10(key, ctr):
    """Philox4x32-10 as published (Salmon et al., SC'11), in Python integers."""
    k0, k1 = key
    c = list(ctr)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


@pytest.mark.parametrize("p", PS)
def test_keep_rate(p):
    m = _mask(2024, p, torch.arange(EDGES))
    n = m.numel()
    rate = float(m.double().mean())
    bar = 5 * math.sqrt(p * (1 - p) / n)
    print("p=%.1f: keep rate %.5f over %d bits, expected %.5f, bar +-%.5f" % (p, rate, n, 1 - p, bar))
    assert n == 1 << 20 and abs(rate - (1 - p)) <= bar


@pytest.mark.parametrize("p", PS)
def test_seeds_heads_and_edge_ranges_are_independent(p):
    eids = torch.arange(EDGES)
    a = _mask(11, p, eids)
    _agreement(a, _mask(12, p, eids), p, "two seeds")
    _agreement(a, _mask(11 + (1 << 32), p, eids), p, "seeds that differ in the high word")
    wide = _mask(11, p, torch.arange(1 << 19), heads=2)         # 2^20 bits again: heads 0 and 1 of the same edges
    _agreement(wide[:, 0], wide[:, 1], p, "heads 0 and 1")
    _agreement(a, _mask(11, p, eids + EDGES), p, "two disjoint eid ranges")
    _agreement(a[:, :4], a[:, 4:], p, "heads 0-3 and 4-7 (two Philox blocks)")


def test_p_outside_the_half_open_unit_interval_is_an_error():
    from dgl_amd._lib import DGLAMDError

    for p in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(DGLAMDError):
            _mask(1, p, torch.arange(4))


def test_public_api_accepts_the_new_keywords():
    import dgl_amd as dgl

    for fn in (dgl.ops.gat_attention, dgl.nn.gat_attention):
        par = inspect.signature(fn).parameters
        assert par["attn_drop"].default == 0.0 and par["training"].default is True, fn
        assert par["seed"].default is None and par["get_attention"].default is False, fn
    # the existing positional order is kept
    assert list(inspect.signature(dgl.ops.gat_attention).parameters)[:5] == ["graph", "ft", "el", "er", "negative_slope"]
    assert list(inspect.signature(dgl.nn.gat_attention).parameters)[:7] == ["graph", "ft", "el", "er", "negative_slope",
                                                                             "fused", "handoff"]
    m = dgl.nn.GATAttention(negative_slope=0.1, attn_drop=0.6)
    assert isinstance(m, torch.nn.Module) and m.training and m.attn_drop == 0.6 and m.negative_slope == 0.1
    assert not m.eval().training


def test_attn_drop_of_one_raises_on_the_fused_route():
    import dgl_amd as dgl
    from dgl_amd._lib import DGLAMDError

    ft, el, er = torch.ones(4, 2, 8), torch.ones(4, 2, 1), torch.ones(4, 2, 1)
    for bad in (1.0, -0.5, 2.0):
        with pytest.raises(DGLAMDError, match="attn_drop"):
            dgl.ops.gat_attention(None, ft, el, er, attn_drop=bad)
        with pytest.raises(DGLAMDError, match="attn_drop"):
            dgl.nn.gat_attention(None, ft, el, er, fused=True, attn_drop=bad)
