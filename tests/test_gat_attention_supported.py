"""The accepted set of the fused GAT attention operator (dgla_gat_attention_supported, include/dgl_amd.h) — runs
without a GPU.  The rule, restated here independently of the library: with s = sizeof(element),
V = min(16 / s, largest power of two dividing D) and LPH = next_pow2(ceil(D / V)), a call is taken iff the dtype is
fp32 / fp16 / bf16, H >= 1, D >= 1 and H * LPH <= 64."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, F16, BF16 = 0, 1, 2, 3        # dgla_dtype


def _rule(dtype, h, d):
    s = {F32: 4, F16: 2, BF16: 2}.get(dtype)
    if s is None or h < 1 or d < 1:
        return 0
    v = 16 // s
    while d % v:
        v //= 2
    lanes, lph = -(-d // v), 1
    while lph < lanes:
        lph *= 2
    return int(h * lph <= 64)


def _fn():
    from dgl_amd import _lib

    fn = _lib.LIB.dgla_gat_attention_supported          # AttributeError on a library without the symbol
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    return fn


TABLE = (
    # every shape of the fp32 parity test (tests/test_gpu_gat_attention.py)
    [(F32, h, d, 1) for h, d in ((8, 8), (8, 32), (4, 4), (3, 8), (1, 64), (2, 128), (2, 4))] +
    # new fp32 head widths
    [(F32, h, d, 1) for h, d in ((1, 5), (2, 12), (8, 6), (1, 47), (2, 100), (64, 2), (3, 24), (16, 2), (1, 1), (1, 7),
                                 (1, 40), (1, 96), (8, 12), (4, 48))] +
    # 16-bit
    [(t, h, d, 1) for t in (F16, BF16) for h, d in ((8, 64), (2, 256), (8, 12), (8, 8), (8, 32), (2, 12), (1, 47), (64, 8))] +
    # rejections
    [(F32, 6, 121, 0), (F16, 6, 121, 0), (BF16, 6, 121, 0), (F32, 8, 64, 0), (F32, 3, 100, 0), (F32, 2, 47, 0),
     (F16, 16, 64, 0), (BF16, 4, 256, 0), (F32, 65, 1, 0), (F32, 0, 8, 0), (F32, 8, 0, 0), (F32, -1, 8, 0),
     (F64, 8, 8, 0), (F64, 1, 5, 0), (7, 8, 8, 0)])


@pytest.mark.parametrize("dtype,h,d,want", TABLE)
def test_table(dtype, h, d, want):
    assert _rule(dtype, h, d) == want, "the table itself disagrees with the rule"
    assert _fn()(dtype, h, d) == want


def test_the_function_is_the_rule_on_a_grid():
    fn = _fn()
    for dtype in (F32, F64, F16, BF16):
        for h in (1, 2, 3, 4, 6, 8, 16, 32, 64, 65):
            for d in list(range(1, 130)) + [192, 200, 256, 264, 512, 520, 1024, 1 << 40]:
                assert fn(dtype, h, d) == _rule(dtype, h, d), (dtype, h, d)


def test_today_s_fp32_set_is_kept():
    """fp32 with D a power of two >= 4: exactly H * D <= 256, as before."""
    fn = _fn()
    for lg in range(2, 10):
        for h in range(1, 70):
            assert fn(F32, h, 1 << lg) == int(h * (1 << lg) <= 256)


def test_declared_and_documented_in_the_header():
    with open(os.path.join(ROOT, "include", "dgl_amd.h")) as fh:
        text = fh.read()
    assert re.search(r"int\s+dgla_gat_attention_supported\s*\(\s*dgla_dtype\s+dtype\s*,\s*int64_t\s+heads\s*,\s*int64_t\s+dim\s*\)\s*;",
                     text)
    assert "H * LPH <= 64" in text and "mz" in text and "16-bit contract" in text


def test_python_side_uses_the_same_function():
    import torch

    from dgl_amd import _capi

    assert _capi.gat_attention_supported(torch.bfloat16, 8, 64) and _capi.gat_attention_supported(torch.float32, 1, 47)
    assert not _capi.gat_attention_supported(torch.float32, 8, 64) and not _capi.gat_attention_supported(torch.float64, 8, 8)
