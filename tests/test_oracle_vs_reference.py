"""Pins the oracle (our plain-C restatement) to the REFERENCE ITSELF: oracle/_ref/libdglref.so
is dgl's own src/array/cpu/{spmm,sddmm}.cc + src/bcast.cc compiled where they lie
(oracle/Makefile).  Every case of the exhaustive sweep must agree BIT FOR BIT — values,
arg_u / arg_e, broadcast offset tables.  What the reference build returned is recorded in
tests/golden/reference_digests.npz (tests/golden/make_golden_digests.py), so the sweeps run
without that build; where it is present they also run it and demand it still matches the record.
"""
import json
import os

import numpy as np
import pytest

import oracle
from oracle import ref
from tests.golden_cases import BCAST_CASES, all_cases, c2_shaped_input, run_case
from tests.golden_store import digest, load_digests

needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libdglref.so not built")


def test_full_sweep_bit_exact():
    recorded = load_digests("oracle_sweep")
    live = ref.available()
    bad = []
    cases = all_cases(full=True)
    assert len(cases) > 2000 and len(recorded) == len(cases)
    for c in cases:
        want = recorded[c["name"]]
        if live:
            serial = c["kind"] == "spmm_coo" and c["reduce"] == "sum"
            if serial:
                # SpMMSumCoo adds with `omp atomic` (spmm.h:196-205): its order is only defined
                # on one thread, which is the order the oracle restates
                ref.set_num_threads(1)
            if digest(run_case(ref, c)) != want:
                bad.append((c["name"], "reference build differs from the record"))
            if serial:
                ref.set_num_threads(os.cpu_count() or 1)
        if digest(run_case(oracle, c)) != want:
            bad.append(c["name"])
    assert not bad, bad[:20]


@pytest.mark.parametrize("op,ls,rs", BCAST_CASES)
def test_bcast_tables_match_reference(op, ls, rs):
    """oracle.BcastOff restates CalcBcastOff (src/bcast.cc:36-90)."""
    want = json.loads(load_digests("bcast")["%s|%s|%s" % (op, ls, rs)])
    if ref.available():
        live = ref.calc_bcast_off(op, ls, rs)
        assert {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in live.items()} == want
    got = oracle.BcastOff(op, ls, rs)
    assert got.use_bcast == want["use_bcast"]
    for k in ("lhs_len", "rhs_len", "out_len", "reduce_size"):
        assert getattr(got, k) == want[k], k
    if want["use_bcast"]:
        np.testing.assert_array_equal(got.lhs_offset, want["lhs_offset"])
        np.testing.assert_array_equal(got.rhs_offset, want["rhs_offset"])


@needs_ref
def test_reference_errors_surface():
    # SWITCH_OP default branch: LOG(FATAL) "Unsupported SpMM binary operator" (spmm_binary_ops.h)
    indptr = np.array([0, 1], np.int32)
    idx = np.array([0], np.int32)
    x = np.ones((1, 2), np.float32)
    with pytest.raises(RuntimeError, match="[Uu]nsupported"):
        ref.spmm_csr("pow", "sum", indptr, idx, None, x, x)


def test_c2_shaped_sum_bit_exact():
    """A 1/64-scale ogbn-products-shaped CSR (heavy-tailed rows) through both, copy_u+sum."""
    ip, ix, x = c2_shaped_input()
    want = load_digests("c2_shaped_sum")["out"]
    if ref.available():
        assert digest(ref.spmm_csr("copy_lhs", "sum", ip, ix, None, x, None)[0]) == want
    assert digest(oracle.spmm_csr("copy_lhs", "sum", ip, ix, None, x, None)[0]) == want
    assert digest(oracle.copy_u_sum_csr(ip, ix, x)) == want
