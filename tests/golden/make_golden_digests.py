#!/usr/bin/env python
"""Generates tests/golden/reference_digests.npz from the REFERENCE's own CPU kernels.

Needs the reference build (oracle/_ref/libdglref.so, made by oracle/Makefile where a reference
checkout is present):

    make -C oracle ref && python tests/golden/make_golden_digests.py

For every case of the exhaustive sweeps that pin the oracle to the reference it records the
digest (tests/golden_store.digest) of the outputs the reference returned, run exactly
as the sweeps run it: g-SpMM / g-SDDMM / edge softmax (SpMMSumCoo on one thread, the rest on
all cores), segment reduce (one thread), heterograph g-SpMM and COO -> CSR (one and four
threads), the 1/64-scale C2 copy_u + sum, plus the CalcBcastOff tables themselves.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref  # noqa: E402
from tests import coo_cases, golden_cases, hetero_cases, segment_cases  # noqa: E402
from tests.golden_store import DIGESTS, digest, save_digests  # noqa: E402


def main():
    assert ref.available(), "build oracle/_ref first: make -C oracle ref"
    cores = os.cpu_count() or 1
    rec = {}
    sweep = {}
    for c in golden_cases.all_cases(full=True):
        serial = c["kind"] == "spmm_coo" and c["reduce"] == "sum"
        ref.set_num_threads(1 if serial else cores)
        sweep[c["name"]] = digest(golden_cases.run_case(ref, c))
    rec["oracle_sweep"] = sweep
    bc = {}
    for op, ls, rs in golden_cases.BCAST_CASES:
        w = ref.calc_bcast_off(op, ls, rs)
        bc["%s|%s|%s" % (op, ls, rs)] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in w.items()}
    rec["bcast"] = bc
    ref.set_num_threads(1)
    rec["segment_sweep"] = {c["name"]: digest(segment_cases.run_case(ref, c))
                            for c in segment_cases.all_cases(full=True)}
    for threads in (1, 4):
        ref.set_num_threads(threads)
        rec["hetero_sweep_threads%d" % threads] = {c["name"]: digest(hetero_cases.run_case(ref, c))
                                                   for c in hetero_cases.all_cases(full=True)}
        rec["coo2csr_threads%d" % threads] = {
            c["name"]: digest(dict(zip(("indptr", "indices", "eids"),
                                        ref.coo_to_csr(c["row"], c["col"], c["eids"], c["num_rows"], c["num_cols"]))))
            for c in coo_cases.all_cases()}
    ref.set_num_threads(cores)
    ip, ix, x = golden_cases.c2_shaped_input()
    rec["c2_shaped_sum"] = {"out": digest(ref.spmm_csr("copy_lhs", "sum", ip, ix, None, x, None)[0])}
    save_digests(rec)
    print("wrote %s: %s, %.1f KiB" % (DIGESTS, {k: len(v) for k, v in rec.items()}, os.path.getsize(DIGESTS) / 1024))


if __name__ == "__main__":
    main()
