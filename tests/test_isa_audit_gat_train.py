"""Static invariants of the built training-form GAT attention kernels (build/csrc/gat_attention_train.o,
tools/isa_audit.py) — runs without a GPU, in the style of tests/test_isa_audit_gat.py.

The kernels keep `float[V]` accumulators, `float[U][V]` staging and the four Philox words per lane: an index into any
of them that is not a compile-time constant sends the array to scratch memory, and a pointer that loses its address
space turns the gathers into flat loads.  Neither changes a result bit, so only the disassembly shows it."""
import os

import pytest

from tools import isa_audit

OBJ = os.path.join(isa_audit.ROOT, "build", "csrc", "gat_attention_train.o")
# Itanium-mangled element types as they appear in the kernel symbols
TYPES = {"fp32": "If", "fp16": "IDF16_", "bf16": "INS_6bf16_tE"}
TRAIN = {"forward": "gat_fwd_train_kernel", "B1": "gat_bwd_dst_train_kernel", "B2": "gat_bwd_src_train_kernel"}
WEIGHTS = "gat_weights_kernel"


@pytest.fixture(scope="module")
def stats():
    if not os.path.exists(OBJ) or not os.path.exists(isa_audit.OBJDUMP):
        pytest.skip("no built objects / llvm-objdump here (run __graft_entry__.build())")
    text = isa_audit.disassemble(OBJ)
    assert text, "no gfx950 code object in gat_attention_train.o"
    return isa_audit.audit_text(text)


def test_forward_b1_b2_and_weights_exist_for_all_three_element_types(stats):
    for what, name in TRAIN.items():
        for tname, tag in TYPES.items():
            ks = [k for k in stats if name + tag in k]
            # widths V = 1, 2, 4 (and 8 for 16-bit) x five row widths x two id types
            want = (3 if tname == "fp32" else 4) * 5 * 2
            assert len(ks) == want, "%s %s: %d kernels, expected %d" % (what, tname, len(ks), want)
    # V = 8 (16-byte slabs of 16-bit elements) exists for fp16 / bf16 only
    assert not [k for k in stats if "_train_kernelIfLi8E" in k]
    for tname, tag in TYPES.items():
        ks = [k for k in stats if WEIGHTS + tag in k]
        assert len(ks) == 2, "weights %s: %d kernels, expected one per id type" % (tname, len(ks))
    # the inference-form kernels live in gat_attention.o alone
    assert not [k for k in stats if "_wide_kernelI" in k or "gat_fwd_kernelI" in k]


def test_no_flat_and_no_scratch_instruction_in_any_kernel(stats):
    assert len(stats) > 330
    bad = {k: (c["flat"], c["scratch"]) for k, c in stats.items() if c["flat"] or c["scratch"]}
    assert not bad, list(bad.items())[:5]


def test_every_gather_kernel_loads_through_global_instructions(stats):
    for name in list(TRAIN.values()) + [WEIGHTS]:
        for k, c in stats.items():
            if name in k:
                assert c["global_load"] > 0, k
