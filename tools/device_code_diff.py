#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds (no GPU needed).

`python tools/device_code_diff.py <build dir A> <build dir B>` takes two directories of objects (build/csrc of two
checkouts, both built by dgl_amd/csrc/Makefile) and prints, for every unit present in either, "identical" or the
names of the kernels that differ.  A kernel is its instruction text and its .amdhsa_* descriptor block, as
tools/isa_audit.py's disassemble() prints them with the addresses and encodings left out; the __hip_cuid_* symbols
and the order in which kernels are emitted are ignored.  A plain text comparison: a host-side refactor must leave
every unit identical.  Exit status 1 when a unit differs."""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_audit import _LABEL, disassemble  # noqa: E402


def kernels(text, keep=lambda name: True):
    """{symbol: [instruction or directive text, ...]} of one disassembly."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _LABEL.match(line)
        if m:
            name = m.group(1)
            cur = out.setdefault(name, []) if keep(name) and not name.startswith("__hip_cuid_") else None
            continue
        body = line.split("//")[0].strip()
        if cur is not None and body:
            cur.append(body)
    return out


def device_code(obj):
    """{symbol: lines} of the code and the kernel descriptors of `obj` ({} when it bundles no gfx950 code)."""
    code = disassemble(obj)
    if code is None:
        return {}
    out = kernels(code)
    out.update(kernels(disassemble(obj, sections=(".rodata",)), keep=lambda name: name.endswith(".kd")))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a_dir, b_dir = sys.argv[1:]
    units = sorted({os.path.basename(p) for d in (a_dir, b_dir) for p in glob.glob(os.path.join(d, "*.o"))})
    differ = 0
    for unit in units:
        a, b = os.path.join(a_dir, unit), os.path.join(b_dir, unit)
        if not (os.path.exists(a) and os.path.exists(b)):
            print("%-24s only in %s" % (unit, a_dir if os.path.exists(a) else b_dir))
            differ += 1
            continue
        ka, kb = device_code(a), device_code(b)
        if not ka and not kb:
            continue  # host-only object
        bad = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
        if not bad:
            print("%-24s identical (%d kernels)" % (unit, sum(1 for k in ka if not k.endswith(".kd"))))
            continue
        differ += 1
        print("%-24s %d symbols differ" % (unit, len(bad)))
        for k in bad:
            print("    %s%s" % (k, "" if k in ka and k in kb else "  (only in %s)" % (a_dir if k in ka else b_dir)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
