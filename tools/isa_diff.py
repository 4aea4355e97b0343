#!/usr/bin/env python3
"""Device code of two builds of the library, kernel by kernel: is it the same?

    python tools/isa_diff.py OLD.so NEW.so

Disassembles the gfx950 code objects of both libraries (the LLVM tools are found the way tools/isa_lint.py finds them) and compares,
for every code symbol, the instruction stream and, for every kernel, the resource lines of its descriptor as the metadata note
states them: VGPRs, AGPRs, SGPRs, spilled registers, scratch, LDS, kernarg size, workgroup size.  Prints the counts of kernels and
instructions on both sides and the kernels that differ, are new, or are gone.  It compares only -- it looks for nothing in
particular.  What a host-only change is checked with: the two libraries must come out equal.

Exit code 1: a kernel both libraries have differs; 2: only the sets of kernels differ; 3: the LLVM tools were not found; 0: equal."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_lint

RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def parse_resources(notes):
    """{kernel symbol: {resource: value}} from the text of `llvm-readelf --notes`: under `amdhsa.kernels:` every kernel is one list
    item, opened by `  - ` at indent 2 with its keys (alphabetical: .agpr_count first, .name and .symbol in the middle) at indent 4;
    deeper lines belong to its .args.  A record is closed where the next item opens or the list ends, never at a key"""
    out, vals, inside = {}, None, False

    def close():
        if vals and vals.get("symbol"):
            out[vals["symbol"].replace(".kd", "")] = {k: vals.get(k, "?") for k in RESOURCES}

    for ln in notes.splitlines():
        if ln.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and ln[:1] not in (" ", ""):      # the next top-level key: the list is over
            close()
            vals, inside = None, False
        if not inside:
            continue
        if ln.startswith("  - "):
            close()
            vals = {}
        m = re.match(r"^(?:  - |    )\.(\w+):\s*(.*)$", ln)
        if m and vals is not None and (m.group(1) in RESOURCES or m.group(1) == "symbol"):
            vals[m.group(1)] = m.group(2).strip().strip("'\"")
    close()
    return out


def resources(path):
    return parse_resources(subprocess.run([isa_lint.READELF, "--notes", path], capture_output=True, text=True).stdout)


def library(path):
    """({symbol: [instructions]}, {kernel symbol: resources}) over every gfx950 code object of the library"""
    code, res = {}, {}
    for co in isa_lint.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            tmp = f.name
        try:
            dis = subprocess.run([isa_lint.OBJDUMP, "-d", tmp], capture_output=True, text=True).stdout
            res.update(resources(tmp))
        finally:
            os.unlink(tmp)
        code.update(isa_lint.kernels(dis))
    return code, res


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 3
    if not isa_lint.OBJDUMP or not isa_lint.READELF:
        print("isa_diff: llvm-objdump / llvm-readelf not found (ROCM_PATH, beside HIPCC, /opt/rocm, PATH)")
        return 3
    (code_a, res_a), (code_b, res_b) = library(sys.argv[1]), library(sys.argv[2])
    for tag, path, code, res in (("old", sys.argv[1], code_a, res_a), ("new", sys.argv[2], code_b, res_b)):
        print(f"{tag}: {path}: {len(code)} code symbols, {len(res)} kernels with a descriptor, {sum(len(v) for v in code.values())} instructions")
    names = isa_lint.demangle(sorted(set(code_a) | set(code_b) | set(res_a) | set(res_b)))
    short = lambda s: names.get(s, s).split("(")[0]
    gone = sorted(set(code_a) - set(code_b))
    new = sorted(set(code_b) - set(code_a))
    differ = []
    for sym in sorted(set(code_a) & set(code_b)):
        a, b = code_a[sym], code_b[sym]
        what = []
        if a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            what.append(f"instructions {len(a)} -> {len(b)}, {sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))} changed, first at {first}")
        ra, rb = res_a.get(sym), res_b.get(sym)
        if ra != rb:
            what.append("resources " + ", ".join(f"{k} {(ra or {}).get(k)} -> {(rb or {}).get(k)}" for k in RESOURCES if (ra or {}).get(k) != (rb or {}).get(k)))
        if what:
            differ.append(f"  {short(sym)}: " + "; ".join(what))
    for title, rows in (("kernels that differ", differ), ("new kernels", ["  " + short(s) for s in new]), ("kernels that are gone", ["  " + short(s) for s in gone])):
        print(f"{title}: {len(rows)}")
        for r in rows:
            print(r)
    if not differ and not new and not gone:
        print("device code identical: every instruction stream and every resource line")
    return 1 if differ else 2 if (new or gone) else 0


if __name__ == "__main__":
    sys.exit(main())
