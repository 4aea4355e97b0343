#!/usr/bin/env python3
"""Development aid: how the vector-memory loads of a kernel's stage loop leave the wave, read off the assembly hipcc
writes (`hipcc -O3 --offload-arch=gfx950 --offload-device-only -S`) or off a built library.  Per kernel one line:
registers, scratch, LDS, and the sequence of load bursts of the LONGEST loop body -- `L<n>` = n buffer / global loads
issued back to back (arithmetic between them does not end a burst), `w<n>` = an `s_waitcnt vmcnt(n)` -- e.g.
`L173 w18 .. L16 .. w0`: 173 loads in flight before the first wait; `{ .. }` encloses what a forward branch can skip.

    python tools/wait_pattern.py FILE.s [substring of the demangled kernel name ...]
    python tools/wait_pattern.py acados_amd/csrc/libacados_amd_qp.so kb_forward kb_backrhs
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_lint

LOAD = re.compile(r"^(buffer_load|global_load|flat_load|scratch_load)")
STORE = re.compile(r"^(buffer_store|global_store|flat_store|scratch_store)")
VMCNT = re.compile(r"^s_waitcnt\b.*vmcnt\((\d+)\)")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\S+)")


def asm_kernels(text):
    """{symbol: [(label or None, instruction)]} of a hipcc -S listing"""
    out, cur = {}, None
    for ln in text.splitlines():
        s = ln.split(";")[0].rstrip()
        m = re.match(r"^(\w+):\s*$", s)
        if m and not s.startswith(".L"):
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        m = re.match(r"^(\.L\w+):\s*$", s)
        if m:
            out[cur].append((m.group(1), None))
        elif s.startswith("\t") and not s.strip().startswith("."):
            out[cur].append((None, s.strip()))
        elif s.strip().startswith(".end_amdhsa_kernel") or s.strip().startswith(".section"):
            cur = None
    return {k: v for k, v in out.items() if any(i for _, i in v)}


def objdump_kernels(lib):
    """the same shape from a built library: labels are the `<L..>` targets of llvm-objdump"""
    out = {}
    for co in isa_lint.code_objects(lib):
        import tempfile
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            tmp = f.name
        try:
            dis = subprocess.run([isa_lint.OBJDUMP, "-d", "--symbolize-operands", tmp], capture_output=True, text=True).stdout
        finally:
            os.unlink(tmp)
        cur = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
            if m and not re.match(r"^L\d+$", m.group(1)):
                cur = m.group(1)
                out[cur] = []
                continue
            if cur is None:
                continue
            m = re.match(r"^[0-9a-f]+ <(L\d+)>:$", ln.strip())
            if m:
                out[cur].append((m.group(1), None))
            elif ln.startswith("\t"):
                out[cur].append((None, ln.strip().split("//")[0].strip()))
    return out


def longest_loop(items):
    """the stage loop of a sweep: of the backward branches, the shortest span that holds most of the loads any span holds
    (block layout puts some forward edges behind their targets: a span that merely encloses the loop is not taken for it)"""
    pos, cands = {}, []
    for i, (lab, ins) in enumerate(items):
        if lab:
            pos[lab] = i
        elif ins:
            m = BRANCH.match(ins)
            if m and m.group(1) in pos:
                lo = pos[m.group(1)]
                cands.append((sum(1 for _, t in items[lo:i + 1] if t and LOAD.match(t)), i - lo, lo, i))
    if not cands:
        return []
    most = max(c[0] for c in cands)
    _, _, lo, hi = min((c for c in cands if c[0] >= 0.6 * most), key=lambda c: c[1])
    return items[lo:hi + 1]


def pattern(body):
    out, run, n_ld, n_st, n_ds, n_ins = [], 0, 0, 0, 0, 0
    skips = set()       # targets of forward branches inside the body: `{ .. }` = a stretch a wave-uniform branch can skip
    for k, (lab, ins) in enumerate(body):
        if lab:
            if lab in skips:
                if run:
                    out.append(f"L{run}")
                    run = 0
                out.append("}")
            continue
        n_ins += 1
        m = BRANCH.match(ins)
        if m and any(l == m.group(1) for l, _ in body[k + 1:]):
            if run:
                out.append(f"L{run}")
                run = 0
            out.append("{")
            skips.add(m.group(1))
        if LOAD.match(ins):
            run += 1
            n_ld += 1
        elif STORE.match(ins):
            n_st += 1
        elif ins.startswith("ds_"):
            n_ds += 1
        m = VMCNT.match(ins)
        if m:
            if run:
                out.append(f"L{run}")
                run = 0
            out.append(f"w{m.group(1)}")
    if run:
        out.append(f"L{run}")
    return " ".join(out), n_ld, n_st, n_ds, n_ins


def main():
    path, subs = sys.argv[1], sys.argv[2:]
    ks = objdump_kernels(path) if path.endswith(".so") else asm_kernels(open(path).read())
    names = isa_lint.demangle(list(ks))
    for sym, items in ks.items():
        dn = names.get(sym, sym).split("(")[0]
        if subs and not any(s in dn for s in subs):
            continue
        pat, n_ld, n_st, n_ds, n_ins = pattern(longest_loop(items))
        print(f"{dn}\n    stage loop: {n_ins} instructions, {n_ld} loads, {n_st} stores, {n_ds} LDS ops\n    {pat}")


if __name__ == "__main__":
    main()
