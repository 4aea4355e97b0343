"""CPU tier: the one-instance-per-lane box sweeps (ipm_kernels_box.hpp) of the built library, read off the kernel descriptors and
the disassembly the way tools/isa_lint.py does.

The C2 instantiations kb_forward<8, 3, false, *> and kb_backrhs<8, 3, false> hold a whole stage in registers: they must stay
out of scratch and spill nothing (the affine sweep used to spill scalar registers to lanes of a vector register around its stage
loop), and four single-wave blocks per CU must keep fitting beside each other and beside kb_factor's 32 KB of LDS.  No kb_*
kernel uses LDS-DMA (tests/test_isa_lint.py pins that set to the ky_ / kt_ families), and no other kb_* instantiation may carry
more scratch than it did before the affine sweep stopped loading the factor block it does not use (PARENT_SCRATCH: bytes per
lane, from the build of the preceding commit)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so")

C2 = ("kb_forward<8, 3, false, false>", "kb_forward<8, 3, false, true>", "kb_backrhs<8, 3, false>")

# .private_segment_fixed_size of every kb_* kernel of the library before this change
PARENT_SCRATCH = {
    "kb_backrhs<12, 3, false>": 0, "kb_backrhs<12, 3, true>": 0, "kb_backrhs<24, 3, false>": 6432, "kb_backrhs<24, 3, true>": 6432,
    "kb_backrhs<24, 6, false>": 7152, "kb_backrhs<24, 6, true>": 7152, "kb_backrhs<4, 1, false>": 0, "kb_backrhs<4, 1, true>": 0,
    "kb_backrhs<4, 4, false>": 0, "kb_backrhs<4, 4, true>": 0, "kb_backrhs<8, 15, false>": 2960, "kb_backrhs<8, 15, true>": 2960,
    "kb_backrhs<8, 3, false>": 0, "kb_backrhs<8, 3, true>": 0,
    "kb_factor<12, 3, false>": 2148, "kb_factor<12, 3, true>": 3248, "kb_factor<24, 3, false>": 13248, "kb_factor<24, 3, true>": 14016,
    "kb_factor<24, 6, false>": 14688, "kb_factor<24, 6, true>": 15456, "kb_factor<4, 1, false>": 0, "kb_factor<4, 1, true>": 0,
    "kb_factor<4, 4, false>": 0, "kb_factor<4, 4, true>": 0, "kb_factor<8, 15, false>": 5520, "kb_factor<8, 15, true>": 5776,
    "kb_factor<8, 3, false>": 0, "kb_factor<8, 3, true>": 800,
    "kb_finalize<12, 3>": 0, "kb_finalize<24, 3>": 224, "kb_finalize<24, 6>": 256, "kb_finalize<4, 1>": 0, "kb_finalize<4, 4>": 0,
    "kb_finalize<8, 15>": 192, "kb_finalize<8, 3>": 0,
    "kb_forward<12, 3, false, false>": 0, "kb_forward<12, 3, false, true>": 1188, "kb_forward<12, 3, true, false>": 964,
    "kb_forward<12, 3, true, true>": 1964, "kb_forward<24, 3, false, false>": 9664, "kb_forward<24, 3, false, true>": 9824,
    "kb_forward<24, 3, true, false>": 11968, "kb_forward<24, 3, true, true>": 11968, "kb_forward<24, 6, false, false>": 11184,
    "kb_forward<24, 6, false, true>": 11328, "kb_forward<24, 6, true, false>": 13488, "kb_forward<24, 6, true, true>": 13488,
    "kb_forward<4, 1, false, false>": 0, "kb_forward<4, 1, false, true>": 0, "kb_forward<4, 1, true, false>": 0,
    "kb_forward<4, 1, true, true>": 0, "kb_forward<4, 4, false, false>": 0, "kb_forward<4, 4, false, true>": 0,
    "kb_forward<4, 4, true, false>": 0, "kb_forward<4, 4, true, true>": 0, "kb_forward<8, 15, false, false>": 5936,
    "kb_forward<8, 15, false, true>": 5936, "kb_forward<8, 15, true, false>": 6704, "kb_forward<8, 15, true, true>": 6704,
    "kb_forward<8, 3, false, false>": 0, "kb_forward<8, 3, false, true>": 0, "kb_forward<8, 3, true, false>": 0,
    "kb_forward<8, 3, true, true>": 332,
}


def _kb_kernels():
    """{`kb_name<args>`: (descriptor fields, instruction lines)} of every kb_* kernel of the library"""
    import isa_lint
    out = {}
    for co in isa_lint.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            tmp = f.name
        try:
            meta = isa_lint.metadata(tmp)
            notes = subprocess.run([isa_lint.READELF, "--notes", tmp], capture_output=True, text=True).stdout
            dis = isa_lint.kernels(subprocess.run([isa_lint.OBJDUMP, "-d", tmp], capture_output=True, text=True).stdout)
        finally:
            os.unlink(tmp)
        # static LDS per kernel: .group_segment_fixed_size precedes .name / .symbol inside a kernel's metadata entry
        lds, cur = {}, None
        for ln in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(group_segment_fixed_size|symbol):\s*(\S+)", ln)
            if m and m.group(1) == "group_segment_fixed_size":
                cur = int(m.group(2))
            elif m and cur is not None:
                lds[m.group(2).strip("'\"").replace(".kd", "")] = cur
                cur = None
        names = isa_lint.demangle(list(meta))
        for sym, md in meta.items():
            m = re.search(r"gqp::(kb_\w+<[^>]*>)", names[sym].split("(")[0])
            if m:
                out[m.group(1)] = (dict(md, lds=lds.get(sym)), dis.get(sym, []))
    return out


@pytest.fixture(scope="module")
def kb():
    import isa_lint
    if not isa_lint.OBJDUMP or not isa_lint.READELF:
        pytest.skip("llvm-objdump / llvm-readelf not found")
    ks = _kb_kernels()
    assert set(C2) <= set(ks), sorted(ks)
    return ks


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
@pytest.mark.parametrize("name", C2)
def test_c2_sweeps_stay_in_registers_and_fit_four_per_cu(kb, name):
    md, ins = kb[name]
    assert ins, name
    assert int(md.get("private_segment_fixed_size", 0)) == 0, (name, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, (name, md)
    assert md["lds"] is not None and md["lds"] <= 40960, (name, md)
    assert not any(t.startswith(("scratch_load", "scratch_store")) for t in ins), name


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_no_lds_dma_in_the_box_sweeps(kb):
    for name, (md, ins) in kb.items():
        dma = [t for t in ins if t.startswith("global_load_lds") or (t.startswith("buffer_load") and re.search(r"\blds\b", t))]
        assert not dma, (name, dma[:3])


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_no_box_sweep_gained_scratch(kb):
    assert set(kb) == set(PARENT_SCRATCH), sorted(set(kb) ^ set(PARENT_SCRATCH))
    worse = {n: (int(md.get("private_segment_fixed_size", 0)), PARENT_SCRATCH[n]) for n, (md, _) in kb.items()
             if int(md.get("private_segment_fixed_size", 0)) > PARENT_SCRATCH[n]}
    assert not worse, worse
