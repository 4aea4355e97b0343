"""CPU tier: the seed kernel of a cotangent on the whole output blob (grad_kernels.hpp: k_adj_seed_all) of the built library uses no
scratch and spills no register -- read off the kernel descriptor the way tools/isa_lint.py does."""
import os
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_seed_all_kernel_no_scratch_no_spill():
    import isa_lint
    found = {}
    for co in isa_lint.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            tmp = f.name
        try:
            meta = isa_lint.metadata(tmp)
        finally:
            os.unlink(tmp)
        for sym, md in meta.items():
            if "k_adj_seed_all" in sym:
                found["k_adj_seed_all"] = md
    assert set(found) == {"k_adj_seed_all"}, list(found)
    md = found["k_adj_seed_all"]
    assert int(md.get("private_segment_fixed_size", 0)) == 0, md
    assert int(md.get("vgpr_spill_count", 0)) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, md
