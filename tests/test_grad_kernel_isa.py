"""CPU tier: the data-gradient kernels (grad_kernels.hpp: k_data_grad, k_adj_seed) of the built library use no scratch and
spill no register -- read off the kernel descriptors the way tools/isa_lint.py does."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="product library not built")
def test_grad_kernels_no_scratch_no_spill():
    import isa_lint
    found = {}
    for co in isa_lint.code_objects(LIB):
        import tempfile
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            tmp = f.name
        try:
            meta = isa_lint.metadata(tmp)
        finally:
            os.unlink(tmp)
        for sym, md in meta.items():
            for k in ("k_data_grad", "k_adj_seed"):
                if k in sym:
                    found[k] = md
    assert set(found) == {"k_data_grad", "k_adj_seed"}, list(found)
    for k, md in found.items():
        assert int(md.get("private_segment_fixed_size", 0)) == 0, (k, md)
        assert int(md.get("vgpr_spill_count", 0)) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, (k, md)
