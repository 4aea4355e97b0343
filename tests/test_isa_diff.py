"""CPU tier: the descriptor half of tools/isa_diff.py.  In the metadata note the keys of a kernel stand in alphabetical order, so
.agpr_count, .group_segment_fixed_size, .kernarg_segment_size and .max_flat_workgroup_size come BEFORE the kernel's .name and .symbol:
a parser that opens a record at .name gives them to the kernel in front.  Two kernels with different LDS, kernarg and workgroup
sizes must come out under their own names, the last one complete."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = """  - .agpr_count:     {agpr}
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
      - .offset:         8
        .size:           4
        .value_kind:     hidden_block_count_x
    .group_segment_fixed_size: {lds}
    .kernarg_segment_align: 8
    .kernarg_segment_size: {kernarg}
    .language:       OpenCL C
    .language_version:
      - 2
      - 0
    .max_flat_workgroup_size: {wg}
    .name:           {name}
    .private_segment_fixed_size: {scratch}
    .sgpr_count:     {sgpr}
    .sgpr_spill_count: 0
    .symbol:         {name}.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     {vgpr}
    .vgpr_spill_count: 0
    .wavefront_size: 64
"""
NOTE = ("Displaying notes found in: .note\n  Owner                Data size \tDescription\n"
        "  AMDGPU               0x00000400\tNT_AMDGPU_METADATA (AMDGPU Metadata)\n    AMDGPU Metadata:\n        ---\namdhsa.kernels:\n"
        "{kernels}amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n")
ONE = dict(name="k_one", agpr=0, lds=512, kernarg=12, wg=1024, scratch=0, sgpr=10, vgpr=4)
TWO = dict(name="k_two", agpr=8, lds=2048, kernarg=24, wg=128, scratch=16, sgpr=20, vgpr=40)
THREE = dict(name="k_three", agpr=0, lds=0, kernarg=8, wg=256, scratch=0, sgpr=6, vgpr=2)


def _note(*kernels):
    return NOTE.format(kernels="".join(KERNEL.format(**k) for k in kernels))


def _expect(k):
    return {"vgpr_count": str(k["vgpr"]), "agpr_count": str(k["agpr"]), "sgpr_count": str(k["sgpr"]), "vgpr_spill_count": "0",
            "sgpr_spill_count": "0", "private_segment_fixed_size": str(k["scratch"]), "group_segment_fixed_size": str(k["lds"]),
            "kernarg_segment_size": str(k["kernarg"]), "max_flat_workgroup_size": str(k["wg"]), "wavefront_size": "64"}


def test_every_kernel_gets_its_own_resource_lines():
    import isa_diff
    got = isa_diff.parse_resources(_note(ONE, TWO, THREE))
    assert got == {k["name"]: _expect(k) for k in (ONE, TWO, THREE)}
    # a change of the middle kernel's LDS shows under that kernel and nowhere else
    after = isa_diff.parse_resources(_note(ONE, dict(TWO, lds=4096), THREE))
    assert [k for k in got if got[k] != after[k]] == ["k_two"] and after["k_two"]["group_segment_fixed_size"] == "4096"


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so")), reason="product library not built")
def test_product_library_descriptors_are_complete():
    """every kernel of the built library with all ten lines, and a kernel whose sizes the sources fix under its own name: the
    wave-per-instance kernels are launched as ONE wave (workgroup size 64, __launch_bounds__), k_scatter is not"""
    import isa_diff
    import isa_lint
    if not isa_lint.OBJDUMP or not isa_lint.READELF:
        pytest.skip("llvm-objdump / llvm-readelf not found")
    code, res = isa_diff.library(os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so"))
    assert len(res) >= 300 and set(res) <= set(code)
    assert all("?" not in r.values() for r in res.values())
    names = isa_lint.demangle(sorted(res))
    wg = {names[s].split("(")[0]: r["max_flat_workgroup_size"] for s, r in res.items()}
    assert wg["void gqp::kw_init<false>"] == "64" and wg["gqp::k_scatter"] == "1024", (wg["void gqp::kw_init<false>"], wg["gqp::k_scatter"])
