"""What the held-dynamics test files share (test_hold_dynamics.py, test_hold_rhs.py, test_hold_factor.py): nx = 8, nu = 3, batch 130
(two full tiles and a tile of 2 lanes), family forced with ACADOS_AMD_WPI=0, seeded random_lqr_batch, outputs x u pi lam t iter status
under numpy.array_equal; both tiers: `hostsim` (kernel sources under g++, one lane at a time) and `gpu` (the product library).
A plain module like random_qp.py; each file binds its own seed (and horizon) to these helpers."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

TIERS = [pytest.param("hostsim", id="hostsim"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
NX, NU, B = 8, 3, 130
TILES = (B + 63) // 64
MID = 64 + 17            # an instance of the middle tile
FIELDS = ("x", "u", "pi", "lam", "t")
LIB = os.path.join(ROOT, "acados_amd", "csrc", "libacados_amd_qp.so")


@pytest.fixture
def clib(request, monkeypatch):
    monkeypatch.setenv("ACADOS_AMD_WPI", "0")   # one instance per lane whatever the batch size
    return request.getfixturevalue("hostsim_lib" if request.param == "hostsim" else "gpu_lib")


_BASE = {}


def base_data(N, seed, zero_entry=None):
    """the batch with the same A, B at every stage (computed once per horizon and seed, never changed: callers copy what they alter);
    zero_entry: (row, column) of A set to +0.0 in every instance"""
    if (N, seed, zero_entry) not in _BASE:
        from acados_amd.generators import random_lqr_batch
        d = random_lqr_batch(N=N, nx=NX, nu=NU, batch=B, seed=seed)
        if zero_entry is not None:
            d["A"][:, zero_entry[0], zero_entry[1]] = 0.0
        _BASE[N, seed, zero_entry] = d
    return _BASE[N, seed, zero_entry]


def make_batch(clib, data, N, a_stage=None, opts=None):
    """a_stage: {stage: A of the whole batch at that stage} on top of the base batch `data`"""
    from acados_amd import OcpQpGpuBatch
    from acados_amd.generators import fill_lqr_batch, lqr_dims
    gb = OcpQpGpuBatch(lqr_dims(N, NX, NU), B, _clib=clib)
    fill_lqr_batch(gb, data, N)
    for k, a in (a_stage or {}).items():
        gb.set("A", k, a)
    gb.opts_set("tol_stat", 1e-8)
    for f, v in (opts or {}).items():
        gb.opts_set(f, v)
    return gb


def outputs(gb, N):
    out = {"iter": gb.info("iter").copy(), "status": gb.info("status").copy()}
    for k in range(N + 1):
        for f in FIELDS:
            if (f == "pi" or f == "u") and k == N:
                continue
            out[f, k] = np.array(gb.get(f, k), copy=True)
    return out


_SOLVED = {}


def solved(clib, data, N, hold, a_stage=None, opts=None, key=None):
    """(batch, outputs) of one solve; runs named by `key` are computed once per library and base batch and shared between the tests"""
    ck = (id(clib), id(data), N, hold, key)
    if key is not None and ck in _SOLVED:
        return _SOLVED[ck]
    gb = make_batch(clib, data, N, a_stage, dict(opts or {}, hold_dynamics=hold))
    gb.solve()
    assert gb.kernel_name.startswith("1tpi-box<NX=8,NU=3"), gb.kernel_name
    res = (gb, outputs(gb, N))
    if key is not None:
        _SOLVED[ck] = res
    return res


def assert_same(a, b, skip=()):
    assert a.keys() == b.keys()
    keep = np.array([i not in skip for i in range(B)])
    for key in a:
        assert np.array_equal(a[key][keep], b[key][keep], equal_nan=True), key


@functools.lru_cache(maxsize=None)
def _code_objects():
    """per gfx950 code object of the built library: (metadata, static LDS bytes, demangled names, image)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not isa_lint.READELF:
        pytest.skip("llvm-readelf not found")
    out = []
    for co in isa_lint.code_objects(LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            meta = isa_lint.metadata(f.name)
            notes = subprocess.run([isa_lint.READELF, "--notes", f.name], capture_output=True, text=True).stdout
        # static LDS per kernel: .group_segment_fixed_size precedes .name / .symbol inside a kernel's metadata entry
        lds, cur = {}, None
        for ln in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(group_segment_fixed_size|symbol):\s*(\S+)", ln)
            if m and m.group(1) == "group_segment_fixed_size":
                cur = int(m.group(2))
            elif m and cur is not None:
                lds[m.group(2).strip("'\"").replace(".kd", "")] = cur
                cur = None
        out.append((meta, lds, isa_lint.demangle(list(meta)), co))
    return out


def built_kernel_facts(demangled_name, instructions=True):
    """(kernel descriptor metadata, static LDS bytes, instructions) of gqp::<demangled_name> in the built library, read the way
    tests/test_box_sweep_isa.py does; None where the library has no such kernel.  The instructions take a disassembly of the
    kernel's code object: None where they are not asked for or llvm-objdump is missing"""
    objs = _code_objects()
    import isa_lint
    found = None
    for meta, lds, names, co in objs:
        for sym, md in meta.items():
            if "gqp::" + demangled_name + "(" in names[sym]:
                ins = None
                if instructions and isa_lint.OBJDUMP:
                    with tempfile.NamedTemporaryFile(suffix=".co") as f:
                        f.write(co)
                        f.flush()
                        ins = isa_lint.kernels(subprocess.run([isa_lint.OBJDUMP, "-d", f.name], capture_output=True, text=True).stdout).get(sym, [])
                found = (md, lds.get(sym), ins)
    return found


def assert_no_scratch(md):
    """no private segment, no spilled register in the kernel descriptor"""
    assert int(md.get("private_segment_fixed_size", 0)) == 0, md
    assert int(md.get("vgpr_spill_count", 0)) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, md
