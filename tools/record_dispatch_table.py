"""Records tests/dispatch_table.json: what every row of tests/test_dispatch_table.py leaves on THIS tree (kernel name, w16_tiles
scalar, refusal), under host simulation.  Run it on the commit whose dispatch is the reference -- a change of the family choice
that is meant to leave the table alone is then checked against that file, not against itself:

    python tools/record_dispatch_table.py [--tree PATH [--commit NAME]]

--tree: another checkout of this repository (the parent commit's) whose sources are built and evaluated; the ROWS are this tree's."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--commit", help="name of the commit of --tree where it is an export without history")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    spec = importlib.util.spec_from_file_location("rows", os.path.join(ROOT, "tests", "test_dispatch_table.py"))
    from hostsim.build import build
    from acados_amd import _lib
    clib = _lib.bind(ctypes.CDLL(build()))
    rows = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rows)
    commit = a.commit or subprocess.check_output(["git", "-C", tree, "rev-parse", "--short", "HEAD"]).decode().strip()
    out = {"recorded_from_commit": commit, "tier": "hostsim", "rows": {}}
    for r in rows.ROWS:
        key = rows.row_key(r) + "".join(f" {k}={v}" for k, v in sorted(r["env"].items()))
        out["rows"][key] = rows.evaluate(clib, r, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
    with open(os.path.join(ROOT, "tests", "dispatch_table.json"), "w") as f:
        rows_out = out.pop("rows")   # one row per line
        f.write(json.dumps(out)[:-1] + ', "rows": {\n' + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rows_out.items()) + "\n}}\n")
    print(f"{len(rows_out)} rows recorded from {commit}")


if __name__ == "__main__":
    main()
