#!/usr/bin/env python3
"""Golden file of the getblocks tests from the reference's own addctginfo + clustermumsbydiagonal (reveal/transform.py:184-202, 562-600) -- TEST
INFRASTRUCTURE, build container only.

The reference is Python 2.  This script converts reveal/transform.py IN MEMORY with lib2to3 (nothing of it is written to the repository), pulls the
two functions out of the converted syntax tree and executes THEM, with update_progress stubbed.  They run on the MUM lists of the CPU oracle
(tests/blocks_cases.py oracle_mums: oracle_ctypes.getmums(.., rc=, nT=)) and on the abstract lists of tests/blocks_cases.py, the way transform()
calls them (transform.py:256-291): cluster=False takes the list addctginfo leaves.  Two outcomes are written as the library defines them, not as the
reference behaves: an empty list gives [] (the reference's forward leg raises IndexError on mums[0]), and the reference's `assert dist >= 0` is
recorded as "error".

    python tools/gen_blocks_golden.py      # rewrites tests/golden/blocks.json
"""
import ast
import json
import logging
import os
import sys
from lib2to3 import refactor

REF = "/root/reference/reveal"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blocks_cases as C                      # noqa: E402

LONG = 40      # block lists above this length are kept as count + digest


def load():
    tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    path = os.path.join(REF, "transform.py")
    src = open(path).read()
    if not src.endswith("\n"):
        src += "\n"
    tree = ast.parse(str(tool.refactor_string(src, path)))
    names = {"addctginfo", "clustermumsbydiagonal"}
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == names
    env = {"logging": logging, "update_progress": lambda *a, **k: None}
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), env)
    return env["addctginfo"], env["clustermumsbydiagonal"]


def reference_blocks(fns, mums, ranges, rc, cluster, maxdist, minclustsize):
    addctginfo, clustermumsbydiagonal = fns
    if not mums:
        return []
    mums = addctginfo([tuple(m) for m in mums], [tuple(r) for r in ranges])
    if not cluster:
        return [(m[1][0], m[1][0] + m[0], m[1][1], m[1][1] + m[0], m[2], m[0], m[3], m[4]) for m in mums]
    try:
        return clustermumsbydiagonal(mums, maxdist=maxdist, minclustsize=minclustsize, rcmums=bool(rc))
    except AssertionError:
        return "error"


def record(blocks, **meta):
    rec = dict(meta)
    if blocks == "error":
        rec["error"] = True
    elif len(blocks) > LONG:
        rec.update(count=len(blocks), sha256=C.digest(blocks), largest_score=max(b[5] for b in blocks))
    else:
        rec["blocks"] = [list(map(int, b)) for b in blocks]
    return rec


def main():
    fns = load()
    out = {"fixtures": {}, "multi": {}, "abstract": {}}
    for name in C.FIXTURES:
        for rc in (0, 1):
            lists = {}
            for vname, v in C.VARIANTS.items():
                p = C.params(**v)
                if p["minlength"] not in lists:
                    lists[p["minlength"]] = C.oracle_mums(C.fixture_inputs(name), p["minlength"], rc)
                mums, ranges = lists[p["minlength"]]
                assert C.keys_unique(mums, rc)
                b = reference_blocks(fns, mums, ranges, rc, p["cluster"], p["maxdist"], p["minclustsize"])
                out["fixtures"]["%s|rc%d|%s" % (name, rc, vname)] = record(b, mums=len(mums))
    for rc in (0, 1):
        mums, ranges = C.oracle_mums(C.multi_inputs(), C.MULTI["minlength"], rc)
        assert C.keys_unique(mums, rc)
        b = reference_blocks(fns, mums, ranges, rc, True, C.MULTI["maxdist"], C.MULTI["minclustsize"])
        out["multi"]["rc%d" % rc] = record(b, mums=len(mums))
    for name, c in C.abstract_cases().items():
        b = reference_blocks(fns, c["mums"], c["ranges"], c["rc"], c["kw"]["cluster"], c["kw"]["maxdist"], c["kw"]["minclustsize"])
        out["abstract"][name] = record(b, mums=len(c["mums"]))
    path = os.path.join(ROOT, "tests", "golden", "blocks.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for k in ("1a+1b|rc0|defaults", "1a+1b|rc1|defaults", "1a+1brc|rc1|defaults"):
        r = out["fixtures"][k]
        print(k, r["mums"], "MUMs ->", r.get("count", len(r.get("blocks", []))), "blocks")
    print("multi:", {k: (v["mums"], len(v["blocks"])) for k, v in out["multi"].items()})
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
