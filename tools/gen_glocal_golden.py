#!/usr/bin/env python3
"""Golden file of the glocal chain tests from the reference's own glocalchain + gapcost (reveal/transform.py:947-1244) -- TEST INFRASTRUCTURE, build
container only.

The reference is Python 2.  This script converts reveal/transform.py IN MEMORY with lib2to3 (nothing of it is written to the repository), pulls the two
functions out of the converted syntax tree and executes THEM with useheap=False, update_progress stubbed.  One thing is rewritten in the extracted
tree: glocalchain compares None with integers (`pblock[c2] >= block[c2]` on a dummy, transform.py:1055), which Python 2 allows -- None sorts below
everything -- and Python 3 refuses.  Every <, <=, >, >= of the two functions goes through a helper with Python 2's ordering; the result there is always
and-ed with `prefid != None`, so the outcome is the reference's.

Per case of tests/glocal_cases.py (cases() under "cases", large_cases() under "large"): one pass on either axis (the chain as indices of the kept input blocks, the end score from the function's own log
line) and, for the cases named there, the two loops of transform.py:307-356.  An empty list is written as the library defines it (an empty chain).

    python tools/gen_glocal_golden.py      # rewrites tests/golden/glocal.json
"""
import ast
import json
import logging
import os
import re
import sys
import time
from lib2to3 import refactor

REF = "/root/reference/reveal"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import glocal_cases as C                      # noqa: E402


def _py2_order(op, a, b):
    """a op b as Python 2 orders None: below everything, equal to itself"""
    if a is None or b is None:
        ka, kb = (0 if a is None else 1), (0 if b is None else 1)
        a, b = ka, kb
    return {"Lt": a < b, "LtE": a <= b, "Gt": a > b, "GtE": a >= b}[op]


class Py2Compare(ast.NodeTransformer):
    def visit_Compare(self, node):
        self.generic_visit(node)
        if len(node.ops) == 1 and type(node.ops[0]).__name__ in ("Lt", "LtE", "Gt", "GtE"):
            return ast.Call(func=ast.Name(id="_py2_order", ctx=ast.Load()), args=[ast.Constant(type(node.ops[0]).__name__), node.left, node.comparators[0]], keywords=[])
        assert not any(type(o).__name__ in ("Lt", "LtE", "Gt", "GtE") for o in node.ops), "a chained ordering comparison"
        return node


class Capture(logging.Handler):
    score = None

    def emit(self, record):
        m = re.match(r"Optimal glocal chain contains: (\d+) anchors and scores (-?\d+)", record.getMessage())
        if m:
            self.score = int(m.group(2))


def load():
    tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    path = os.path.join(REF, "transform.py")
    src = open(path).read()
    if not src.endswith("\n"):
        src += "\n"
    tree = ast.parse(str(tool.refactor_string(src, path)))
    names = {"glocalchain", "gapcost"}
    body = [Py2Compare().visit(n) for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == names
    env = {"logging": logging, "update_progress": lambda *a, **k: None, "time": time, "sys": sys, "_py2_order": _py2_order}
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), env)
    return env["glocalchain"]


CAP = Capture()


def one_pass(fn, blocks, c, axis, kw=None):
    """-> (chain as tuples, end score): the function appends its dummies to the list it is given and sorts it, so it gets a copy"""
    if not blocks:
        return [], None
    CAP.score = None
    chain = fn([tuple(b) for b in blocks], c["rlength"], c["qlength"], [tuple(r) for r in c["ctg2range"]], useheap=False, axis=axis, **(kw or c["kw"]))
    return chain, CAP.score


def loops(fn, blocks, c, kw=None):
    """transform.py:307-356 -> (chain, passes per axis, blocks after every pass)"""
    cur, passes, after = [tuple(b) for b in blocks], [0, 0], []
    for axis in (0, 1):
        nbefore, nafter = len(cur), None
        while nbefore != nafter:
            nbefore = len(cur)
            cur = one_pass(fn, cur, c, axis, kw)[0]
            nafter = len(cur)
            passes[axis] += 1
            after.append(nafter)
    return cur, passes, after


def main():
    logging.getLogger().setLevel(logging.INFO)
    logging.getLogger().handlers[:] = [CAP]
    fn = load()
    out = {"cases": {}, "multi": {}}
    cases = C.cases()
    for name, c in cases.items():
        rec = {"n": len(c["blocks"])}
        for axis in (0, 1):
            chain, score = one_pass(fn, c["blocks"], c, axis)
            rec["axis%d" % axis] = C.chain_record(C.indices(c["blocks"], chain))
            rec["score%d" % axis] = score
        if name in C.FILTERED:
            chain, passes, after = loops(fn, c["blocks"], c)
            rec["filter"] = dict(chain=C.chain_record(C.indices(c["blocks"], chain)), passes=passes, after=after)
        out["cases"][name] = rec
    g = out["cases"]
    # what the cases are there for
    for o in (0, 1):
        assert g["wide_o%d" % o]["score0"] > 1 << 32 and g["wide_o%d" % o]["score1"] > 1 << 32, "wide: the end score stays inside 32 bits"
    f = g["passes_second_drops"]["filter"]
    assert f["passes"][0] >= 3 or f["passes"][1] >= 3, "no second pass drops a block: %s" % f
    f = g["passes_four"]["filter"]
    assert max(f["passes"]) >= 4, "fewer than four passes: %s" % f
    for name in ("window_n1_bp0", "window_n2_bp10", "window_n8_bp100", "lastn100_150", "ties", "long_span"):
        assert 0 < len(g[name]["axis0"]) < g[name]["n"] and 0 < len(g[name]["axis1"]) < g[name]["n"], name
    assert g["window_n1_bp0"]["axis0"] != g["window_n8_bp100"]["axis0"], "the window does not matter at 70 blocks"
    # the large cases: the same per case, under "large"
    out["large"] = {}
    large = C.large_cases()
    for name, c in large.items():
        rec = {"n": len(c["blocks"])}
        for axis in (0, 1):
            chain, score = one_pass(fn, c["blocks"], c, axis)
            idx = C.indices(c["blocks"], chain)
            if name.startswith("collinear"):
                assert axis == 1 or idx == list(range(rec["n"])), "%s: the chain on axis 0 is not the whole list" % name
            if name.startswith("far_") and name.endswith("axis%d" % axis):
                between = int(name.split("_")[1])
                _, a, b = C.far_blocks(between, axis)
                assert idx[idx.index(b) - 1] == a, "%s: the block behind the gap is not reached from the last one in front of it" % name
            rec["axis%d" % axis] = C.chain_record(idx)
            rec["score%d" % axis] = score
        if name in C.LARGE_FILTERED:
            chain, passes, after = loops(fn, c["blocks"], c)
            rec["filter"] = dict(chain=C.chain_record(C.indices(c["blocks"], chain)), passes=passes, after=after)
        out["large"][name] = rec
    gl = out["large"]
    f = gl["passes_big"]["filter"]
    assert max(f["passes"]) >= 3 and f["after"][0] > C.WG, "passes_big: fewer than three passes on either axis, or a second pass of one workgroup: %s" % f
    for o in (0, 1):
        assert gl["wide_600_o%d" % o]["score0"] > 1 << 32 and gl["wide_600_o%d" % o]["score1"] > 1 << 32, "wide_600: the end score stays inside 32 bits"
    # end to end: the loops on the blocks of blocks_cases.multi_case() with the command line's weights
    blocks, nodes, rlength, qlength = C.multi_blocks()
    c = dict(blocks=blocks, ctg2range=nodes, rlength=rlength, qlength=qlength)
    chain, passes, after = loops(fn, blocks, c, C.COMMAND)
    out["multi"] = dict(n=len(blocks), chain=C.chain_record(C.indices(blocks, chain)), passes=passes, after=after)
    path = os.path.join(ROOT, "tests", "golden", "glocal.json")
    with open(path, "w") as f:
        rows = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in sorted(out["cases"].items()))      # a case per line
        lrows = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in sorted(out["large"].items()))
        f.write('{"cases": {\n%s\n},\n"large": {\n%s\n},\n"multi": %s}\n' % (rows, lrows, json.dumps(out["multi"], sort_keys=True, separators=(",", ":"))))
    for name in ("passes_second_drops", "passes_four", "lastn100_150", "wide_o1"):
        print(name, g[name]["n"], "blocks ->", len(g[name]["axis0"]), "/", len(g[name]["axis1"]), "filter", g[name]["filter"]["passes"], g[name]["filter"]["after"])
    for name, rec in sorted(gl.items()):
        print(name, rec["n"], "blocks ->", [rec[a]["count"] if isinstance(rec[a], dict) else len(rec[a]) for a in ("axis0", "axis1")],
              "filter %s %s" % (rec["filter"]["passes"], rec["filter"]["after"]) if "filter" in rec else "")
    print("multi:", out["multi"])
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
