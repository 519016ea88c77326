#!/usr/bin/env python3
"""Golden file of the layout tests from the reference's own merge_consecutive, remove_overlap_conservative_blocks, remove_overlap_greedy_blocks,
chainscore, optimise, extendblocks and gapcost (reveal/transform.py) -- TEST INFRASTRUCTURE, build container only.

The reference is Python 2.  This script converts reveal/transform.py IN MEMORY with lib2to3 (nothing of it is written to the repository), pulls the
seven functions out of the converted syntax tree and executes THEM, update_progress stubbed.  One thing is rewritten in the extracted tree: every `/`
becomes `//` (the operands are integers there, and Python 2 divides them with a floor).

Per merge case of tests/layout_cases.py: the merged list (long ones as count + digest).  Per tail case: the list behind every stage of
transform.py:376-435 and 528-530, each stage run on the reference's own output of the one before; where the reference raises, the exception's type,
and nothing behind it.  The file holds data only.

    python tools/gen_layout_golden.py            # rewrites tests/golden/layout.json
    python tools/gen_layout_golden.py --search   # prints, for a range of seeds, what the tail lists do (how layout_cases.TAIL was chosen)
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

import layout_cases as C                      # noqa: E402

NAMES = {"merge_consecutive", "remove_overlap_conservative_blocks", "remove_overlap_greedy_blocks", "chainscore", "optimise", "extendblocks", "gapcost"}


class FloorDiv(ast.NodeTransformer):
    def visit_BinOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Div):
            node.op = ast.FloorDiv()
        return node


def load():
    tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
    path = os.path.join(REF, "transform.py")
    src = open(path).read()
    if not src.endswith("\n"):
        src += "\n"
    tree = ast.parse(str(tool.refactor_string(src, path)))
    body = [FloorDiv().visit(n) for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert {n.name for n in body} == NAMES
    env = {"logging": logging, "update_progress": lambda *a, **k: None, "sys": sys}
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), env)
    return env


def tup(blocks):
    return [tuple(b) for b in blocks]


def tail(env, c):
    """transform.py:376-435, 528-530 with the reference's functions -> the record of a tail case, and (blocks dropped by a sweep, accepted sweeps)"""
    kw, args = c["kw"], (c["rlength"], c["qlength"], tup(c["ctg2range"]))
    rec = {"n": len(c["chain"])}
    stats = dict(dropped=0, sweeps=0, raises=None)

    def stage(name, fn):
        try:
            out = fn()
        except (IndexError, AssertionError) as e:
            rec[name] = {"raises": type(e).__name__}
            stats["raises"] = name
            return None
        return out

    blocks = env["merge_consecutive"](tup(c["chain"]))
    rec["merged"] = C.record(blocks)
    blocks = stage("overlap", lambda: env["remove_overlap_greedy_blocks" if c["greedy"] else "remove_overlap_conservative_blocks"](tup(blocks)))
    if blocks is None:
        return rec, stats
    rec["overlap"] = C.record(blocks)
    blocks = [b for b in blocks if b[5] >= c["minchainsum"]]
    rec["filtered"] = C.record(blocks)
    blocks = env["merge_consecutive"](blocks)
    rec["merged2"] = C.record(blocks)
    w, cost, edges = env["chainscore"](tup(blocks), *args, **kw)
    rec["chainscore"] = [w, cost, edges]
    if len(blocks) > 1:
        t, tw, tc, te = env["optimise"](tup(sorted(blocks, key=lambda s: s[0])), *args, **kw)
        rec["sweep"] = dict(blocks=C.record(t), weight=tw, cost=tc, edgecosts=te)
        weight, cost, edgecosts = env["chainscore"](blocks, *args, **kw)
        score = weight - cost
        while True:
            t, tw, tc, te = env["optimise"](blocks, *args, **kw)
            if tw - tc <= score:
                break
            stats["dropped"] += len(blocks) - len(t)
            stats["sweeps"] += 1
            score, blocks, weight, cost, edgecosts = tw - tc, t, tw, tc, te
            blocks = env["merge_consecutive"](blocks)
        rec["loop"] = dict(blocks=C.record(blocks), weight=weight, cost=cost, edgecosts=edgecosts, sweeps=stats["sweeps"])
    blocks = env["merge_consecutive"](blocks)
    weight, cost, edgecosts = env["chainscore"](blocks, *args, **kw)
    assert len(edgecosts) == len(blocks) + 1
    rec["final"] = dict(blocks=C.record(sorted(blocks, key=lambda s: s[0])), weight=weight, cost=cost, edgecosts=edgecosts)
    blocks = tup(blocks)
    if stage("extended", lambda: (env["extendblocks"](blocks, tup(c["ctg2range"])), blocks)[1]) is not None:      # (it extends the list it is given)
        rec["extended"] = C.record(blocks)
    return rec, stats


def search(env):
    for seed in range(60):
        for n in (18, 25, 33, 45, 60):
            for greedy in (False, True):
                for w in ("command", "small"):
                    c = dict(chain=C.tail_list(seed, n), ctg2range=list(C.RANGES), rlength=C.SEP, qlength=C.RANGES[-1][1] + 1 - C.SEP, greedy=greedy, minchainsum=50,
                             kw=dict(C.COMMAND if w == "command" else C.SMALL))
                    rec, st = tail(env, c)
                    if st["dropped"] or st["raises"]:
                        print(C.tail_name(seed, n, greedy, w), st)


def main():
    logging.getLogger().setLevel(logging.ERROR)
    env = load()
    if "--search" in sys.argv:
        return search(env)
    out = {"merge": {}, "tail": {}}
    for name, c in C.merge_cases().items():
        got = env["merge_consecutive"](tup(C.merge_list(c)))
        out["merge"][name] = dict(n=len(C.merge_list(c)), merged=C.record(got))
    g = out["merge"]
    # what the cases are there for
    assert g["join_o0"]["merged"] == [[100, 380, 10100, 10380, 0, 140, 0, 2]] and g["join_o1"]["merged"] == [[100, 380, 10100, 10360, 1, 140, 0, 2]]
    for name in ("o1_ranks_ascending", "o0_ranks_descending", "ranks_not_adjacent", "other_ctgid", "equal_s2_o1"):
        assert len(g[name]["merged"]) == g[name]["n"], name
    assert len(g["other_refid_joins"]["merged"]) == 1 and len(g["mixed_o"]["merged"]) == 3
    assert len(g["equal_s1_first"]["merged"]) == 3 and len(g["equal_s1_second"]["merged"]) == 1 and len(g["equal_s2_o0"]["merged"]) == 1
    assert len(g["run_257"]["merged"]) == 1 and len(g["run_1025_o1"]["merged"]) == 1
    assert g["singles_256"]["merged"]["count"] == 256 and g["singles_257"]["merged"]["count"] == 257 and g["run_254_258"]["merged"]["count"] == 596
    assert g["scores_2p31"]["merged"][0][5] == 5 << 31 and len(g["wide_coordinates"]["merged"]) == 4
    assert 2300 // 9 < g["runs_2300"]["merged"]["count"] < 2300 and g["sel_600"]["n"] == 300
    stats = {}
    for name, c in C.tail_cases().items():
        out["tail"][name], stats[name] = tail(env, c)
    raising = [n for n, s in stats.items() if s["raises"]]
    assert 5 * len(raising) <= len(stats), "more than one tail case in five raises: %s" % raising
    assert stats[C.TAIL_DROPS]["dropped"] >= 1, stats[C.TAIL_DROPS]
    assert stats[C.TAIL_TWO_SWEEPS]["sweeps"] >= 2, stats[C.TAIL_TWO_SWEEPS]
    path = os.path.join(ROOT, "tests", "golden", "layout.json")
    with open(path, "w") as f:
        parts = []
        for key in ("merge", "tail"):
            rows = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in sorted(out[key].items()))      # a case per line
            parts.append('"%s": {\n%s\n}' % (key, rows))
        f.write("{%s}\n" % ",\n".join(parts))
    print("merge cases: %d; tail cases: %d, raising %d (%s), sweeps accepted in %d, blocks dropped in %d" % (
        len(out["merge"]), len(stats), len(raising), sorted(set(stats[n]["raises"] for n in raising)), sum(1 for s in stats.values() if s["sweeps"]),
        sum(1 for s in stats.values() if s["dropped"])))
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
