#!/usr/bin/env python3
"""Digests of the oracle's arrays for the two large inputs of tests/construct_paths_cases.py (D11: a common prefix of 2^21 - 1 and
of 2^21 bases, 4.2 x 10^6 positions each) -- TEST INFRASTRUCTURE ONLY.

    python oracle/gen_construct_paths_golden.py

The oracle needs seconds per input and width, which a GPU test of a few seconds cannot spend: tests/golden/construct_paths.json holds
sha256 of SA, LCP and the list of getmums(20), the largest LCP and the seconds the CPU took.  tests/test_gpu_construct_paths.py compares
the library's arrays with these digests; tests/test_cpu_construct_paths.py makes them again and compares."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "construct_paths.json")


def record(cid):
    import numpy as np
    import construct_paths_cases as C
    from oracle import oracle_ctypes
    c = C.case(cid)
    T, nsep = C.text_of(c)
    O = oracle_ctypes.Oracle(False)
    t0 = time.perf_counter()
    r = O.construct(T, nsep, len(c["samples"]))
    l, a, b = O.getmums(r["tbuf"], r["SA"], r["LCP"], nsep, 20)
    t1 = time.perf_counter()
    mums = np.stack([np.asarray(l, dtype=np.int64), np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)], axis=1) if len(l) else np.zeros((0, 3), dtype=np.int64)
    return {"n": len(T), "sha_SA": C.digest(r["SA"]), "sha_LCP": C.digest(r["LCP"]), "sha_mums": C.digest(mums), "mums": int(len(l)),
            "maxlcp": int(r["LCP"].max())}, round(t1 - t0, 2)


def main():
    import construct_paths_cases as C
    data = {}
    for cid in C.LARGE_IDS:
        data[cid], secs = record(cid)
        data[cid]["cpu_seconds"] = secs
        print(cid, json.dumps(data[cid]), flush=True)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
