"""glocalchain's rule on the CPU: the Python restatement (reveal_amd.transform.glocalchain_python) and the library's host C++ (glocalchain_native,
rv_glocal_host: no device is asked for) against tests/golden/glocal.json, which tools/gen_glocal_golden.py wrote from the reference's own glocalchain
(one pass per axis, and the two loops of transform.py:307-356); what rv_glocal_admit takes and refuses; what the list validation refuses."""
import pytest

import glocal_cases as C
from reveal_amd import transform

GOLD = C.golden()
CASES = C.cases()
ADMITTED = [n for n in CASES if n not in C.REFUSED]


def args(c):
    return c["blocks"], c["rlength"], c["qlength"], c["ctg2range"]


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_python_matches_the_reference(name, axis):
    c = CASES[name]
    blocks = list(c["blocks"])
    got = transform.glocalchain_python(blocks, *args(c)[1:], axis=axis, **c["kw"])
    assert blocks == c["blocks"]                                             # the reference appends its dummies to the caller's list and sorts it; this does not
    assert C.matches(C.indices(c["blocks"], got), GOLD["cases"][name]["axis%d" % axis])
    assert got is not blocks


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", ADMITTED)
def test_native_matches_the_reference(name, axis, sa64):
    c = CASES[name]
    got = transform.glocalchain_native(*args(c), axis=axis, sa64=sa64, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), GOLD["cases"][name]["axis%d" % axis])


@pytest.mark.parametrize("route", ["python", "host"])
@pytest.mark.parametrize("name", C.FILTERED)
def test_filter_matches_the_reference_loops(name, route):
    c = CASES[name]
    want = GOLD["cases"][name]["filter"]
    if name in C.REFUSED and route == "host":
        with pytest.raises(transform.error, match="outside the library's integer arithmetic"):
            transform.glocal_filter(*args(c), route="host", **c["kw"])
        return
    got, info = transform.glocal_filter(*args(c), route=route, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), want["chain"])
    if c["blocks"]:
        assert list(info["passes"]) == want["passes"] and info["after"] == want["after"]
    assert info["route"] == route


def test_filter_one_axis_at_a_time():
    """axes=(0,) then axes=(1,) on its result is the filter"""
    c = CASES["passes_four"]
    want = GOLD["cases"]["passes_four"]["filter"]
    first, i0 = transform.glocal_filter(*args(c), axes=(0,), route="host", **c["kw"])
    assert i0["passes"] == (want["passes"][0], 0) and i0["after"] == want["after"][:want["passes"][0]]
    second, i1 = transform.glocal_filter(first, *args(c)[1:], axes=(1,), route="host", **c["kw"])
    assert i1["passes"] == (0, want["passes"][1])
    assert C.matches(C.indices(c["blocks"], second), want["chain"])


def test_expectations():
    """what the cases are there for, spelled out"""
    g = GOLD["cases"]
    assert g["empty"]["axis0"] == g["empty"]["axis1"] == [] and g["one"]["axis0"] == g["one"]["axis1"] == [0]
    assert max(g["passes_four"]["filter"]["passes"]) >= 4
    f = g["passes_second_drops"]["filter"]
    n0 = f["passes"][0]
    assert (n0 >= 3 and f["after"][1] < f["after"][0]) or (f["passes"][1] >= 3 and f["after"][n0 + 1] < f["after"][n0])
    for o in (0, 1):
        assert g["wide_o%d" % o]["score0"] > 1 << 32 and g["wide_o%d" % o]["score1"] > 1 << 32
    assert g["window_n1_bp0"]["axis0"] != g["window_n8_bp100"]["axis0"]      # the window matters at 70 blocks
    assert GOLD["multi"]["n"] == len(C.multi_blocks()[0]) and len(GOLD["multi"]["chain"]) > 0


# ---- the large cases (glocal_cases.large_cases): the golden records under "large" pinned here, without a GPU
LARGE = C.large_cases()


# (the Python rule takes seconds on 2000 entries with whole-prefix windows: the far_2047 / far_2048 lists run it on the axis they are built on)
@pytest.mark.parametrize("name,axis", [(n, a) for n in LARGE for a in (0, 1) if not (n.startswith("far_20") and a == 1)])
def test_large_python_matches_the_reference(name, axis):
    c = LARGE[name]
    got = transform.glocalchain_python(*args(c), axis=axis, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), GOLD["large"][name]["axis%d" % axis])


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", list(LARGE))
def test_large_native_matches_the_reference(name, axis, sa64):
    c = LARGE[name]
    got = transform.glocalchain_native(*args(c), axis=axis, sa64=sa64, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), GOLD["large"][name]["axis%d" % axis])


@pytest.mark.parametrize("route", ["python", "host"])
@pytest.mark.parametrize("name", C.LARGE_FILTERED)
def test_large_filter_matches_the_reference_loops(name, route):
    c = LARGE[name]
    want = GOLD["large"][name]["filter"]
    got, info = transform.glocal_filter(*args(c), route=route, **c["kw"])
    assert C.matches(C.indices(c["blocks"], got), want["chain"])
    assert list(info["passes"]) == want["passes"] and info["after"] == want["after"] and info["route"] == route


def test_large_reach():
    """the arithmetic that takes each large case to the line of rv_glocal.hip it is there for"""
    g = GOLD["large"]
    assert set(g) == set(LARGE) and all(g[n]["n"] == len(LARGE[n]["blocks"]) for n in LARGE)
    assert set(C.LARGE_FILTERED) <= set(LARGE) and set(C.WHOLE_PREFIX) <= set(LARGE) and set(C.LARGE_BUDGETS) <= set(C.WHOLE_PREFIX)
    for c in LARGE.values():
        assert tuple(C.entries(c, a) - len(c["blocks"]) for a in (0, 1)) == C.NDUMMY
    # entries_256_*: m + 2 slots, the grid of every per-entry kernel, from two below 256 to two above it: one workgroup and two, with
    # k = m and k = m + 1 (what the guards k > m and k <= m + 1 tell apart) on either side of the workgroup border
    slots = sorted({C.entries(LARGE["entries_256_%d" % n], a) + 2 for n in (250, 251, 252, 253) for a in (0, 1)})
    assert slots == [254, 255, 256, 257, 258]
    assert {-(-s // C.WG) for s in slots} == {1, 2}
    # collinear_n: the path from `end` runs through all n blocks (the generator asserts it on the reference's chain; here the record is that chain),
    # so it is at least n steps long: at m + 1 = 256 and 1024 the last launch of k_glc_double is needed (2^(t-1) - 1 steps do not reach the first
    # block), at 257 and 1025 the count has just grown by one
    want = {253: (256, 8), 254: (257, 9), 1021: (1024, 10), 1022: (1025, 11)}
    for n in C.COLLINEAR:
        c, rec = LARGE["collinear_%d" % n], g["collinear_%d" % n]
        assert C.matches(list(range(n)), rec["axis0"])
        m = C.entries(c, 0)
        t = C.doubling_launches(m)
        assert (m + 1, t) == want[n] and 2 ** (t - 1) < m + 1 <= 2 ** t
        if (m + 1) & m == 0:
            assert 2 ** (t - 1) - 1 < n
        assert -(-(m + 2) // C.WG) >= 2
    # whole-prefix windows: no entry lies more than lastbp in front of another and lastn is above the list, so the walk back never ends early:
    # the k-th entry has k edges, the pass m (m + 1) / 2
    for name in C.WHOLE_PREFIX:
        c = LARGE[name]
        lo = min(min(b[0], b[2]) for b in c["blocks"])
        hi = max(e for _, e in c["ctg2range"])
        assert hi - lo <= c["kw"]["lastbp"] and c["kw"]["lastn"] > max(C.entries(c, 0), C.entries(c, 1))
    for axis in (0, 1):
        m = C.entries(LARGE["window_260"], axis)
        assert m >= 257 > C.AHEAD + 64 and m + 2 > C.WG                       # windows of 191, 192, 193, 256 and 257 edges: 1 .. m are all there
        for budget in C.LARGE_BUDGETS["window_260"]:
            assert C.whole_prefix_edges(m) // budget + 1 >= 30                # tiles of a few windows each: the long ones reach over their borders
        m = C.entries(LARGE["ring_2300"], axis)
        assert m > C.RING + C.AHEAD and m + 2 > C.SCAN_TILE                   # windows above the ring, every scan of the pass over two scan tiles
        assert -(-(m + 2) // C.WG) == (9, 10)[axis]                           # m + 2 = 2304 = 9 * 256 on axis 0, one more entry and workgroup on axis 1
        assert C.whole_prefix_edges(m) < 1 << 25                              # one tile at the default budget
        tiles = C.whole_prefix_edges(m) // C.RING_TILE_BUDGET + 1
        assert tiles == 6
        klo = C.first_entry_of_tile(tiles - 1, C.RING_TILE_BUDGET)
        assert C.RING < klo <= m and klo in (2237, 2238)                      # the last tile begins behind entry RING: its pre-load starts at klo - RING > 0
    # far_*: the best predecessor of block B (the generator asserts that the reference's chain reaches B from A[39]) lies `between` entries in front
    # of it in the sorted order, that is edge number `between` of its window: 191 = the last edge loaded ahead, 192 = the first of the tail loop,
    # 2047 = the oldest score in the ring, 2048 = the first one read from global memory
    assert {b for b, _ in C.FAR} == {C.AHEAD - 1, C.AHEAD, C.RING - 1, C.RING}
    for between, axis in C.FAR:
        blocks, a, b = C.far_blocks(between, axis)
        order = sorted(range(len(blocks)), key=lambda i: (blocks[i][2 * axis], -blocks[i][5]))
        assert order.index(b) - 1 - order.index(a) == between
    # passes_big: three passes on one axis, and the second pass' list is spread over several workgroups
    f = g["passes_big"]["filter"]
    assert max(f["passes"]) >= 3 and f["after"][0] > C.WG and g["passes_big"]["n"] + 2 > C.SCAN_TILE
    # wide_600: 2^40 coordinates and scores of more than 24 bits leave no room for one 64-bit key, and three workgroups gather the permutation
    for o in (0, 1):
        c = LARGE["wide_600_o%d" % o]
        mc, ms = max(e for _, e in c["ctg2range"]), max(b[5] for b in c["blocks"])
        assert mc.bit_length() + ms.bit_length() > 64 and -(-(C.entries(c, 0) + 2) // C.WG) == 3
        assert g["wide_600_o%d" % o]["score0"] > 1 << 32


def test_multi_case_filter():
    """the end-to-end list of synteny_chain (the golden blocks of blocks_cases.multi_case) through both CPU routes"""
    blocks, nodes, rlength, qlength = C.multi_blocks()
    want = GOLD["multi"]
    for route in ("python", "host"):
        got, info = transform.glocal_filter(blocks, rlength, qlength, nodes, route=route)      # the command line's defaults
        assert C.indices(blocks, got) == want["chain"] and list(info["passes"]) == want["passes"] and info["after"] == want["after"]


def test_admit_and_refuse():
    for name in ADMITTED:
        c = CASES[name]
        assert transform.glocal_admit(*args(c), **c["kw"]), name
    for name in C.REFUSED:
        c = CASES[name]
        assert not transform.glocal_admit(*args(c), **c["kw"]), name
        _, info = transform.glocal_filter(*args(c), **c["kw"])                   # no route asked for: Python's arithmetic by itself
        assert info["route"] == "python"
        with pytest.raises(transform.error):
            transform.glocalchain_native(*args(c), **c["kw"])
    c = CASES["ties"]
    assert transform.glocal_admit(*args(c), **dict(c["kw"], eps=2.0, alfa=3.0))     # integral floats are integers
    assert not transform.glocal_admit(*args(c), **dict(c["kw"], eps=(1 << 62) - 1))
    # the bound follows the list: the same weights on longer coordinates
    far = [(s1 + (1 << 50), e1 + (1 << 50), s2 + (1 << 50), e2 + (1 << 50), o, sc, r, g) for s1, e1, s2, e2, o, sc, r, g in CASES["one"]["blocks"]]
    rng = [(0, (1 << 50) + 4999)] + [((1 << 50) + s, (1 << 50) + e) for s, e in C.RANGES[1:]]
    assert transform.glocal_admit(far, (1 << 50) + C.SEP, 0, rng, eps=1 << 6)
    assert not transform.glocal_admit(far, (1 << 50) + C.SEP, 0, rng, eps=1 << 12)


@pytest.mark.parametrize("weight", ["rearrangecost", "inversioncost", "_lambda", "eps", "alfa", "gapopen"])
def test_negative_weight_raises(weight):
    c = CASES["cross"]
    kw = dict(c["kw"], **{weight: -1})
    for fn in (transform.glocalchain_python, transform.glocalchain_native):
        with pytest.raises(transform.error, match="negative weight"):
            fn(*args(c), **kw)
    with pytest.raises(transform.error, match="negative weight"):
        transform.glocal_filter(*args(c), route="host", **kw)


BAD = {
    "s_behind_e": ((200, 100, 10100, 10200, 0, 50, 0, 2), "coordinates"),
    "negative": ((-5, 100, 10100, 10200, 0, 50, 0, 2), "coordinates"),
    "orientation": ((100, 200, 10100, 10200, 2, 50, 0, 2), "orientation"),
    "refid_is_a_contig": ((100, 200, 10100, 10200, 0, 50, 2, 2), "refid"),
    "ctgid_is_a_reference": ((100, 200, 10100, 10200, 0, 50, 0, 1), "ctgid"),
    "ctgid_outside": ((100, 200, 10100, 10200, 0, 50, 0, 5), "ctgid"),
    "negative_score": ((100, 200, 10100, 10200, 0, -1, 0, 2), "score"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_validation(name):
    blk, what = BAD[name]
    c = CASES["one"]
    with pytest.raises(transform.error, match=what):
        transform.glocalchain_native(c["blocks"] + [blk], *args(c)[1:], **c["kw"])


def test_no_sequence_on_an_axis():
    c = CASES["one"]
    with pytest.raises(transform.error, match="no sequence on axis 1"):
        transform.glocalchain_python(c["blocks"], c["rlength"] + 10 ** 6, c["qlength"], c["ctg2range"], axis=1)
    with pytest.raises(transform.error, match="ctgid names no contig"):          # the library meets the block's ids first
        transform.glocalchain_native(c["blocks"], c["rlength"] + 10 ** 6, c["qlength"], c["ctg2range"], axis=1)
    far = (c["blocks"][0][:6] + (0, 0),)                                          # every sequence a contig: the block's refid names none
    with pytest.raises(transform.error, match="refid names no reference sequence"):
        transform.glocalchain_native(far, -1, c["qlength"], c["ctg2range"], axis=0)
