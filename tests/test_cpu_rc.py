"""The reverse complement of construct(rc=1) as a host rule (rv_revcomp_bytes: rv_comp_of of csrc/rv_revcomp.h in the host loop, no device is
asked for) against the CPU oracle's revcomp, on the ranges of tests/rc_cases.py and on every byte value."""
import ctypes

import numpy as np

import rc_cases as C
from helpers import oracle


def _dll():
    from reveal_amd import _lib
    return _lib.get(False).dll, _lib.get(True).dll


def revcomp_bytes(dll, data):
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    assert dll.rv_revcomp_bytes(buf, len(data)) == 0
    return buf.raw[:len(data)]


def oracle_revcomp(data):
    t = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    oracle(False).revcomp(t)
    return t.tobytes()


def _ranges():
    for name, case in list(C.small_cases().items()) + list(C.fixture_cases().items()):
        T, nsep, _ = C.text_of(case)
        yield name, T[nsep[0]:]
    for r, c in C.ALIGNMENT_GRID:
        T, nsep, _ = C.text_of(C.alignment_case(r, c))
        yield "align_%d_%d" % (r, c), T[nsep[0]:]


def test_host_rule_equals_the_oracle_on_every_case():
    for dll in _dll():
        for name, rng in _ranges():
            assert revcomp_bytes(dll, rng) == oracle_revcomp(rng), name


def test_host_rule_on_single_bytes():
    """every byte value the oracle's table takes (0..127) gives the oracle's byte; bytes of 128 and above -- where the reference indexes its table
    with a negative char -- stay as they are"""
    for dll in _dll():
        for b in range(128):
            assert revcomp_bytes(dll, bytes([b])) == oracle_revcomp(bytes([b])), b
        for b in range(128, 256):
            assert revcomp_bytes(dll, bytes([b])) == bytes([b]), b
        assert revcomp_bytes(dll, b"") == b""


# the reference's table folds U into A's class and ` into @: U -> A -> T, u -> a -> t, ` -> @ -> @.  On every other byte value the rule is its own inverse.
NOT_INVOLUTIVE = {ord("U"): (ord("A"), ord("T")), ord("u"): (ord("a"), ord("t")), 96: (64, 64)}


def test_host_rule_is_its_own_inverse():
    for dll in _dll():
        for b in range(256):
            once = revcomp_bytes(dll, bytes([b]))
            twice = revcomp_bytes(dll, once)
            if b in NOT_INVOLUTIVE:
                assert (once[0], twice[0]) == NOT_INVOLUTIVE[b], b
            else:
                assert twice == bytes([b]), b
        every = bytes(b for b in range(256) if b not in NOT_INVOLUTIVE) * 3 + b"ACGT"
        assert revcomp_bytes(dll, revcomp_bytes(dll, every)) == every
        assert revcomp_bytes(dll, b"AACG$TN") == b"NA$CGTT"
