"""shared cases of the construct(rc=1) tests (tests/test_cpu_rc.py, tests/test_gpu_rc_device.py): texts whose range T[nsep[0], n) -- the part
construct(rc=1) reverses and complements -- meets every path of k_text_revcomp (reveal_amd/csrc/rv_revcomp.hip).  Everything is small and seeded.

A case is a list of samples, each a list of sequences (bytes), fed with toupper=False.  The range holds the separator of the first sample, the
later samples' sequences and one '$' behind each: a single later sequence of c bytes gives a range of c + 2."""
import random

from helpers import assemble, fa

P = 32          # bytes one thread pair moves: 2 x RV_RC_PIECE (rv_revcomp.h)
G = 256 * P     # bytes one workgroup moves: RV_RC_THREADS pairs

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rnd(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _related(rng, ref, c):
    """a sequence of c bytes: random flanks round the reverse complement of (a piece of) ref with a few substitutions, so that MUMs exist"""
    core = bytearray(ref[:max(0, min(len(ref), c - 2))].translate(_COMP)[::-1])
    for k in range(len(core)):
        if rng.random() < 0.03:
            core[k] = rng.choice(b"ACGT")
    left = (c - len(core)) // 2
    return _rnd(rng, left) + bytes(core) + _rnd(rng, c - len(core) - left)


RANGE_LENGTHS = (3, 4, 5, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, G - 1, G, G + 1, G + P + 1, 5 * G + 17)


def length_case(length, seed=0):
    """two samples of one sequence each, the range `length` bytes long"""
    rng = random.Random(1000003 * length + seed)
    c = length - 2
    ref = _rnd(rng, min(max(c, 8), 900) + 17)
    return [[ref], [_related(rng, ref, c)]]


ALIGN_L = 2 * P + 3      # just above 2 P: at least one pair and a middle, whatever the peeled head


def alignment_case(reflen, ctglen):
    """the range begins at text position reflen and is ctglen + 2 bytes long: reflen 1..16 x ctglen ALIGN_L..ALIGN_L+15 brings every value of
    lo mod 16 together with every value of (lo + len) mod 16"""
    rng = random.Random(7919 * reflen + ctglen)
    ref = _rnd(rng, reflen)
    return [[ref], [_rnd(rng, ctglen)]]


ALIGNMENT_GRID = [(r, ALIGN_L + d) for r in range(1, 17) for d in range(16)]

ALPHABET = bytes(b for b in range(1, 128) if b != ord("$"))      # every byte value addsequence takes, the separator apart


def alphabet_case():
    """sequences over every byte value 1..127 except '$': both cases, the IUPAC letters, U, ` and punctuation, control bytes"""
    rng = random.Random(127)
    a = bytearray(ALPHABET * 3)
    rng.shuffle(a)
    b = bytearray(bytes(a)[40:300][::-1] + ALPHABET * 2)
    for k in range(0, len(b), 37):
        b[k] = rng.choice(ALPHABET)
    return [[bytes(a)], [bytes(b)]]


def shape_cases():
    """name -> samples"""
    rng = random.Random(31337)
    ref = _rnd(rng, 700)
    three = [_related(rng, ref[:300], 333), b"G", _related(rng, ref[300:], 415)]
    more = [[ref], [_related(rng, ref, 500)], [_related(rng, ref, 611), _rnd(rng, 45)]]
    return {"three_contigs_one_single_base": [[ref], three], "three_samples": more}


def fixture_cases():
    """name -> FASTA paths of tests/golden"""
    return {"1a+1brc": fa("1a", "1brc"), "1a+1b": fa("1a", "1b")}


def small_cases():
    """name -> samples: the length, alphabet and shape cases (the alignment grid and the fixtures are run apart)"""
    C = {"len_%d" % n: length_case(n) for n in RANGE_LENGTHS}
    C["alphabet"] = alphabet_case()
    C.update(shape_cases())
    return C


def text_of(inputs):
    """-> (T bytes, nsep, nodes) of a case or a list of FASTA paths, as the index assembles it with toupper=False"""
    return assemble(inputs, toupper=False)
