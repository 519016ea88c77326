"""Inputs that sit on either side of every decision rv_build_sa takes on the host (reveal_amd/csrc/rv_construct.hip:2496-3090).

Every case is a dict:
    id        its name
    decision  D1 .. D12 ("Both sides of the SA build's decisions")
    samples   the input: a list of samples, each a list of contigs (str)
    expect    census fields (index.sa_paths()) the DEFAULT build must report, read off the decision's code -- the line is cited
              beside each.  A value is an int, or one of the strings ">0" / "<=cap" for counts whose size the code does not fix
    claim     what the CPU test confirms with the oracle alone (n, copy counts, largest LCP, bytes below '$', positions mod 128)

`derive()` restates the host decisions that only need the text's byte statistics (alphabet, key layout, hint, twins, head kernel);
it is the written-down reasoning behind those fields of `expect`, never a copy of a run.  Nothing here needs a GPU or the library."""
import functools
import hashlib

import numpy as np

from helpers import assemble, synth

TINY_MAX = 1024          # rv_construct.hip:2505   n <= TINY_N / 2
HINT_K = 16              # :687
TEXT_LIM = 4096          # :1354
PK_BLOCK = 128           # :1363
MEDIUM_GROUP = 64        # :1499
FAR_MAXIT = 64           # :1961
LL_LIMIT = 4096 * 512    # :2111, :2139  LL_MAX_STEPS steps of 512 bytes
KP_MAXG, KP_MAXFIELD = 5, 4096      # :361-362

FIELDS = ("tiny", "short_alphabet", "ends_with_sep", "g", "K", "bits", "fused_asked", "fused_final", "hint_ns", "nd_bits", "collapse",
          "diag_table_tried", "diag_table_kept", "heads_kernel", "text_round", "text_mode", "packed_text", "text_big", "far_ran", "nd_table",
          "doubling_rounds", "slow_class", "text_jump", "lcp_list_overflow", "defer_max", "defer_cap", "lcp_by_rank")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a).astype(np.int64)).tobytes()).hexdigest()


def text_of(case):
    """-> (T bytes, nsep) as addsample / addsequence assemble it"""
    T, nsep, _ = assemble([list(s) for s in case["samples"]], toupper=False)
    return T, nsep


def feed_case(idx, case):
    for k, contigs in enumerate(case["samples"]):
        idx.addsample("s%d" % k)
        for c in contigs:
            idx.addsequence(c)
    return idx


# ---- the host decisions that need only the text's statistics ---------------------------------------------------------------------------
def _bitlen(v):
    return int(v).bit_length()


def key_layout(sigma, radix, n, nseps, digit_bits=8):
    """rv_construct.hip:2555-2596 -> (g, K, bits)"""
    base = float(sigma - 1) if sigma > 2 else 2.0                                # :2559
    want = float(n) * (16.0 if nseps > 1 else 1.0)                               # :2562
    passes = lambda b: 0 if b <= 0 else (b + digit_bits - 1) // digit_bits       # rv_prims.hip:345
    best = (0, 0, 0)
    rg = 1
    for g in range(1, KP_MAXG + 1):
        rg *= radix
        if rg > KP_MAXFIELD and g > 1:                                           # :2567
            break
        fb = _bitlen(rg - 1)

        def bits_of(k):
            return (k // g) * fb + (_bitlen(radix ** (k % g) - 1) if k % g else 0)
        exact = True                                                             # :2570-2576
        f = np.arange(rg, dtype=np.uint64)
        for i in range(1, g):
            d = radix ** (g - i)
            m = ((1 << 20) + d - 1) // d
            exact = exact and bool(np.all(((f * np.uint64(m)) >> np.uint64(20)) == f // np.uint64(d))) and (rg - 1) * m < (1 << 32)
        if not exact:
            continue
        k, cap = 1, base
        while cap < want and bits_of(k + 1) <= 62:                               # :2578
            cap *= base
            k += 1
        p = passes(bits_of(k))
        while bits_of(k + 1) <= 62 and passes(bits_of(k + 1)) == p:              # :2580
            k += 1
        b = bits_of(k)
        if k > best[1] or (k == best[1] and b < best[2]):                        # :2582
            best = (g, k, b)
    return best


def derive(T, nsep, no_tiny=False, no_short=False, no_diag=False, no_packed=False, no_heads_fusion=False, no_fused=False):
    """the census fields that follow from the text's bytes and separators alone, for the default build or one switch"""
    n = len(T)
    if n <= TINY_MAX and not no_tiny:                                            # :2505
        e = {f: 0 for f in FIELDS}
        e.update(tiny=1, fused_asked=1, fused_final=1)
        return e
    a = np.frombuffer(T, dtype=np.uint8)
    hist = np.bincount(a, minlength=256)
    sigma = int((hist > 0).sum())                                                # :2537
    radix = 256 if sigma >= 255 else sigma + 1                                   # :2540-2541
    twice = bool(np.any((a[:-1] == 36) & (a[1:] == 36)))                         # hist[256], :69-72
    short = (2 <= sigma < 255 and hist[36] > 0 and int(np.nonzero(hist)[0][0]) == 36 and not twice and not no_short)      # :2546
    ends = short and T[-1:] == b"$"                                              # :2548
    if short and ends:
        radix = sigma                                                            # :2551
    g, K, bits = key_layout(sigma, radix, n, len(nsep))
    fused = bits <= 48 and not no_fused                                          # :2607
    at_bits = 5 if K <= 30 else 8                                                # :2612
    at_shift, nd_shift = 56 - at_bits, (bits + 7) // 8 * 8                       # :2612-2613
    D = nsep[0] + 1 if (nsep and 0 < nsep[0] < n - 1) else 0                     # :2614
    ns = 0
    if nsep and D > 0:                                                           # :2618-2626
        ns = min(len(nsep) + 1, HINT_K)
        if len(nsep) + 1 > HINT_K:
            ns = 0
    want_hint = fused and D > 0 and ns >= 2 and at_shift - nd_shift >= 8 and not no_diag and not no_packed      # :2627
    nd_bits = min(at_shift - nd_shift - 1, 11) if want_hint else 0               # :2628
    collapse = fused and nd_bits > 0 and ns == 2 and K < 64 and D > 1 and n > D + 1 and not no_heads_fusion     # :2666
    heads = 2 if collapse else (1 if fused and nd_bits > 0 and not no_heads_fusion else 0)                      # :2763-2787
    return dict(tiny=0, short_alphabet=int(short), ends_with_sep=int(ends), g=g, K=K, bits=bits, fused_asked=int(fused), hint_ns=ns,
                nd_bits=nd_bits, collapse=int(collapse), heads_kernel=heads, lcp_by_rank=0)


def text_mode_of(e):
    """the work division the text round takes when it runs (:2958): 3 with the hint on the fused path, else 1"""
    return 3 if e["nd_bits"] > 0 and e["fused_asked"] else 1


# ---- generators ---------------------------------------------------------------------------------------------------------------------------
def _rnd(rng, L, letters="ACGT"):
    return "".join(letters[x] for x in rng.integers(0, len(letters), L))


def _snp(rng, s, rate, keep=()):
    """substitutions at `rate`, none inside the (lo, hi) ranges of `keep`"""
    b = list(s)
    for p in np.nonzero(rng.random(len(b)) < rate)[0]:
        if any(lo <= p < hi for lo, hi in keep) or b[p] not in "ACGT":
            continue
        b[p] = "ACGT"[("ACGT".index(b[p]) + 1 + int(rng.integers(3))) % 4]
    return "".join(b)


def _case(cid, decision, samples, expect=None, **claim):
    samples = [list(s) if isinstance(s, (list, tuple)) else [s] for s in samples]
    c = dict(id=cid, decision=decision, samples=samples, claim=claim)
    T, nsep = text_of(c)
    e = derive(T, nsep)
    e.update(expect or {})
    if e.get("text_round") == 1:      # :2937-2958  the packed text is made whenever the round runs; its work division follows the hint
        e.setdefault("packed_text", 1)
        e.setdefault("text_mode", text_mode_of(e))
    c["expect"] = e
    claim.setdefault("n", len(T))
    return c


def _pair_to_n(a, b, n):
    """a pair of sequences -> the second trimmed so that the text holds exactly n positions"""
    need = n - 2 - len(a)
    assert 0 < need <= len(b), (len(a), len(b), n)
    return [a, b[:need]]


def d1_cases():
    """D1  the counting build, n <= TINY_N / 2 (:2505): six classes at n = 1024 | 1025, three samples at 1024, n = 2 and 9"""
    out = []
    for n in (1024, 1025):
        rng = np.random.default_rng(1100 + n)
        la, lb = 511, n - 2 - 511
        base = _rnd(rng, 512)
        out.append(_case("D1_related_%d" % n, "D1", [base[:la], _snp(rng, base, 0.02)[:lb]], n=n))
        out.append(_case("D1_identical_%d" % n, "D1", [base[:la], base[:lb]], n=n))      # (1025: the second sample one base longer)
        out.append(_case("D1_homopolymer_%d" % n, "D1", ["A" * 512, "A" * (n - 2 - 512)], n=n))
        s = base[:100] + "N" * 9 + base[109:300].lower() + base[300:la]
        out.append(_case("D1_n_lower_%d" % n, "D1", [s, _snp(rng, base, 0.02)[:100] + "N" * 9 + base[109:lb]], n=n))
        contigs = [base[70 * k:70 * k + 69] for k in range(7)]                      # 7 x 69 + 7 separators = 490
        out.append(_case("D1_contigs_%d" % n, "D1", [contigs, _snp(rng, base + base, 0.02)[:n - 490 - 1]], n=n))
        letters = "".join(chr(c) for c in range(33, 127) if chr(c) not in "$N")[:88]      # '!', '"', '#' sort below '$'
        a = _rnd(rng, la, letters)
        out.append(_case("D1_88_letters_%d" % n, "D1", [a, (a[:200] + _rnd(rng, lb, letters))[:lb]], below_sep=3, n=n))
    rng = np.random.default_rng(1199)
    base = _rnd(rng, 341)
    out.append(_case("D1_three_1024", "D1", [base[:340], _snp(rng, base, 0.03)[:340], _snp(rng, base, 0.03)[:341]], n=1024))
    out.append(_case("D1_single_2", "D1", ["A"], n=2))
    out.append(_case("D1_pair_9", "D1", ["ACGT", "ACG"], n=9))
    return out


def d2_cases():
    """D2  "past the end" spells the separator (:2546): DNA on; a byte below '$' off; two letters; one letter (sigma = 2); an empty
    sequence (two separators in a row) off -- each at n about 3000 and at n <= 1024, where the counting build does not ask"""
    out = []
    for tag, L in (("3000", 1500), ("small", 400)):
        rng = np.random.default_rng(1200 + L)
        base = _rnd(rng, L)
        var = _snp(rng, base, 0.01)
        out.append(_case("D2_dna_%s" % tag, "D2", [base, var], below_sep=0))
        low = base[:L // 3] + "!" + base[L // 3 + 1:]
        low2 = var[:L // 2] + "#" + var[L // 2 + 1:]
        out.append(_case("D2_below_sep_%s" % tag, "D2", [low, low2], below_sep=2))
        two = _rnd(rng, L, "AC")
        out.append(_case("D2_two_letters_%s" % tag, "D2", [two, _snp(rng, two, 0.01)], below_sep=0))
        out.append(_case("D2_one_letter_%s" % tag, "D2", ["A" * L, "A" * (L - 3)], below_sep=0))
        out.append(_case("D2_empty_sequence_%s" % tag, "D2", [[base[:L // 2], "", base[L // 2:]], var], below_sep=0, empty=1))
    return out


def d4_cases():
    """D4  the hint knows HINT_K = 16 samples (:2618-2626), D5  the twins of the second of TWO samples leave (:2666)"""
    out = []
    for k in (2, 3, 16, 17):
        fam = [g.decode() for g in synth.genomes(600, k, seed=1400 + k, snp=0.01)]
        e = {}
        if k > 2:
            e = dict(text_round=1)      # k homologues share their K symbols and no kernel in front of the text round orders three
        out.append(_case("D4_family_%d" % k, "D4", fam, e))
    rng = np.random.default_rng(1401)
    out.append(_case("D4_single_1500", "D4", [_rnd(rng, 1500)]))
    base = _rnd(rng, 1500)
    out.append(_case("D5_second_of_one_base", "D5", [base, "G"], n=1503))      # n = D + 2: :2666 asks n > D + 1
    out.append(_case("D5_second_empty", "D5", [base, ""], empty=1, n=1502))     # n = D + 1: the other side
    return out


def d6_cases():
    """D6  piecewise diagonals (:2689): n >= 4096, tried when 30 % of the second sample stays, kept when a fifth more leaves (:2713)"""
    out = []
    ind = [g.decode() for g in synth.genomes(2100, 2, seed=1601, snp=0.02, indelfrac=0.5)]
    for n in (4095, 4096):
        out.append(_case("D6_indel_%d" % n, "D6", _pair_to_n(ind[0][:2040], ind[1], n), dict(diag_table_tried=int(n >= 4096)), n=n))
    snp = [g.decode() for g in synth.genomes(2999, 2, seed=1602, snp=0.01)]
    out.append(_case("D6_snp_6000", "D6", snp, dict(diag_table_tried=0, diag_table_kept=0), n=6000))
    rng = np.random.default_rng(1603)
    base = _rnd(rng, 3999)
    out.append(_case("D6_unrelated_8000", "D6", [base, _rnd(rng, 3999)], dict(diag_table_tried=1, diag_table_kept=0), n=8000))
    # halves swapped: every seed of the first 2000 bases votes dd = +1999, every seed of the rest -2000 -- tile by tile, on both sides of a
    # pair, so the links hold (:195-246) and the table lets the twins leave that the fixed diagonal keeps
    out.append(_case("D6_rearranged_8000", "D6", [base, _snp(rng, base[2000:] + base[:2000], 0.01)], dict(diag_table_tried=1, diag_table_kept=1), n=8000))
    ind8 = [g.decode() for g in synth.genomes(4100, 2, seed=1604, snp=0.02, indelfrac=0.5)]
    out.append(_case("D6_indel_8000", "D6", _pair_to_n(ind8[0][:3999], ind8[1], 8000), dict(diag_table_tried=1, diag_table_kept=1), n=8000))
    return out


def d7_cases():
    """D7  group sizes: SMALL_GROUP 8, MEDIUM_GROUP 64 (:1802, :1523): exactly c copies of one random 120-mer"""
    out = []
    for c in (2, 4, 5, 8, 9, 64, 65):
        rng = np.random.default_rng(1700 + c)
        kmer = _rnd(rng, 120)
        s = "".join(_rnd(rng, 30) + kmer for _ in range(c)) + _rnd(rng, 30)
        e = dict(text_round=1, text_big=int(c > MEDIUM_GROUP), defer_max="<=cap")
        if c <= 4:
            e["defer_max"] = ">0"       # :1891-1918  groups of up to four that no hint orders go to the work list
        if c > MEDIUM_GROUP:            # the radix path orders 2 K symbols: the copies stay tied, the rounds go on by ranks (:3005, :3047)
            e.update(doubling_rounds=">0", slow_class=1, text_jump=0)
        else:
            e.update(doubling_rounds=0, slow_class=0, text_jump=0, fused_final=1, far_ran=0)
        out.append(_case("D7_copies_%d" % c, "D7", [s, _rnd(rng, max(200, 1100 - len(s)))], e, copies=(kmer, c)))      # (above the counting build's 1024)
    for c in (8, 9, 16, 17):
        rng = np.random.default_rng(1750 + c)
        kmer = _rnd(rng, 120)
        fam = []
        for k in range(c):
            at = 20 + 17 * k
            fam.append(_rnd(rng, at) + kmer + _rnd(rng, 400 - at))
        e = dict(text_round=1, text_big=0, doubling_rounds=0, slow_class=0, text_jump=0, fused_final=1, far_ran=0, defer_max="<=cap")
        out.append(_case("D7_spread_%d" % c, "D7", fam, e, copies=(kmer, c)))
    return out


def d8_cases():
    """D8  n > 2 TEXT_LIM (:3047 classes, :3061 jump): ties beyond 4096 symbols at n = 8192 | 8193"""
    out = []
    for n in (8192, 8193):
        big = n > 2 * TEXT_LIM
        # one group of thousands: the radix path in the text round (text_big), so no jump on either side; classes above 8192
        e = dict(text_round=1, text_big=1, text_jump=0, slow_class=int(big), doubling_rounds=">0")
        out.append(_case("D8_homopolymer_%d" % n, "D8", ["A" * 4096, "A" * (n - 2 - 4096)], e, n=n))
        rng = np.random.default_rng(1800 + n)
        unit = "ACGGTCA"
        t = unit * 600
        out.append(_case("D8_tandem_%d" % n, "D8", [t[:4096], t[3:3 + n - 2 - 4096]], e, n=n))
        # identical but for the length: no group above two, every pair of partners is left tied by the text round (:1910), the jump is taken above 8192
        base = _rnd(rng, 4096)
        e2 = dict(text_round=1, text_big=0, text_jump=int(big), slow_class=0, far_ran=1, doubling_rounds=0, fused_final=1)
        out.append(_case("D8_identical_%d" % n, "D8", [base, base[:n - 2 - 4096]], e2, n=n))
    return out


def d9_cases():
    """D9  the text round's compare (:1448 / :1408): it starts at offset K and goes on in whole steps of 128 (packed) or 32 bytes while the
    offset is below TEXT_LIM, so it sees a difference at offsets below K + 4096 (K < 32).  Two copies of an element of E bases inside one
    sample, different bases in front of and behind them: finished by the text round for E = 4095, 4096, 4097 and K + 4095, left to the
    rounds by ranks from E = K + 4096 on"""
    out = []

    def two_copies(E, seed):
        rng = np.random.default_rng(seed)
        elem = _rnd(rng, E)
        return ["C" + _rnd(rng, 40) + "A" + elem + "C" + _rnd(rng, 40) + "G" + elem + "T" + _rnd(rng, 40), _rnd(rng, 300)]
    K = derive(*text_of(dict(samples=[[s] for s in two_copies(4096, 1900)])))["K"]
    assert 2 <= K < 32
    for E in (4095, 4096, 4097, K + 4095, K + 4096, K + 4160):
        s = two_copies(E, 1900)
        assert derive(*text_of(dict(samples=[[x] for x in s])))["K"] == K
        if E < K + TEXT_LIM:
            e = dict(text_round=1, text_big=0, doubling_rounds=0, text_jump=0, far_ran=0, fused_final=1, defer_max=">0")
        else:       # tied after the text round: jump (n > 8192, no big group), the far round looks (two samples), then ranks
            e = dict(text_round=1, text_big=0, doubling_rounds=">0", text_jump=1, far_ran=1, fused_final=1, lcp_list_overflow=0, defer_max=">0")
        out.append(_case("D9_copies_%d" % E, "D9", s, e, maxlcp=E))
    for L in (4095, 4096, 4097):
        rng = np.random.default_rng(1950)
        base = _rnd(rng, L)
        e = dict(text_round=1, text_big=0, far_ran=1, nd_table=0, doubling_rounds=0, text_jump=int(2 * L + 2 > 2 * TEXT_LIM), fused_final=1)
        out.append(_case("D9_partners_%d" % L, "D9", [base, base], e, maxlcp=L, n=2 * L + 2))
    return out


def d10_cases():
    """D10  far_cmp looks at FAR_MAXIT = 64 windows (:1991): identical samples with j single N more than 4096 bases apart.  A pair of
    partners in front of the first N meets one exception mark per N, then the separator: j + 1 windows.  j = 63: decided in the last
    one; j = 64: left to the rounds by ranks"""
    out = []
    for j in (FAR_MAXIT - 1, FAR_MAXIT):
        rng = np.random.default_rng(2000)
        b = list(_rnd(rng, 4200 * (FAR_MAXIT + 1)))
        for k in range(j):
            b[4150 + 4200 * k] = "N"
        s = "".join(b)
        e = dict(text_round=1, far_ran=1, nd_table=0, text_big=0, text_jump=1, doubling_rounds=0 if j < FAR_MAXIT else ">0", fused_final=1)
        out.append(_case("D10_marks_%d" % j, "D10", [s, s], e, ncount=2 * j))
    return out


def d11_cases():
    """D11  k_lcp_list gives up after LL_MAX_STEPS x 512 = 2^21 bytes (:2124-2142): two copies of an element of E bases"""
    out = []
    for E in (LL_LIMIT - 1, LL_LIMIT):
        rng = np.random.default_rng(2100)
        elem = synth.genomes(E, 1, seed=2100)[0].decode()
        s = "C" + _rnd(rng, 50) + "A" + elem + "C" + _rnd(rng, 50) + "G" + elem + "T" + _rnd(rng, 50)
        over = int(E >= LL_LIMIT)
        e = dict(text_round=1, text_big=0, text_jump=1, far_ran=1, doubling_rounds=">0", lcp_list_overflow=over, fused_final=1 - over)
        out.append(_case("D11_copies_%s" % ("2p21" if over else "2p21m1"), "D11", [s, _rnd(rng, 1000)], e, maxlcp=E, large=1))
    return out


def d12_cases():
    """D12  the packed text's flag per PK_BLOCK = 128 positions (:1392, :1451): one N, one lower-case base or one contig border at text
    position 127, 128, 129 or in the text's last block, inside a stretch where the samples agree for more than 200 bases on either side
    (fewer behind it in the last block).  A pair of partners that the hint cannot order is left to k_far_twins, which reads the text
    itself (:1910, :2004); with three samples nothing but the packed compare orders the homologues across the character"""
    out = []

    def put(s, at, what):
        if what == "N":
            return s[:at] + "N" + s[at + 1:]
        if what == "lower":
            return s[:at] + s[at].lower() + s[at + 1:]
        return [s[:at], s[at + 1:]]
    for count in (2, 3):
        for what in ("N", "lower", "border"):
            for where in (127, 128, 129, "last"):
                for who in ("one", "all"):      # one: the comparison ends at the character; all: every sample has it there, the comparison crosses it
                    rng = np.random.default_rng(2200 + count)
                    L = 3000 if count == 2 else 2000
                    base = _rnd(rng, L)
                    k_at = 0 if where != "last" else count - 1                    # the sample whose character sits at the named text position
                    at = where if where != "last" else L - 60                      # offset inside the sample
                    fam = [base] + [_snp(rng, base, 0.004, keep=[(0, 400), (L - 330, L)]) for _ in range(count - 1)]
                    fam = [put(s, at, what) if (who == "all" or k == k_at) else s for k, s in enumerate(fam)]
                    pos = at + (L + 1) * k_at                                      # text position of that character
                    e = dict(text_round=1, text_big=0, doubling_rounds=0, fused_final=1)
                    if count == 2:
                        e.update(far_ran=1)
                    out.append(_case("D12_%s_%s_%s_%d" % (what, where, who, count), "D12", fam, e, special=(pos, what), last=int(where == "last")))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    cs = d1_cases() + d2_cases() + d4_cases() + d6_cases() + d7_cases() + d8_cases() + d9_cases() + d10_cases() + d12_cases()
    assert len({c["id"] for c in cs}) == len(cs)
    return tuple(cs)


LARGE_IDS = ("D11_copies_2p21m1", "D11_copies_2p21")      # 4.2 x 10^6 positions each: made when a test asks for them


@functools.lru_cache(maxsize=None)
def large_cases():
    cs = tuple(d11_cases())
    assert tuple(c["id"] for c in cs) == LARGE_IDS
    return cs


def small_ids():
    return [c["id"] for c in small_cases()]


def case(cid):
    return next(c for c in (large_cases() if cid in LARGE_IDS else small_cases()) if c["id"] == cid)
