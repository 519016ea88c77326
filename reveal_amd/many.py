"""Many small alignments in one call (include/reveal_amd.h "many small alignments", csrc/rv_many.hip).

`reveal refine --method reveal_rem` calls `rem.align` once per bubble (reveal/refine.py:220-229).  `align_many` takes the
sequences of many bubbles at once: the pair jobs of at most 2048 ranks share their kernel launches (one index build per size
class with the text in LDS, one launch of the leaf kernel for every job's recursion), every other job runs the ordinary way
inside the same call.  The built-in picker (as `index.align_builtin`) unless `picker=` is given; no CPU fallback.

`align_many(.., picker=schemes.PickerArgs(..))` (`Batch.set_picker`) aligns every job with the reference's default picker instead
(schemes.graphmumpicker: trim the overlaps, chain, split on the largest match of the chain) -- what `reveal refine` gets from
`rem.align` for a bubble, and what `index.set_picker(args)` + `align_builtin` give a stand-alone index of the job.  The shared
classes below all finish with built-in-picker kernels, so with a picker set none of them takes a job, whatever its switch says:
without one of the chain switches the jobs run the ordinary way with the picker in host C++ (`info["ordinary"]`).  With the switch RV_MANY_CHAIN on
(`align_many(.., chain=True)`, `Batch.option("RV_MANY_CHAIN", 1)` or the environment variable; off by default, and it means
something with a picker only) the pair jobs of at most 2048 ranks share their launches all the same, finished by the leaf kernel
with the picker's decision for two samples as its pick stage (csrc/rv_leaf_chain.hip), when the options leave the picker nothing a
workgroup cannot do: trim on, minlength > 0, weights 0 .. 65536, a seedsize no match can reach and a maxmums that cannot bite
(`takes_shared_launch(.., picker=args, chain=True)`).  The results do not depend on the switch.  `PickerArgs.maxsize` and
`.maxdepth` are not taken (the native picker has neither).

With the switch RV_MANY_CHAIN_MULTI on (`align_many(.., chain_multi=True)`, `Batch.option("RV_MANY_CHAIN_MULTI", 1)` or the environment
variable; off by default, independent of RV_MANY_CHAIN and RV_MANY_MULTI, and it means something with a picker only) the jobs of 3 .. 16
sequences and at most 2048 ranks share their launches under the picker as well: layout and index build of RV_MANY_MULTI and one launch of the
multi-sample leaf kernel with the whole picker as its pick stage (csrc/rv_leaf_multi_chain.hip: matches on sample subsets, `segment`, trim and
chain over k paths, a three-way split with a `rest` child), when trim is on, minlength > 0, the weights are 0 .. 1024, no match can reach
seedsize and maxmums is at least the job's ranks (`takes_shared_launch(.., picker=args, chain_multi=True)`).  A job the kernel cannot finish
(where the reference's trim_overlap raises) is flagged and runs the ordinary way
inside the same call.  The results do not depend on the switch.

With the switch RV_MANY_CHAIN_WIDE on (`align_many(.., chain_wide=True)`, `Batch.option("RV_MANY_CHAIN_WIDE", 1)` or the environment variable; off by
default, independent of every other switch, and it means something with a picker only) the jobs of 17 .. 64 sequences and at most 2048 ranks share
their launches under the picker too, in rounds of their own: layout and index build of the small RV_MANY_WIDE rounds and one launch of the 64-sample
form of the same kernel (a wavefront holds one predecessor of a chain step, a lane per path; the gap costs over up to 64 paths by reductions over the
wavefront), under the same conditions (`takes_shared_launch(.., picker=args, chain_wide=True)`); flagged jobs as above.  Under a picker the jobs of
more than 64 sequences always run the ordinary way.  The results do not depend on the switch.

With the switch RV_MANY_CHAIN_LARGE on (`align_many(.., chain_large=True)`, `Batch.option("RV_MANY_CHAIN_LARGE", 1)` or the environment variable; off by
default, independent of every other switch, and it means something with a picker only) the pair jobs of 2049 .. min(RV_MANY_LARGE_MAX, 2^17) ranks share
their launches under the picker too, in rounds of their own: layout, index build and level pipeline of the RV_MANY_LARGE rounds, with the pick of every
sub-index above 2048 ranks made on the device by a kernel that takes the picker's decision for two samples (csrc/rv_pick_chain.hip: a wavefront per
sub-index, up to 1024 candidates) in place of the longest-match kernel, and the sub-indices below finished by the chain form of the leaf kernel -- when
trim is on, minlength > 0, the weights are 0 .. 1024, no match can reach seedsize and maxmums is at least the shorter sequence
(`takes_shared_launch(.., picker=args, chain_large=True)`): `rem.align`'s defaults admit every bubble `reveal refine` produces.  A call with fewer than
RV_MANY_CHAIN_LARGE_MIN such jobs (default 4) leaves them on the ordinary path; a job a kernel of any level cannot finish (more candidates than the cap,
or where the reference's trim_overlap raises) is flagged and runs the ordinary way inside the same call.  The results do not depend on the switch.

With the switch RV_MANY_CHAIN_LARGE_MULTI on (`align_many(.., chain_large_multi=True)`, `Batch.option("RV_MANY_CHAIN_LARGE_MULTI", 1)` or the environment
variable; off by default, independent of every other switch, and it means something with a picker only) the jobs of 3 .. 16 sequences and 2049 ..
min(RV_MANY_LARGE_MAX, 2^17) ranks share their launches under the picker too, in rounds of their own: layout, index build and level pipeline of the
RV_MANY_LARGE_MULTI rounds, the scan of every level unfiltered, and the pick of every sub-index made on the device by a kernel that takes the picker's
decision for up to 16 samples (csrc/rv_pick_multi_chain.hip: a wavefront per sub-index, up to 512 candidates; a match of a sample subset leaves a `rest`
child) in place of the longest-match kernels -- when trim is on, minlength > 0, the weights are 0 .. 512, no match can reach seedsize and maxmums is at
least the job's ranks (`takes_shared_launch(.., picker=args, chain_large_multi=True)`): `rem.align`'s default maxmums of 10 000 admits jobs of up to
10 000 ranks only.  A call with fewer than RV_MANY_CHAIN_LARGE_MULTI_MIN such jobs (default 4) leaves them on the ordinary path; a flagged job runs the
ordinary way inside the same call.  The results do not depend on the switch.

With the switch RV_MANY_CHAIN_WIDE_LARGE on (`align_many(.., chain_wide_large=True)`, `Batch.option("RV_MANY_CHAIN_WIDE_LARGE", 1)` or the environment
variable; off by default, independent of every other switch, and it means something with a picker only) the jobs of 17 .. 64 sequences and 2049 ..
min(RV_MANY_LARGE_MAX, 2^17) ranks -- the bubbles of a graph of 25 or 100 genomes with alleles above about 60 bases -- share their launches under the
picker too, in rounds of their own: the rounds of RV_MANY_CHAIN_LARGE_MULTI with up to 64 samples, the pick of every sub-index made by the 64-sample form
of the same kernel (a lane per sample, one predecessor a chain step, 64-bit sample sets, up to 256 candidates a sub-index) -- when trim is on,
minlength > 0, the weights are 0 .. 128, no match can reach seedsize and maxmums is at least the job's ranks
(`takes_shared_launch(.., picker=args, chain_wide_large=True)`).  A call with fewer than RV_MANY_CHAIN_WIDE_LARGE_MIN such jobs (default 2) leaves them on
the ordinary path; a flagged job (more than 256 candidates in one sub-index, or where the reference's trim_overlap raises) runs the ordinary way inside
the same call.  The results do not depend on the switch.

Jobs of three and more sequences -- a bubble of a graph of N genomes carries up to N -- run the ordinary way unless the switch
RV_MANY_MULTI is on (`align_many(.., multi=True)`, `Batch.option("RV_MANY_MULTI", 1)` or the environment variable; off by default).
With it the jobs of 3 .. 16 sequences and at most 2048 ranks share their launches as well, in rounds of their own: every job
contiguous in the round's text, the same index build, and one launch of a leaf kernel that runs the whole recursion of a job in
one workgroup (csrc/rv_leaf_multi.hip).  The results do not depend on the switch.

Pair jobs above 2048 ranks -- `reveal refine` takes bubbles with alleles of up to 10 kbp, 20 000 ranks -- run the ordinary way unless the
switch RV_MANY_LARGE is on (`align_many(.., large=True)`, `Batch.option("RV_MANY_LARGE", 1)` or the environment variable; off by default).
With it the pair jobs of 2049 .. RV_MANY_LARGE_MAX ranks (default 2^17) share their launches too, in rounds of their own: the pair layout of
the small jobs, the index of every job of a round built at once by a segmented prefix doubling in device memory
(csrc/rv_many_large.hip), and the level pipeline of the recursion over all of them together.  A call with fewer than RV_MANY_LARGE_MIN
such jobs (default 4) leaves them on the ordinary path.

Jobs of three and more sequences above 2048 ranks -- a bubble of a graph of more than two genomes with alleles above about 700 bases -- run the
ordinary way unless the switch RV_MANY_LARGE_MULTI is on (`align_many(.., large_multi=True)`, `Batch.option("RV_MANY_LARGE_MULTI", 1)` or the
environment variable; off by default).  With it the jobs of 3 .. 16 sequences and 2049 .. RV_MANY_LARGE_MAX ranks share their launches too, in
rounds of their own that may mix jobs of different k: the round's text is sample-major (`sample_major_layout`: sample q holds the q-th sequence
of every job that has one), the same segmented prefix doubling builds every job's index from its job-local text, and the level pipeline for
more than two samples finishes all of them together.  A call with fewer than RV_MANY_LARGE_MULTI_MIN such jobs (default 16, counted on their
own) leaves them on the ordinary path.  With all three switches on, every
clean job of 2 .. 16 sequences up to RV_MANY_LARGE_MAX ranks that fits a round goes through shared launches -- in a call that holds at least
RV_MANY_LARGE_MIN pair jobs and RV_MANY_LARGE_MULTI_MIN jobs of three and more sequences above 2048 ranks, where it has any.
The results do not depend on these switches either.

Jobs of more than 16 sequences -- every bubble of a graph of 25 or 100 genomes refined without --uniqueonly -- run the ordinary way unless
the switch RV_MANY_WIDE is on (`align_many(.., wide=True)`, `Batch.option("RV_MANY_WIDE", 1)` or the environment variable; off by default,
independent of the other switches).  With it the clean jobs of 17 .. 64 sequences share their launches too, in rounds of their own: up to
2048 ranks the layout and the index build of RV_MANY_MULTI and one launch of the 64-sample form of the leaf kernel; at 2049 ..
RV_MANY_LARGE_MAX ranks the sample-major rounds of RV_MANY_LARGE_MULTI with up to 64 samples, in a call with at least
RV_MANY_WIDE_LARGE_MIN such jobs (default 8, counted on their own).  64 is the limit because a lane of a wavefront owns a sample in the
leaf kernel, the sample id has six bits of its per-position byte, and the level pipeline's scan keeps a one-word census up to 64 samples.
Jobs of more than 64 sequences always run the ordinary way.  The results do not depend on this switch either.

`mums_many(jobs, minlength, minn, kind)` (`Batch.scan` + `Batch.matches`) gives the MUM / multi-MUM LISTS of the jobs instead of a finished recursion:
what `index.getmums` / `index.getmultimums` give a stand-alone index of each job, in its coordinates and in the reference's emission order -- for a
caller who brings a picker of their own, or for `reveal chain --recurse`, which builds an index per gap for exactly these two calls.  Every job of
2 .. 64 sequences, at most 2048 ranks and no NUL byte shares its launches, with no switch (`takes_shared_scan`): the index build above, then a count
pass, an exclusive sum and a write pass flat over the ranks of the round (csrc/rv_many_scan.hip) into CSR arrays.  Every other job runs the ordinary way
inside the call -- jobs above 2048 ranks too, unless the switch RV_MANY_SCAN_LARGE is on (`mums_many(.., large=True)`, `Batch.option("RV_MANY_SCAN_LARGE", 1)`
or the environment variable; off by default).  With it the jobs of 2 .. 64 sequences, 2049 .. RV_MANY_LARGE_MAX ranks (default 2^17) and no NUL byte share
their launches too (`takes_shared_scan(.., large=True)`), in rounds of their own but of one kind for every k: each job contiguous in the round's text as
for the small ones, the index of every job of the round built at once by the segmented prefix doubling on that text in place
(csrc/rv_many_large.hip rv_many_large_build_c), then the same count pass, sum and write pass.  A call with fewer than RV_MANY_SCAN_LARGE_MIN such jobs
(default 4: measured, one or two such jobs lose or tie against the ordinary path, four win) leaves them on the ordinary path, and so does a job larger than a round (RV_MANY_ROUND, 2^26 ranks at most).  The lists
do not depend on the switch.  1000 pairs of 2 x (1100 .. 9999) bases: 17.6 ms against 365 ms with the switch off (20.8 x); 1000 jobs of 3 / 8 / 32 sequences at
2100 .. 30 000 ranks: 14.3 x / 13.6 x / 6.3 x (profiles/many_mums_large.txt).  A scan leaves jobs and text untouched, so `scan` and `run` may follow
each other on one Batch; the live result is the last call's (`text` / `anchors` after a scan and `matches` after a run raise `error`).
"""
import ctypes
import os

import numpy as np

from . import _lib

LEAF_RANKS = 2048          # RV_LEAF_N: a job of sum of lengths + k ranks up to this goes through the shared launches
MULTI_KMAX = 16            # RV_MANY_KMAX: sequences of a job the shared launches take with RV_MANY_MULTI
WIDE_KMAX = 64             # RV_MANY_WIDE_KMAX: sequences of a job the shared launches take with RV_MANY_WIDE (17 .. 64)
WIDE_LARGE_MIN = 8         # default of RV_MANY_WIDE_LARGE_MIN: fewer jobs of 17 .. 64 sequences above 2048 ranks in a call stay ordinary
CHAIN_WMAX = 65536         # RV_LEAF_CHAIN_WMAX: weights up to this keep the chain's scores in 32 bits on the device
CHAIN_MULTI_WMAX = 1024    # RV_LEAF_MCHAIN_WMAX: the same for chains over up to 16 paths (gain factor n (n - 1) / 2 <= 120) and over up to 64 (csrc/rv_leaf_multi_chain.hip)
LARGE_MAX = 1 << 17        # default of RV_MANY_LARGE_MAX: ranks of the largest pair job the shared launches take with RV_MANY_LARGE
CHAIN_LARGE_RANKS = 1 << 17  # RV_PICK_CHAIN_RANKS: ranks of the largest pair job RV_MANY_CHAIN_LARGE takes, whatever RV_MANY_LARGE_MAX says (17-bit positions)
CHAIN_LARGE_MULTI_WMAX = 512  # RV_PICK_MCHAIN_WMAX: weights up to this keep the chain's scores in 32 bits over up to 16 paths of a job of 2^17 ranks (csrc/rv_pick_multi_chain.hip)
CHAIN_LARGE_MULTI_MIN = 4  # default of RV_MANY_CHAIN_LARGE_MULTI_MIN: fewer admitted jobs of 3 .. 16 sequences above 2048 ranks in a call under a picker stay ordinary
CHAIN_WIDE_LARGE_WMAX = 128  # RV_PICK_WCHAIN_WMAX: the same over up to 64 paths (2016 pairs) of a job of 2^17 ranks: 256 does not hold (csrc/rv_pick_multi_chain.hip)
CHAIN_WIDE_LARGE_MIN = 2   # default of RV_MANY_CHAIN_WIDE_LARGE_MIN: fewer admitted jobs of 17 .. 64 sequences above 2048 ranks in a call under a picker stay ordinary
SCAN_LARGE_MIN = 4         # default of RV_MANY_SCAN_LARGE_MIN: fewer admitted jobs above 2048 ranks in a call of mums_many with RV_MANY_SCAN_LARGE stay ordinary
SCAN_ROUND_RANKS = 1 << 26  # RV_MANY_SCAN_RANKS: ranks of the largest round of a scan, whatever RV_MANY_ROUND says
CHAIN_LARGE_MIN = 4        # default of RV_MANY_CHAIN_LARGE_MIN: fewer admitted pair jobs above 2048 ranks in a call under a picker stay ordinary
SCAN_KINDS = {"mums": 0, "multimums": 1, "auto": 2}      # rv_many_scan's kind: getmums, getmultimums, getmums for pair jobs and getmultimums for the rest


class error(Exception):
    pass


def job_sequences(job, toupper=True):
    """a job as given -- a list of (name, seq) or of plain sequences (str / bytes) -> list of bytes; raises `error` for a job
    the library would refuse (fewer than two sequences, an empty sequence)"""
    if isinstance(job, (str, bytes, bytearray)) or not hasattr(job, "__len__"):
        raise error("a job is a list of sequences or of (name, sequence) pairs")
    seqs = []
    for item in job:
        s = item[1] if isinstance(item, (tuple, list)) else item
        if isinstance(s, str):
            s = s.encode("latin-1")
        elif isinstance(s, (bytes, bytearray)):
            s = bytes(s)
        else:
            raise error("a sequence is a str or bytes, not %s" % type(s).__name__)
        seqs.append(s.upper() if toupper else s)
    if len(seqs) < 2:
        raise error("a job needs at least two sequences (%d given)" % len(seqs))
    for k, s in enumerate(seqs):
        if len(s) == 0:
            raise error("sequence %d of the job is empty" % k)
    return seqs


def picker_struct(args):
    """a schemes.PickerArgs -> the C ABI's rv_picker_args; raises `error` for what the native picker does not take (maxsize, maxdepth, an unknown
    gap cost model) -- before anything asks the library for a device"""
    from . import schemes
    if args.maxsize is not None or args.maxdepth is not None:
        raise error("the native picker does not take --maxbubblesize / maxdepth")
    if args.gcmodel not in schemes.GCMODELS:
        raise error("unknown gap cost model %r (%s)" % (args.gcmodel, ", ".join(sorted(schemes.GCMODELS))))
    return schemes._RvPickerArgs(int(args.wscore), int(args.wpen), int(args.maxmums or 0), int(args.seedsize or 0), schemes.GCMODELS[args.gcmodel],
                                 1 if args.trim else 0, float(args.pcutoff))


# csrc/rv_many.hip many_classes row by row, in its order: (under a picker, k from, k to, above LEAF_RANKS, switch -- the keyword of takes_shared_launch and
# align_many, None: no switch --, weight cap, maxmums against the job's ranks and not the shortest sequence); the last two mean something under a picker only
CLASSES = (
    (False, 2, 2, False, None, None, False),
    (True, 2, 2, False, "chain", CHAIN_WMAX, False),
    (True, 3, MULTI_KMAX, False, "chain_multi", CHAIN_MULTI_WMAX, True),
    (True, MULTI_KMAX + 1, WIDE_KMAX, False, "chain_wide", CHAIN_MULTI_WMAX, True),
    (True, 2, 2, True, "chain_large", CHAIN_MULTI_WMAX, False),
    (True, 3, MULTI_KMAX, True, "chain_large_multi", CHAIN_LARGE_MULTI_WMAX, True),
    (True, MULTI_KMAX + 1, WIDE_KMAX, True, "chain_wide_large", CHAIN_WIDE_LARGE_WMAX, True),
    (False, 2, 2, True, "large", None, False),
    (False, 3, MULTI_KMAX, False, "multi", None, False),
    (False, 3, MULTI_KMAX, True, "large_multi", None, False),
    (False, MULTI_KMAX + 1, WIDE_KMAX, False, "wide", None, False),
    (False, MULTI_KMAX + 1, WIDE_KMAX, True, "wide", None, False),
)
SWITCHES = dict(chain="RV_MANY_CHAIN", chain_multi="RV_MANY_CHAIN_MULTI", chain_wide="RV_MANY_CHAIN_WIDE", chain_large="RV_MANY_CHAIN_LARGE",
                chain_large_multi="RV_MANY_CHAIN_LARGE_MULTI", chain_wide_large="RV_MANY_CHAIN_WIDE_LARGE", multi="RV_MANY_MULTI", large="RV_MANY_LARGE",
                large_multi="RV_MANY_LARGE_MULTI", wide="RV_MANY_WIDE")


def takes_shared_launch(seqs, multi=False, large=False, large_max=LARGE_MAX, large_multi=False, wide=False, picker=None, chain=False, minlength=20,
                        chain_multi=False, chain_wide=False, chain_large=False, chain_large_multi=False, chain_wide_large=False):
    """whether the library builds and finishes this job in the shared launches: whether it belongs to a row of CLASSES whose switch is on -- the rule
    csrc/rv_many.hip many_class_admits states once for every row of its table many_classes.  multi, large, large_multi, wide, chain, chain_multi,
    chain_wide, chain_large, chain_large_multi, chain_wide_large: with that row's switch (SWITCHES) on; large_max: RV_MANY_LARGE_MAX, the ranks of the
    largest job of a row above 2048 ranks (under a picker min(large_max, 2^17)); picker: a schemes.PickerArgs -- with the reference's default picker set
    (the rows of the built-in picker then take nothing, and the chain switches mean nothing without one); minlength: of the run.  Under a picker a row
    takes a job when trim is on, minlength > 0, the weights are 0 .. the row's cap (65536, 1024, 512 or 128), no sequence reaches seedsize, and maxmums
    is at least the shorter sequence (pairs) or the job's ranks.  The rows above 2048 ranks take their jobs in a call with at least RV_MANY_*_MIN of
    them and with rounds that hold the job; this function does not know the call."""
    k = len(seqs)
    lens = [len(s) for s in seqs]
    ranks = sum(lens) + k
    if any(b"\0" in s for s in seqs):
        return False
    on = dict(multi=multi, large=large, large_multi=large_multi, wide=wide, chain=chain, chain_multi=chain_multi, chain_wide=chain_wide,
              chain_large=chain_large, chain_large_multi=chain_large_multi, chain_wide_large=chain_wide_large)
    A = picker_struct(picker) if picker is not None else None
    for pk, kmin, kmax, above, switch, wmax, by_ranks in CLASSES:
        if pk != (A is not None) or not kmin <= k <= kmax or above != (ranks > LEAF_RANKS) or not (switch is None or on[switch]):
            continue
        if above and ranks > (min(int(large_max), CHAIN_LARGE_RANKS) if pk else large_max):
            continue
        return not pk or bool(A.trim and int(minlength) > 0 and 0 <= A.wscore <= wmax and 0 <= A.wpen <= wmax
                              and (A.seedsize <= 0 or A.seedsize > max(lens)) and (A.maxmums <= 0 or A.maxmums >= (ranks if by_ranks else min(lens))))
    return False


def takes_shared_scan(seqs, large=False, large_max=LARGE_MAX):
    """whether `mums_many` / `Batch.scan` build and scan this job in the shared launches (csrc/rv_many.hip many_scan_admits): 2 .. 64 sequences,
    at most 2048 ranks, no NUL byte, with no switch.  large: with RV_MANY_SCAN_LARGE on and RV_MANY_LARGE_MAX = large_max, the same jobs of 2049 ..
    large_max ranks as well (many_scan_large_admits) -- in a call with at least RV_MANY_SCAN_LARGE_MIN such jobs, and with rounds that hold the job
    (RV_MANY_ROUND, at most 2^26 ranks).  Every other job runs the ordinary way inside the call."""
    k = len(seqs)
    ranks = sum(len(s) for s in seqs) + k
    if not 2 <= k <= WIDE_KMAX or any(b"\0" in s for s in seqs):
        return False
    return ranks <= LEAF_RANKS or (bool(large) and ranks <= min(int(large_max), SCAN_ROUND_RANKS))


def shared_layout(pairs):
    """the shared text of pair jobs [(a, b), ..] in the given order: every first sequence, then every second one, a '$' behind
    each -> (text, a_begin[], b_begin[])"""
    text, abeg, bbeg = bytearray(), [], []
    for a, _ in pairs:
        abeg.append(len(text))
        text += a + b"$"
    for _, b in pairs:
        bbeg.append(len(text))
        text += b + b"$"
    return bytes(text), abeg, bbeg


def to_local(pos, side, abeg, bbeg, la):
    """position of the shared text inside job's sequence `side` -> stand-alone coordinate of the job's text `a$b$`"""
    return pos - abeg if side == 0 else pos - bbeg + la + 1


def to_shared(loc, abeg, bbeg, la):
    """stand-alone coordinate of `a$b$` -> (side, position of the shared text)"""
    return (0, abeg + loc) if loc <= la else (1, bbeg + loc - la - 1)


def sample_major_layout(jobs):
    """the shared text of jobs of several sequences [[s0, s1, ..], ..] in the given order, k mixed: sample q holds the q-th sequence of every
    job that has one, a '$' behind each -> (text, nsep, begins): nsep[q] = the '$' behind the last sequence of sample q, begins[j][q] = where
    sequence q of job j begins"""
    K = max(len(j) for j in jobs)
    text, nsep, begins = bytearray(), [], [[] for _ in jobs]
    for q in range(K):
        for j, seqs in enumerate(jobs):
            if q < len(seqs):
                begins[j].append(len(text))
                text += seqs[q] + b"$"
        nsep.append(len(text) - 1)
    return bytes(text), nsep, begins


def to_shared_k(loc, begins, lens):
    """stand-alone coordinate of the job's text `s0$s1$..` (begins, lens: of its sequences) -> (sequence, position of the shared text)"""
    at = 0
    for q, n in enumerate(lens):
        if loc <= at + n:
            return q, begins[q] + loc - at
        at += n + 1
    raise error("coordinate %d outside a job of %d ranks" % (loc, at))


def to_local_k(pos, q, begins, lens):
    """position of the shared text inside the job's sequence q (or on its '$') -> stand-alone coordinate of the job's text `s0$s1$..`"""
    return pos - begins[q] + sum(lens[:q]) + q


class Batch:
    """the C object behind align_many (rv_many_*): add jobs, run, read the results; clear() keeps the allocations"""

    def __init__(self, sa64=False, device=None):
        self._lib = _lib.get(sa64)
        self._dll = self._lib.dll
        self._m = self._dll.rv_many_new(_lib.device() if device is None else int(device))
        if not self._m:
            raise error(self._lib.err())
        self._lens = []
        for k in range(self._dll.rv_option_count()):      # RV_* switches of the environment, as a new index object applies them
            name = self._dll.rv_option_name(k).decode()
            v = os.environ.get(name)
            if v is not None:
                try:
                    iv = int(v) if v.strip() else 1
                except ValueError:
                    iv = 1
                self.option(name, iv)
        for name in ("RV_MANY_KEEP", "RV_MANY_ROUND", "RV_MANY_WAVE_MAX", "RV_MANY_MULTI", "RV_MANY_LARGE", "RV_MANY_LARGE_MAX", "RV_MANY_LARGE_MIN",
                     "RV_MANY_LARGE_MULTI", "RV_MANY_LARGE_MULTI_MIN", "RV_MANY_WIDE", "RV_MANY_WIDE_LARGE_MIN", "RV_MANY_CHAIN", "RV_MANY_CHAIN_MULTI", "RV_MANY_CHAIN_WIDE",
                     "RV_MANY_CHAIN_LARGE", "RV_MANY_CHAIN_LARGE_MIN", "RV_MANY_CHAIN_LARGE_MULTI", "RV_MANY_CHAIN_LARGE_MULTI_MIN",
                     "RV_MANY_CHAIN_WIDE_LARGE", "RV_MANY_CHAIN_WIDE_LARGE_MIN", "RV_MANY_SCAN_ORDINARY", "RV_MANY_SCAN_LARGE", "RV_MANY_SCAN_LARGE_MIN"):
            v = os.environ.get(name)
            if v is not None and v.strip():
                self.option(name, int(v))

    def __del__(self):
        m, self._m = getattr(self, "_m", None), None
        if m:
            self._dll.rv_many_free(m)

    def _fail(self):
        raise error(self._lib.err())

    def option(self, name, value=1):
        if self._dll.rv_many_option(self._m, name.encode(), int(value)) != 0:
            self._fail()

    def set_picker(self, args=None):
        """rv_many_set_picker: None = the built-in picker; a schemes.PickerArgs = the reference's default picker (schemes.graphmumpicker) with these
        options, for this and later runs (args.maxsize / maxdepth are not supported)"""
        if args is None:
            r = self._dll.rv_many_set_picker(self._m, 0, None)
        else:
            A = picker_struct(args)
            r = self._dll.rv_many_set_picker(self._m, 1, ctypes.byref(A))
        if r != 0:
            self._fail()

    def add(self, seqs):
        k = len(seqs)
        ptrs = (ctypes.c_char_p * k)(*seqs)
        lens = (ctypes.c_int64 * k)(*[len(s) for s in seqs])
        j = self._dll.rv_many_add(self._m, ptrs, lens, k)
        if j < 0:
            self._fail()
        self._lens.append(sum(len(s) for s in seqs) + k)
        return j

    def clear(self):
        if self._dll.rv_many_clear(self._m) != 0:
            self._fail()
        self._lens = []

    def info(self):
        o = (ctypes.c_int64 * 5)()
        self._dll.rv_many_info(self._m, o)
        return dict(jobs=int(o[0]), shared=int(o[1]), ordinary=int(o[2]), rounds=int(o[3]), launches=int(o[4]))

    def flagged(self):
        """-> {bit: jobs}: the jobs of the last run a round under a picker gave back to the ordinary path, by the bits of their flag words (1 trim_overlap
        raises in the reference, 2 a broken chain, 4 a job `kchain_many`'s kernel gave back to the host's rv_kchain, 8 twin offsets, 16 the RV_MANY_CHAIN_FLAG hook, 32 more candidates than a kernel's cap, 64 an interval
        of 2^17 positions, 128 the host's picker gave up); bits no job set are left out"""
        o = (ctypes.c_int64 * 8)()
        self._dll.rv_many_flagged(self._m, o)
        return {1 << b: int(o[b]) for b in range(8) if o[b]}

    def run(self, minlength=20, minn=2):
        st = _lib.RvAlignStats()
        if self._dll.rv_many_run(self._m, int(minlength), int(minn), ctypes.byref(st)) != 0:
            self._fail()
        return {f[0]: getattr(st, f[0]) for f in _lib.RvAlignStats._fields_}

    def anchors(self):
        """-> (first[jobs + 1], l, off, pos): job j owns the anchors first[j] .. first[j+1]"""
        nj = len(self._lens)
        first = np.zeros(nj + 1, np.int64)
        mem = ctypes.c_int64(0)
        na = self._dll.rv_many_anchor_count(self._m, first.ctypes.data, ctypes.byref(mem))
        if na < 0:
            self._fail()
        l = np.zeros(max(na, 1), np.uint32); off = np.zeros(na + 1, np.int64); pos = np.zeros(max(mem.value, 1), np.int64)
        if self._dll.rv_many_fetch(self._m, l.ctypes.data, off.ctypes.data, pos.ctypes.data) != 0:
            self._fail()
        return first, l[:na], off, pos[:mem.value]

    def scan(self, minlength=20, minn=2, kind="auto"):
        """rv_many_scan: the match lists of every job instead of a finished recursion.  kind "mums" (0): getmums; "multimums" (1): getmultimums;
        "auto" (2): getmums for the jobs of two sequences, getmultimums for the rest.  The jobs stay; the result of an earlier run() does not."""
        if self._dll.rv_many_scan(self._m, int(minlength), int(minn), SCAN_KINDS[kind] if kind in SCAN_KINDS else int(kind)) != 0:
            self._fail()

    def matches(self):
        """-> (first[jobs + 1], l, n, off, so, pos): job j owns the matches first[j] .. first[j+1], match k the members off[k] .. off[k+1] of so / pos
        (sample and position in the coordinates of the job's own text), in the reference's emission order"""
        nj = len(self._lens)
        first = np.zeros(nj + 1, np.int64)
        mem = ctypes.c_int64(0)
        nm = self._dll.rv_many_match_count(self._m, first.ctypes.data, ctypes.byref(mem))
        if nm < 0:
            self._fail()
        l = np.zeros(max(nm, 1), np.uint32); n = np.zeros(max(nm, 1), np.int32); off = np.zeros(nm + 1, np.int64)
        so = np.zeros(max(mem.value, 1), np.uint16); pos = np.zeros(max(mem.value, 1), np.int64)
        if self._dll.rv_many_fetch_matches(self._m, l.ctypes.data, n.ctypes.data, off.ctypes.data, so.ctypes.data, pos.ctypes.data) != 0:
            self._fail()
        return first, l[:nm], n[:nm], off, so[:mem.value], pos[:mem.value]

    def text(self, j):
        n = self._lens[j] if 0 <= j < len(self._lens) else 0      # (no such job: the library says so)
        buf = ctypes.create_string_buffer(max(n, 1))
        if self._dll.rv_many_text(self._m, j, buf, n) != n or n == 0:
            self._fail()
        return buf.raw

    def arrays(self, j):
        """test hook (RV_MANY_KEEP): (SA, LCP) of a shared-launch job, job-local positions"""
        n = self._lens[j]
        sa = np.zeros(n, self._lib.sa_t); lcp = np.zeros(n, self._lib.lcp_t)
        if self._dll.rv_many_arrays(self._m, j, _lib.RV_SA, sa.ctypes.data, n) != n or self._dll.rv_many_arrays(self._m, j, _lib.RV_LCP, lcp.ctypes.data, n) != n:
            self._fail()
        return sa, lcp


def align_many(jobs, minlength=20, minn=2, sa64=False, toupper=True, batch=None, multi=None, large=None, large_multi=None, wide=None, picker=None, chain=None,
               chain_multi=None, chain_wide=None, chain_large=None, chain_large_multi=None, chain_wide_large=None):
    """jobs: a list of jobs, each a list of (name, seq) or of plain sequences (two or more, none empty; every sequence is a sample
    of its own, like the inputs of `reveal rem`).  -> (results, info): results[j] = dict(anchors=[(l, (pos, ..)), ..], T=final text
    `s0$s1$..` lower-cased where aligned), positions in the coordinates of the job's own text -- what index.align_builtin gives a
    stand-alone index of the job; info = dict(jobs, shared, ordinary, rounds, launches, stats).  `batch`: a Batch to reuse.
    `multi`: True / False sets RV_MANY_MULTI (jobs of 3 .. 16 sequences through the shared launches) for this and later runs of
    the batch; None leaves it as the batch has it (off, unless the environment variable is set).  `large`: the same for RV_MANY_LARGE
    (pair jobs of 2049 .. RV_MANY_LARGE_MAX ranks through the shared launches), `large_multi`: the same for RV_MANY_LARGE_MULTI (jobs of
    3 .. 16 sequences of 2049 .. RV_MANY_LARGE_MAX ranks through the shared launches), `wide`: the same for RV_MANY_WIDE (jobs of 17 .. 64
    sequences up to RV_MANY_LARGE_MAX ranks through the shared launches; more than 64 sequences always run the ordinary way).
    `picker`: a schemes.PickerArgs -- the reference's default picker with these options for this run: a job's result is then what
    index.set_picker(args) + align_builtin give a stand-alone index of it, the anchors `rem.align` chooses for a bubble; None: the built-in
    picker, as ever (a batch that is reused goes back to it).  `chain`: True / False sets RV_MANY_CHAIN (with a picker: the pair jobs of at most
    2048 ranks through the shared launches, see the module docstring) for this and later runs of the batch; None leaves it.  `chain_multi`: the
    same for RV_MANY_CHAIN_MULTI (with a picker: the jobs of 3 .. 16 sequences and at most 2048 ranks through the shared launches), `chain_wide`: the
    same for RV_MANY_CHAIN_WIDE (with a picker: the jobs of 17 .. 64 sequences and at most 2048 ranks through the shared launches), `chain_large`: the
    same for RV_MANY_CHAIN_LARGE (with a picker: the pair jobs of 2049 .. 2^17 ranks through the shared launches), `chain_large_multi`: the same for
    RV_MANY_CHAIN_LARGE_MULTI (with a picker: the jobs of 3 .. 16 sequences and 2049 .. 2^17 ranks through the shared launches), `chain_wide_large`: the
    same for RV_MANY_CHAIN_WIDE_LARGE (with a picker: the jobs of 17 .. 64 sequences and 2049 .. 2^17 ranks through the shared launches)."""
    if isinstance(jobs, (str, bytes, bytearray)) or not hasattr(jobs, "__iter__"):
        raise error("jobs is a list of jobs")
    if int(minlength) < 0 or int(minn) < 2:
        raise error("minlength >= 0 and minn >= 2")
    prepared = [job_sequences(j, toupper) for j in jobs]      # (argument errors before the library is asked for a device)
    if picker is not None:
        picker_struct(picker)
    b = batch if batch is not None else Batch(sa64)
    b.set_picker(picker)
    given = dict(chain=chain, chain_multi=chain_multi, chain_wide=chain_wide, chain_large=chain_large, chain_large_multi=chain_large_multi,
                 chain_wide_large=chain_wide_large, multi=multi, large=large, large_multi=large_multi, wide=wide)
    for key, name in SWITCHES.items():
        if given[key] is not None:
            b.option(name, 1 if given[key] else 0)
    b.clear()
    for seqs in prepared:
        b.add(seqs)
    stats = b.run(minlength, minn)
    first, l, off, pos = b.anchors()
    l, off, pos, first = l.tolist(), off.tolist(), pos.tolist(), first.tolist()
    results = []
    for j in range(len(prepared)):
        an = [(l[k], tuple(pos[off[k]:off[k + 1]])) for k in range(first[j], first[j + 1])]
        results.append(dict(anchors=an, T=b.text(j).decode("latin-1")))
    info = b.info()
    info["stats"] = stats
    return results, info


class Matches:
    """the match lists of `mums_many`: `arrays` = the CSR (first, l, n, off, so, pos) as numpy arrays; matches[j] = job j's list in the reference's
    shapes, built when asked for: [(l, (a, b), 0), ..] where the job was scanned with getmums, [(l, n, ((sample, pos), ..)), ..] with getmultimums"""

    def __init__(self, arrays, pair_shape):
        self.arrays = arrays
        self._pair = pair_shape      # per job: the list has getmums' shape

    def __len__(self):
        return len(self._pair)

    def __getitem__(self, j):
        if not -len(self._pair) <= j < len(self._pair):
            raise IndexError("job %d of %d" % (j, len(self._pair)))
        j %= len(self._pair)
        first, l, n, off, so, pos = self.arrays
        lo, hi = int(first[j]), int(first[j + 1])
        if self._pair[j]:
            return [(int(l[k]), (int(pos[off[k]]), int(pos[off[k] + 1])), 0) for k in range(lo, hi)]
        return [(int(l[k]), int(n[k]), tuple((int(so[q]), int(pos[q])) for q in range(int(off[k]), int(off[k + 1])))) for k in range(lo, hi)]

    def __iter__(self):
        return (self[j] for j in range(len(self._pair)))


def mums_many(jobs, minlength=20, minn=2, kind="auto", sa64=False, toupper=True, batch=None, large=None):
    """jobs: as for `align_many`.  -> (matches, info): the MUM / multi-MUM list of every job -- what `index.getmums(minlength)` (kind "mums"; for a
    job of more than two sequences: sample 0 against the rest) or `index.getmultimums(minlength, minn)` (kind "multimums") give a stand-alone index
    of the job, in its coordinates and emission order; kind "auto": getmums for the jobs of two sequences, getmultimums for the rest, as
    `reveal chain --recurse` asks per gap.  The jobs `takes_shared_scan` names share their launches (index build with the text in LDS, a count
    pass, a sum and a write pass over every job of a round at once); every other job runs the ordinary way inside the call.  matches: a `Matches`
    (`.arrays` = first, l, n, off, so, pos; matches[j] = the job's list in the reference's shapes); info = dict(jobs, shared, ordinary, rounds,
    launches).  `batch`: a Batch to reuse.  `large`: True / False sets RV_MANY_SCAN_LARGE (the jobs of 2049 .. RV_MANY_LARGE_MAX ranks through shared
    launches as well, their indices built by the segmented prefix doubling; `takes_shared_scan(.., large=True)`) for this and later scans of the
    batch; None leaves it as the batch has it (off, unless the environment variable is set)."""
    if isinstance(jobs, (str, bytes, bytearray)) or not hasattr(jobs, "__iter__"):
        raise error("jobs is a list of jobs")
    if kind not in SCAN_KINDS:
        raise error("kind is one of %s" % ", ".join(sorted(SCAN_KINDS)))
    if int(minlength) < 0:
        raise error("minlength >= 0")
    prepared = [job_sequences(j, toupper) for j in jobs]      # (argument errors before the library is asked for a device)
    b = batch if batch is not None else Batch(sa64)
    if large is not None:
        b.option("RV_MANY_SCAN_LARGE", 1 if large else 0)
    b.clear()
    for seqs in prepared:
        b.add(seqs)
    b.scan(minlength, minn, kind)
    code = SCAN_KINDS[kind]
    return Matches(b.matches(), [code == 0 or (code == 2 and len(s) == 2) for s in prepared]), b.info()
