// rv_tail.h -- the stages of `reveal transform` behind merge_consecutive that score a chain: chainscore (transform.py:836-935) and one sweep of
// optimise (:801-834), host C++ with 64-bit integers: rv_tail.hip.  The lists are the few blocks merge_consecutive leaves; nothing here asks for a device.
#pragma once
#include "rv_glocal.h"
#include <vector>

struct RvTailIn {
    int64_t n = 0;
    const int64_t *s1 = nullptr, *e1 = nullptr, *s2 = nullptr, *e2 = nullptr; const int32_t *o = nullptr; const int64_t *score = nullptr;
    const int32_t *refid = nullptr, *ctgid = nullptr;
    int64_t nseq = 0; const int64_t *rs = nullptr, *re = nullptr;      // (begin, '$') of every sequence in order of addition (ctg2range)
    int64_t rlength = 0, qlength = 0;
};

// coordinates inside 0 .. 2^61, o in {0, 1}, scores >= 0, ctgid names a sequence, weights >= 0 and inside rv_glocal_admit_rule's bound; -> 0
int rv_tail_validate(const RvTailIn &in, const RvGlcParams &w);
// chainscore of the list (ties of s1 in list order): weight, cost, and the n + 1 edge costs where edgecosts is not NULL
int rv_chainscore_rule_host(const RvTailIn &in, const RvGlcParams &w, int64_t *weight, int64_t *cost, std::vector<int64_t> *edgecosts);
// one sweep of optimise: kept = the rows of the best chain in reference order, with its weight and cost
int rv_optimise_rule_host(const RvTailIn &in, const RvGlcParams &w, int64_t *weight, int64_t *cost, std::vector<int32_t> &kept);
