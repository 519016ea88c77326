// rv_merge.h -- merge_consecutive of `reveal transform` (transform.py:713-746) on a block list in columns: rv_merge.hip.  The rule is stated in
// include/reveal_amd.h (rv_merge_blocks); the join test and the merged block are ONE pair of functions below, compiled for the host rule and for
// the kernels alike.
#pragma once
#include "rv_common.h"
#include <vector>

// the caller's columns (n rows) and the rows that make the list: sel[0 .. m) in list order, or every row where sel is NULL (then m = n)
struct RvMrgIn {
    int64_t n = 0;
    const int64_t *s1 = nullptr, *e1 = nullptr, *s2 = nullptr, *e2 = nullptr; const int32_t *o = nullptr; const int64_t *score = nullptr;
    const int32_t *refid = nullptr, *ctgid = nullptr;
    const int32_t *sel = nullptr; int64_t m = 0;
};
// the merged list on the host, in the order of the rule (ascending s1, ties in list order)
struct RvMrgOut {
    std::vector<int64_t> s1, e1, s2, e2, score;
    std::vector<int32_t> o, refid, ctgid;
    void clear() { s1.clear(); e1.clear(); s2.clear(); e2.clear(); score.clear(); o.clear(); refid.clear(); ctgid.clear(); }
    void resize(size_t k) { s1.resize(k); e1.resize(k); s2.resize(k); e2.resize(k); score.resize(k); o.resize(k); refid.resize(k); ctgid.resize(k); }
    size_t size() const { return s1.size(); }
};
// info[] of a call (int64)
enum { RV_MRG_ROUTE = 0, RV_MRG_ROWS_IN, RV_MRG_ROWS_OUT, RV_MRG_BYTES_UP, RV_MRG_BYTES_DOWN, RV_MRG_BITS1, RV_MRG_BITS2, RV_MRG_LAUNCHES, RV_MRG_KERNEL_NS,
       RV_MRG_INFO };

// R[i] joins R[i-1]: the same contig, neighbours in the query order in the direction of their common orientation (refid is not compared)
__host__ __device__ inline bool mrg_joins(int32_t ctg_p, int32_t o_p, int64_t q_p, int32_t ctg, int32_t o, int64_t q) {
    if (ctg != ctg_p || o != o_p) return false;
    return o == 0 ? q == q_p + 1 : q == q_p - 1;
}

// what the list's entries hold: -> 0 and the largest s1 and s2 of the list; the columns' rows, sel and the scores' total are checked
int rv_merge_validate(const RvMrgIn &in, int64_t *max_s1, int64_t *max_s2);
// the rule in host C++ (no device is asked for); the input is taken as validated
int rv_merge_rule_host(const RvMrgIn &in, RvMrgOut &out);
// the kernels; max_s1 / max_s2 size the two sorts' keys.  info: RV_MRG_INFO words or NULL
int rv_merge_device(Workspace &ws, const RvMrgIn &in, int64_t max_s1, int64_t max_s2, int64_t *info, RvMrgOut &out);
