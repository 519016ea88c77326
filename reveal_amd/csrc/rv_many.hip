// rv_many.hip -- many small pair alignments in one call (include/reveal_amd.h "many small alignments").
//
// `reveal refine --method reveal_rem` calls the recursion once per bubble (reveal/refine.py:220-229): 10^4 - 10^6 inputs of a few
// bases up to 10 kbp.  Through a handle each of them pays for a construct() and a level loop -- dozens of launches and several
// stream waits, whatever its size.  Here the pair jobs of at most RV_LEAF_N ranks share their launches:
//   text     all first sequences, then all second sequences (a_0$a_1$..a_J-1$b_0$..b_J-1$): ONE nsep[0] separates the two samples
//            of every job, so the leaf kernel, pair_intervals and the lower-casing work on it unchanged
//   build    k_many_build: SA, LCP and the BWT byte of every job from a job-local copy of its text `a$b$` in LDS
//   finish   the segments become a level-0 frontier of J roots of a handle that was never constructed (rv_frontier_import);
//            every root is leaf-sized, so rv_align_builtin_resume is ONE leaf launch
// Jobs the shared launches do not take (more than two sequences, more than RV_LEAF_N ranks) run the ordinary way -- construct() +
// rv_align_builtin -- on one internal handle reused with rv_reset.
//
// RV_MANY_MULTI (off by default): the jobs of 3 .. RV_MANY_KMAX sequences with at most RV_LEAF_N ranks (sum of lengths + k) and no NUL
// byte share their launches as well, in rounds of their own (many_round_multi):
//   text     every job contiguous, s0$s1$..s(k-1)$, job after job: a position minus the job's begin is its stand-alone coordinate
//   build    k_many_build as it is: to it such a job is its first sequence and "the rest" -- the job-local text is the stand-alone
//            text whatever '$' it holds (the side bit of the BWT byte means nothing here; the leaf kernel masks it)
//   finish   ONE launch of k_leaf_multi (rv_leaf_multi.hip) over the built segments: a job's whole recursion in one workgroup, one
//            interval per sample in a frame; it lower-cases the text itself.  No frontier, no handle: three launches per round
//
// k_many_build, per job (n = la + lb + 2 <= 2048 ranks, local positions in 16 bits):
//   order    prefix doubling: first key = six text bytes (past the end: 0, so a suffix that is a prefix of another sorts first and
//            suffixes that tie through a '$' come out in the stand-alone order), then keys (rank[i], rank[i + h]), h = 6, 12, 24 ..
//            until every rank is its own; each round is one bitonic sort of (key << 16 | position) words in LDS -- alleles of one
//            bubble tie for hundreds of characters, homopolymers within a sequence: <= 10 rounds at 2048 ranks
//   LCP      text order with Kasai's carry (interface.c:97-114: stops at '$' / 'N'), eight bytes per step; a thread takes
//            consecutive text positions, so its work is its share plus one LCP value, not share x LCP
//   BWT      the character in front ('$' for local position 0), RV_BWT_SIDE for the suffixes of the second sequence
//
// RV_MANY_LARGE (off by default): the pair jobs of more than RV_LEAF_N and at most RV_MANY_LARGE_MAX ranks with no NUL byte share their launches
// too, in rounds of their own (many_round with `large`): the pair layout above, the index built by a segmented prefix doubling in HBM over every
// job of the round at once (rv_many_large.hip), and the same finish -- rv_frontier_import of J roots + rv_align_builtin_resume.  The roots are not
// leaf-sized, so the resume runs the level pipeline: every sub-index of a level in one scan, split and bubble launch, children dropping into the
// leaf kernel as they shrink.  A level-0 frontier of several roots is to builtin_levels what a worker of a divided alignment imports (install_frontier
// makes it level 1; a root is told from a child by nothing but its depth, which only the statistics read).
//
// RV_MANY_LARGE_MULTI (off by default): the jobs of 3 .. RV_MANY_KMAX sequences with more than RV_LEAF_N and at most RV_MANY_LARGE_MAX ranks and no
// NUL byte share their launches too, in rounds of their own (many_round_large_multi).  A round may mix jobs of different k; its handle has K
// samples, K the round's widest job:
//   text     sample-major: sample q holds the q-th sequence of every job that has one, in the round's job order, a '$' behind each; nsep[q] is the
//            '$' behind the last of them.  The sample of a position is then right for every job at once, and a job's stand-alone coordinate ->
//            shared position map is strictly increasing, so every tie-break by position comes out as in the stand-alone index
//   build    the segmented prefix doubling of rv_many_large.hip over job-local texts s0$s1$..s(k-1)$ gathered from the k places
//   finish   rv_frontier_import of J roots (nsamples = the job's k, k intervals each) + rv_align_builtin_resume: the level pipeline for more
//            than two samples, down to the last sub-index (there is no leaf kernel for multi-sample sub-indices of a handle)
//
// RV_MANY_WIDE (off by default, independent of the other switches): the jobs of 17 .. RV_MANY_WIDE_KMAX = 64 sequences with no NUL byte share their
// launches too, in rounds of their own -- the composition of the other classes' rounds does not change.  Up to RV_LEAF_N ranks: many_round_multi
// with the 64-sample form of k_leaf_multi (k_many_build does not know k).  Above, up to RV_MANY_LARGE_MAX ranks and from RV_MANY_WIDE_LARGE_MIN such
// jobs in a call on: many_round_large_multi with K up to 64.  64: a lane of a wavefront owns a sample in the leaf kernel, the sample id has six
// bits of its `smp` byte, and the level pipeline's multi-sample scan keeps a one-word census up to 64 samples.  Jobs of more than 64 sequences
// stay ordinary.
//
// rv_many_set_picker(m, 1, args): the reference's default picker (schemes.graphmumpicker; rv_pick_chain, rv_chain.hip) instead of the built-in one -- what
// `reveal refine` aligns its bubbles with.  Every shared class above finishes with built-in-picker kernels, so under kind 1 none of them takes a job,
// whatever its switch says: the jobs run the ordinary way with rv_set_picker(h, 1, args) on the internal handle.  RV_MANY_CHAIN (off by default): the
// pair jobs of its row of many_classes (many_class_admits) share their launches all the same -- layout, index build and frontier of the small pair jobs, and ONE launch of
// k_leaf_chain (rv_leaf_chain.hip), the leaf kernel with the picker's decision for two samples as its pick stage.  A job the kernel flags (where the
// reference's own trim_overlap raises) is dropped from the round's results and runs the ordinary way.  The results do not depend on the switch.
// RV_MANY_CHAIN_MULTI (off by default, independent of RV_MANY_CHAIN and RV_MANY_MULTI; it means something under kind 1 only): the jobs of 3 .. RV_MANY_KMAX
// sequences of its row of many_classes share their launches too, in rounds of their own -- layout and index build of RV_MANY_MULTI (many_round_multi) and
// ONE launch of k_leaf_multi_chain (rv_leaf_multi_chain.hip), the multi-sample leaf kernel with the whole picker as its pick stage: matches on sample
// subsets, `segment`, trim and chain over k paths, a three-way split with a `rest` child.  Flags as for k_leaf_chain, per job.
// RV_MANY_CHAIN_WIDE (off by default, independent of every other switch; it means something under kind 1 only): the jobs of 17 .. RV_MANY_WIDE_KMAX = 64
// sequences of its row of many_classes share their launches too, in rounds of their own -- layout and index build of the small RV_MANY_WIDE rounds
// (many_round_multi with kmax = 64) and ONE launch of the 64-sample form of k_leaf_multi_chain.  Flags and test hooks as for RV_MANY_CHAIN_MULTI.  Under a
// picker the jobs of 17 .. 64 sequences above RV_LEAF_N ranks are RV_MANY_CHAIN_WIDE_LARGE's (below); every job of more than 64 sequences stays ordinary.
// RV_MANY_CHAIN_LARGE (off by default, independent of every other switch; it means something under kind 1 only): the pair jobs of its row of many_classes
// -- more than RV_LEAF_N and at most min(RV_MANY_LARGE_MAX, 2^17) ranks -- share their launches too, in rounds of their own, from RV_MANY_CHAIN_LARGE_MIN such
// jobs in a call on: layout, segmented index build and frontier of the RV_MANY_LARGE rounds (many_round with `large` and `redo`), and the level pipeline under
// the chain route -- every sub-index above RV_LEAF_N ranks gets its pick from k_pick_chain (rv_pick_chain.hip: the picker's decision for two samples, a
// wavefront per sub-index, in place of the longest-match kernel; k_decide and the early split as they are), the others drop into k_leaf_chain as they shrink.
// The flag words are the jobs': a flag set by any launch of any level drops all of the job's anchors, leaves its text untaken and sends it to the ordinary path.
// RV_MANY_CHAIN_LARGE_MULTI (off by default, independent of every other switch; it means something under kind 1 only): the jobs of 3 .. RV_MANY_KMAX sequences
// of its row of many_classes -- more than RV_LEAF_N and at most min(RV_MANY_LARGE_MAX, 2^17) ranks -- share their launches too, in rounds of their own,
// from RV_MANY_CHAIN_LARGE_MULTI_MIN such jobs in a call on: sample-major layout, index build and frontier of the RV_MANY_LARGE_MULTI rounds
// (many_round_large_multi with `redo`), and the multi-sample level pipeline under its chain route (rv_multi_chain_route) -- every level's scan unfiltered, every
// sub-index picked by k_pick_multi_chain (rv_pick_multi_chain.hip: the picker's decision for up to 16 samples, a wavefront per sub-index) in place of
// k_multi_pick1 / k_multi_pick2, the early split off; a pick of a sample subset leaves a `rest` child.  There is no leaf kernel for multi-sample sub-indices of
// a handle: sub-indices of every size are picked this way.  Flag words per job as above.
// RV_MANY_CHAIN_WIDE_LARGE (off by default, independent of every other switch; it means something under kind 1 only): the jobs of 17 .. RV_MANY_WIDE_KMAX = 64
// sequences of its row of many_classes -- more than RV_LEAF_N and at most min(RV_MANY_LARGE_MAX, 2^17) ranks -- share their launches too, in rounds of
// their own, from RV_MANY_CHAIN_WIDE_LARGE_MIN such jobs in a call on: the rounds of RV_MANY_CHAIN_LARGE_MULTI with kmax = RV_MANY_WIDE_KMAX
// (many_round_large_multi with `redo`), every sub-index picked by the 64-sample form of k_pick_multi_chain.  That form holds 256 candidates a sub-index, not
// 512, and its weight bound is 128: a sub-index with more flags its job (32), which finishes on the ordinary path.  Jobs of more than 64 sequences stay ordinary.
// rv_many_scan: the MUM / multi-MUM lists of every job instead of a finished recursion (many_scan below; the kernels are rv_many_scan.hip's).  Every clean job
// of 2 .. RV_MANY_WIDE_KMAX sequences and at most RV_LEAF_N ranks goes through rounds of its own kind (many_round_scan): the job-contiguous layout of
// many_round_multi for every k, k_many_build as it is, then a count pass, an exclusive sum and a write pass flat over the ranks of the round.  No switch, no
// threshold.  With RV_MANY_SCAN_LARGE on, the clean jobs of 2 .. RV_MANY_WIDE_KMAX sequences and RV_LEAF_N + 1 .. RV_MANY_LARGE_MAX ranks go through rounds of the
// same layout as well, from RV_MANY_SCAN_LARGE_MIN such jobs in a call on: the index build is rv_many_large_build_c -- the segmented prefix doubling on the
// round's text in place --, everything behind it is the small rounds' (many_round_scan with `large`).  One class for every k.
// The other jobs run rv_getmums / rv_getmultimums on the internal handle.  A scan does not touch the jobs or their text; `ran` and `scanned` say
// which result is live.
// Size classes (DESIGN.md "Many small alignments" has the measurements): up to `wave_max` ranks (default 512) a wavefront per job,
// four jobs per workgroup, no workgroup barrier; above, a workgroup of 256 threads per job.  Both hold 22.6 KB of LDS per workgroup:
// seven workgroups per CU.
#include "rv_index.h"
#include "rv_leaf.h"
#include "rv_leaf_multi.h"
#include "rv_many_large.h"
#include "rv_many_scan.h"
#include "rv_kchain_big.h"
#include <algorithm>
#include <limits.h>
#include <new>
#include <stdexcept>

namespace {

constexpr int MT = 256;                    // threads per workgroup
constexpr int CAP_L = RV_LEAF_N;           // ranks of the largest job a workgroup builds
constexpr int CAP_S = 512;                 // ... a wavefront builds
static_assert(CAP_L <= 2048, "local ranks are packed in 12 bits, positions in 16");

__device__ inline u32 many_wave_incl_max(u32 v) {
    const int lane = threadIdx.x & 63;
#define MANY_STEP_(CTRL, RM, TAKE) { const u32 o = rv_dpp_u32<CTRL, RM>(v); v = ((TAKE) && o > v) ? o : v; }
    RV_WAVE_SCAN_STEPS(MANY_STEP_)
#undef MANY_STEP_
    return v;
}
__device__ inline u32 many_lane_below(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
// bit 7 of every byte of v that is zero (exact for the lowest such byte)
__device__ inline u64 many_zero_bytes(u64 v) { return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull; }

// TPJ threads per job (64: a wavefront, synchronised by wave barriers; 256: the workgroup), CAP ranks at most
template <int CAP, int TPJ>
__global__ __launch_bounds__(MT) void k_many_build(const ManyDevJob *__restrict__ jobs, int njobs, const uint8_t *__restrict__ T, sa_t *__restrict__ SA,
                                                   lcp_t *__restrict__ LCP, uint8_t *__restrict__ BWT, u32 *__restrict__ d_maxlcp, u32 *__restrict__ d_err) {
    constexpr int JPB = MT / TPJ;          // jobs per workgroup
    constexpr int PER = CAP / TPJ;         // consecutive ranks a thread names
    __shared__ __attribute__((aligned(16))) u64 s_key[JPB][CAP];
    __shared__ __attribute__((aligned(16))) uint8_t s_txt[JPB][CAP + 16];
    __shared__ uint16_t s_rank[JPB][CAP];
    __shared__ u32 s_part[JPB][4];
    __shared__ int s_tied[JPB];
    const int slot = (int)threadIdx.x / TPJ, t = (int)threadIdx.x % TPJ;
    const int jn = (int)blockIdx.x * JPB + slot;
    if (jn >= njobs) return;               // (a whole wavefront of the last workgroup; TPJ == 256: the grid is the job count)
    const ManyDevJob J = jobs[jn];
    const int la = J.la, n = J.la + J.lb + 2;
    if (n > CAP || J.la < 1 || J.lb < 1) { if (t == 0) atomicOr(d_err, 1u); return; }
    u64 *key = s_key[slot];
    uint8_t *txt = s_txt[slot];
    uint16_t *rank = s_rank[slot];
#define MANY_SYNC() do { if (TPJ == 64) RV_WSYNC(); else __syncthreads(); } while (0)
    int N2 = 2;
    while (N2 < n) N2 <<= 1;               // size of the sorting network (<= CAP)

    for (int k = t; k < n + 16; k += TPJ) txt[k] = k <= la ? T[J.abeg + k] : (k < n ? T[J.bbeg + (k - la - 1)] : (uint8_t)0);
    MANY_SYNC();
    for (int p = t; p < N2; p += TPJ) {
        u64 k = ~0ull;                     // (padding of the network: behind every suffix)
        if (p < n) {
            k = 0;
#pragma unroll
            for (int b = 0; b < 6; b++) k = (k << 8) | txt[p + b];
            k = (k << 16) | (u64)p;
        }
        key[p] = k;
    }
    const int c = (N2 + TPJ - 1) / TPJ;    // ranks per thread when the order is read (<= PER)
    int h = 6;
    for (int round = 0;; round++) {
        MANY_SYNC();
        if (t == 0) s_tied[slot] = 0;
        for (int k = 2; k <= N2; k <<= 1) {
            for (int jj = k >> 1; jj > 0; jj >>= 1) {
                for (int p = t; p < (N2 >> 1); p += TPJ) {
                    const int i = ((p & ~(jj - 1)) << 1) | (p & (jj - 1)), q = i | jj;
                    const u64 a = key[i], b = key[q];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[q] = a; }
                }
                MANY_SYNC();
            }
        }
        // a suffix' new rank = 1 + the first position of its run of equal keys: inclusive maximum over the run heads
        u64 kv[PER];
        u32 mine = 0; bool tie = false;
        const int p0 = t * c;
#pragma unroll
        for (int e = 0; e < PER; e++) {
            const int p = p0 + e;
            kv[e] = 0;
            if (e < c && p < n) {
                kv[e] = key[p];
                const bool head = p == 0 || (key[p - 1] >> 16) != (kv[e] >> 16);
                if (head) mine = (u32)p + 1; else tie = true;
            }
        }
        const u32 inc = many_wave_incl_max(mine);
        u32 run = many_lane_below(inc);
        if (TPJ > 64) {
            const int wv = t >> 6;
            if ((t & 63) == 63) s_part[slot][wv] = inc;
            __syncthreads();
            for (int w = 0; w < wv; w++) { const u32 o = s_part[slot][w]; run = o > run ? o : run; }
        }
#pragma unroll
        for (int e = 0; e < PER; e++) {
            const int p = p0 + e;
            if (e < c && p < n) {
                if (p == 0 || (key[p - 1] >> 16) != (kv[e] >> 16)) run = (u32)p + 1;
                rank[(int)(kv[e] & 0xFFFFu)] = (uint16_t)run;
            }
        }
        if (tie) s_tied[slot] = 1;
        MANY_SYNC();
        if (!s_tied[slot]) break;
        if (round >= 16) { if (t == 0) atomicOr(d_err, 2u); return; }      // (cannot happen: h passes n after eleven rounds; a job is left by all its threads)
        for (int p = t; p < n; p += TPJ) {      // (every thread read the order in front of the barrier above)
            const u32 r1 = rank[p], r2 = p + h < n ? rank[p + h] : 0u;
            key[p] = ((u64)((r1 << 12) | r2) << 16) | (u64)p;
        }
        h <<= 1;
    }
    // the order is final: rank[i] - 1 is the inverse.  SA and LCP in 16 bits over the sort's words
    uint16_t *sa16 = (uint16_t *)key, *lcp16 = sa16 + CAP;
    {
        uint16_t mine16[PER];
#pragma unroll
        for (int e = 0; e < PER; e++) { const int p = t + e * TPJ; mine16[e] = p < n ? (uint16_t)(key[p] & 0xFFFFu) : (uint16_t)0; }
        MANY_SYNC();
#pragma unroll
        for (int e = 0; e < PER; e++) { const int p = t + e * TPJ; if (p < n) sa16[p] = mine16[e]; }
        MANY_SYNC();
    }
    u32 lmax = 0;
    {
        const int c2 = (n + TPJ - 1) / TPJ;
        int hh = 0;
        for (int i = t * c2; i < (t + 1) * c2 && i < n; i++) {
            const int k = (int)rank[i] - 1;
            if (k > 0) {
                const int j = sa16[k - 1];
                for (;;) {
                    u64 a, b;
                    __builtin_memcpy(&a, txt + i + hh, 8);
                    __builtin_memcpy(&b, txt + j + hh, 8);
                    const u64 x = a ^ b, z = many_zero_bytes(a ^ 0x2424242424242424ull) | many_zero_bytes(a ^ 0x4E4E4E4E4E4E4E4Eull);      // '$', 'N'
                    const int m = x ? (int)(__builtin_ctzll(x) >> 3) : 8, s = z ? (int)(__builtin_ctzll(z) >> 3) : 8;
                    const int step = m < s ? m : s;
                    hh += step;
                    if (step < 8) break;   // (the text ends with '$': no comparison runs past it)
                }
                lcp16[k] = (uint16_t)hh;
                if ((u32)hh > lmax) lmax = (u32)hh;
            } else lcp16[0] = 0;
            if (hh > 0) hh--;
        }
    }
    MANY_SYNC();
    for (int p = t; p < n; p += TPJ) {
        const int i = sa16[p];
        SA[J.off + p] = (sa_t)(i <= la ? J.abeg + i : J.bbeg + (i - la - 1));
        LCP[J.off + p] = (lcp_t)lcp16[p];
        BWT[J.off + p] = (uint8_t)((i > 0 ? txt[i - 1] : (uint8_t)'$') | (i > la ? RV_BWT_SIDE : 0u));
    }
    lmax = (u32)rv_wave_max_u64((u64)lmax);
    if ((threadIdx.x & 63) == 0 && lmax > __atomic_load_n(d_maxlcp, __ATOMIC_RELAXED)) atomicMax(d_maxlcp, lmax);
#undef MANY_SYNC
}

struct ManyJob {
    int k = 0;                             // sequences
    size_t seq0 = 0;                       // first entry in lens / starts
    int64_t ranks = 0;                     // sum of lengths + k
    bool clean = true;                     // no NUL byte (the past-the-end character of the build)
    bool shared = false;
    int64_t text_off = 0;                  // final text in out_text (ranks bytes)
    int64_t arr_off = -1;                  // RV_MANY_KEEP: SA / LCP in keep_sa / keep_lcp
};
struct ManyRec { int job; u32 l; int np; int64_t p0; };
struct ManyScanSlice { int64_t rec0 = 0, nrec = 0, mem0 = 0, nmem = 0; };      // a job's matches in the scratch of a scan
struct ManyKchainSlice { bool done = false; int64_t node0 = 0, nnodes = 0, pos0 = 0, end = 0; };      // a job's chain in the scratch of rv_many_kchain

}  // namespace

struct rv_many {
    int device = 0;
    rv_index *hs = nullptr, *ho = nullptr;      // the shared launches' handle (never constructed), the ordinary path's
    std::vector<char> in;                       // the jobs' sequences back to back
    std::vector<int64_t> lens, starts;
    std::vector<ManyJob> jobs;
    int64_t keep = 0, round_max = (int64_t)1 << 27, wave_max = CAP_S;
    int64_t multi = 0, stage = 256;             // RV_MANY_MULTI, RV_MANY_STAGE
    int64_t large = 0, large_max = RV_MANY_LARGE_MAX_DEFAULT, large_min = RV_MANY_LARGE_MIN_DEFAULT;      // RV_MANY_LARGE, RV_MANY_LARGE_MAX, RV_MANY_LARGE_MIN
    int64_t large_multi = 0, large_multi_min = 16;      // RV_MANY_LARGE_MULTI, RV_MANY_LARGE_MULTI_MIN (DESIGN.md "Many small alignments": 4 such jobs lose, 16 win)
    int64_t wide = 0, wide_large_min = RV_MANY_WIDE_LARGE_MIN_DEFAULT;      // RV_MANY_WIDE, RV_MANY_WIDE_LARGE_MIN
    int picker = 0; rv_picker_args pargs{};     // rv_many_set_picker
    int64_t chain = 0, chain_flag = 0;          // RV_MANY_CHAIN, RV_MANY_CHAIN_FLAG (test hook)
    int64_t chain_multi = 0;                    // RV_MANY_CHAIN_MULTI
    int64_t chain_wide = 0;                     // RV_MANY_CHAIN_WIDE
    int64_t chain_large = 0, chain_large_min = RV_MANY_CHAIN_LARGE_MIN_DEFAULT;      // RV_MANY_CHAIN_LARGE, RV_MANY_CHAIN_LARGE_MIN
    int64_t chain_large_multi = 0, chain_large_multi_min = RV_MANY_CHAIN_LARGE_MULTI_MIN_DEFAULT;      // RV_MANY_CHAIN_LARGE_MULTI, RV_MANY_CHAIN_LARGE_MULTI_MIN
    int64_t chain_wide_large = 0, chain_wide_large_min = RV_MANY_CHAIN_WIDE_LARGE_MIN_DEFAULT;        // RV_MANY_CHAIN_WIDE_LARGE, RV_MANY_CHAIN_WIDE_LARGE_MIN
    std::vector<std::pair<std::string, int64_t>> fwd;      // switches for the internal handles
    // results of the last run
    bool ran = false;
    std::vector<int64_t> an_first, an_off, an_pos;
    std::vector<u32> an_l;
    std::vector<char> out_text;
    std::vector<sa_t> keep_sa; std::vector<lcp_t> keep_lcp;
    int64_t info[5] = {0, 0, 0, 0, 0};
    int64_t flagged[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // rv_many_flagged: the jobs of the last run a chain round sent to the ordinary path, per bit of their flag word
    DBuf dJobs, dKJobs, dSA, dLCP, dBWT, dCnt;
    DBuf dFlag;                                 // rounds of k_leaf_chain: a word per job
    DBuf dBeg;                                  // ... and the text begins of the jobs' first / second sequences
    DBuf dTxt, dMJobs, dAn, dAnPos;             // rounds of multi-sequence jobs: their text, jobs, anchors
    RvManyLargeBufs large_bufs;                      // rounds of large pair jobs: the scratch of their index build
    // scratch of a run
    std::vector<ManyRec> recs; std::vector<int64_t> rpos;
    // rv_many_scan: at most one of `ran` and `scanned` is set -- the live result is the last call's
    int64_t scan_ordinary = 0;                  // RV_MANY_SCAN_ORDINARY
    int64_t scan_large = 0, scan_large_min = RV_MANY_SCAN_LARGE_MIN_DEFAULT;      // RV_MANY_SCAN_LARGE, RV_MANY_SCAN_LARGE_MIN
    bool scanned = false;
    std::vector<int64_t> mt_first, mt_off, mt_pos;
    std::vector<u32> mt_l; std::vector<int32_t> mt_n; std::vector<uint16_t> mt_so;
    DBuf dScanTab, dScanCnt, dScanFirst, dScanOut;
    // scratch of a scan: the lists as the rounds and the ordinary path deliver them, and every job's slice of them
    std::vector<ManyScanSlice> sc_job;
    std::vector<u32> sc_l; std::vector<int32_t> sc_n; std::vector<uint16_t> sc_so; std::vector<int64_t> sc_pos;
    // rv_many_kchain: a scan (kind 1, minn = k per job) whose lists are chained where they lie; `chained` is live alone, as `ran` and `scanned` are
    const RvKchainArgs *kc = nullptr;           // set while rv_many_kchain runs
    bool kc_host = false;                       // RV_MANY_KCHAIN_HOST of that call
    bool chained = false;
    std::vector<int64_t> kch_first, kch_score, kch_pos, kch_end;
    std::vector<u32> kch_l;
    DBuf dKcStage, dKcJob, dKcOut;
    RvKchainBigBufs kc_big_bufs;                // the device programme for the lists no round has chained (rv_kchain_big.hip)
    int64_t kc_big[2] = {0, 0};                 // rv_many_kchain_big: the lists of the last call it chained, its step launches
    std::vector<ManyKchainSlice> kc_job;        // scratch of the call
    std::vector<u32> kc_l; std::vector<int64_t> kc_score, kc_pos;
};

namespace {

// a job a chain round gives back: which bits its flag word holds (1, 2, 4, .. 128 -> flagged[0 .. 7])
void many_count_flags(rv_many *m, u32 word) {
    for (int b = 0; b < 8; b++) if (word >> b & 1u) m->flagged[b]++;
}

int many_handle(rv_many *m, rv_index **h) {
    if (*h) return 0;
    *h = rv_new(m->device);
    if (!*h) return -1;
    for (auto &o : m->fwd) RV_TRY(rv_set_option(*h, o.first.c_str(), o.second));
    return 0;
}

// The classes of jobs that share launches, in the order in which many_run runs their rounds (the order of `info`, of `rest` and of the launches).  The
// domains of the rows are disjoint in (picker kind, k, ranks): a job matches at most one.  many_class_admits states the rule, rv_many_option takes the
// names of the switches and thresholds from here, and many.CLASSES (many.takes_shared_launch) mirrors the table row by row.
//   picker        the picker kind the class belongs to: every built-in class finishes with built-in-picker kernels, so under kind 1 none of them
//                 takes a job, whatever its switch says, and the kind-1 classes mean nothing without a picker
//   kmin .. kmax  sequences of a job; kmax is the sample bound of the round routine's kernels as well
//   large         false: ranks <= RV_LEAF_N.  true: RV_LEAF_N < ranks <= RV_MANY_LARGE_MAX, and the job has to fit a round (ranks <= lim: one that does not
//                 goes the ordinary way); under kind 1 also ranks <= RV_PICK_CHAIN_RANKS = 2^17 -- positions and lengths of a sub-index in 17 bits,
//                 whatever RV_MANY_LARGE_MAX says
//   sw, min       the switch (none: always on) and the threshold: fewer admitted jobs in a call stay ordinary (none: one job is enough).  Every class is
//                 counted on its own against a threshold of its own: what a call does with the jobs of one class does not depend on the others
//   wmax, by_ranks   kind 1 only: the weight cap, and whether `maxmums` is compared with the job's ranks or (pairs) with the shorter sequence
//   round         the routine that runs the class, with the row's `large` / kmax; a kind-1 round passes `rest` as its `redo`
enum ManyRoundKind { MANY_PAIRS, MANY_CONTIGUOUS, MANY_SAMPLE_MAJOR };      // many_round, many_round_multi, many_round_large_multi
struct ManyClass {
    int picker, kmin, kmax;
    bool large;
    const char *sw_name; int64_t rv_many::*sw;
    const char *min_name; int64_t rv_many::*min;
    int wmax; bool by_ranks;
    ManyRoundKind round;
};
static_assert(RV_PICK_CHAIN_WMAX == RV_LEAF_MCHAIN_WMAX && RV_PICK_CHAIN_WMAX <= RV_LEAF_CHAIN_WMAX, "one weight bound for the class");
static_assert(RV_PICK_MCHAIN_KMAX == RV_MANY_KMAX && RV_PICK_WCHAIN_KMAX == RV_MANY_WIDE_KMAX, "the two forms of k_pick_multi_chain take the two classes");
static const ManyClass many_classes[] = {
    // the small pair jobs: no switch
    {0, 2, 2, false, nullptr, nullptr, nullptr, nullptr, 0, false, MANY_PAIRS},
    // RV_MANY_CHAIN: the pair jobs k_leaf_chain finishes.  Everything the kernel leaves out has to be impossible for the job: no p-value cut (minl > 0), no
    // untrimmed lists, no seeds for the children (--seedsize above the longer sequence: no match is that long), no --maxmums cut (two MUMs never start at the
    // same position of either sequence, so a sub-index never holds more than min(la, lb)), weights that keep the scores in 32 bits (rv_leaf_chain.hip derives
    // the bound)
    {1, 2, 2, false, "RV_MANY_CHAIN", &rv_many::chain, nullptr, nullptr, RV_LEAF_CHAIN_WMAX, false, MANY_PAIRS},
    // RV_MANY_CHAIN_MULTI, RV_MANY_CHAIN_WIDE: the jobs of several sequences the two forms of k_leaf_multi_chain finish.  As above, everything the kernel
    // leaves out has to be impossible for the job; none of the reasons depends on the number of sequences:
    //   trim on, minl > 0, gap model 0 .. 2     no p-value cut, no untrimmed lists
    //   weights 0 .. RV_LEAF_MCHAIN_WMAX        scores of up to 16 / 64 paths in 32 bits (rv_leaf_multi_chain.hip derives the bound for both forms)
    //   seedsize <= 0 or above the longest sequence   no match is that long: no seeds for the children
    //   maxmums <= 0 or >= the job's ranks      the cut is made on the matches of ONE sub-index, every one of them an inner node of the LCP-interval tree over the
    //                                           sub-index' ranks: a tree over len leaves has fewer than len inner nodes, and len <= the job's ranks <= 2048, so
    //                                           rem.align's default of 10 000 passes whatever the job
    {1, 3, RV_MANY_KMAX, false, "RV_MANY_CHAIN_MULTI", &rv_many::chain_multi, nullptr, nullptr, RV_LEAF_MCHAIN_WMAX, true, MANY_CONTIGUOUS},
    {1, RV_MANY_KMAX + 1, RV_MANY_WIDE_KMAX, false, "RV_MANY_CHAIN_WIDE", &rv_many::chain_wide, nullptr, nullptr, RV_LEAF_MCHAIN_WMAX, true, MANY_CONTIGUOUS},
    // RV_MANY_CHAIN_LARGE: the pair jobs above RV_LEAF_N ranks the level pipeline finishes, its picks made by k_pick_chain and k_leaf_chain.  RV_MANY_CHAIN's rule with
    //   weights 0 .. RV_PICK_CHAIN_WMAX = 1024               scores in 32 bits at 2^17 ranks (rv_pick_chain.hip derives the bound)
    //   seedsize <= 0 or above the longer sequence, maxmums <= 0 or at least the shorter one: as there
    // rem.align's defaults (10 000 / 10 000) admit every bubble `reveal refine` produces (alleles below 10 000 bases) and nothing with an allele of 10 000 or more.
    {1, 2, 2, true, "RV_MANY_CHAIN_LARGE", &rv_many::chain_large, "RV_MANY_CHAIN_LARGE_MIN", &rv_many::chain_large_min, RV_PICK_CHAIN_WMAX, false, MANY_PAIRS},
    // RV_MANY_CHAIN_LARGE_MULTI, RV_MANY_CHAIN_WIDE_LARGE: the jobs of several sequences above RV_LEAF_N ranks the multi-sample level pipeline finishes, its picks
    // made by the two forms of k_pick_multi_chain.  RV_MANY_CHAIN_MULTI's rule with
    //   weights 0 .. wmax                                     scores in 32 bits at 2^17 ranks: RV_PICK_MCHAIN_WMAX = 512 over 120 pairs (1024 does not hold),
    //                                                         RV_PICK_WCHAIN_WMAX = 128 over 2016 pairs (256 does not hold); rv_pick_multi_chain.hip derives both
    //   seedsize <= 0 or above the longest sequence, maxmums <= 0 or at least the job's ranks: as there
    // rem.align's default maxmums of 10 000 therefore admits jobs of up to 10 000 ranks only (and its seedsize no sequence of 10 000 bases or more).
    {1, 3, RV_MANY_KMAX, true, "RV_MANY_CHAIN_LARGE_MULTI", &rv_many::chain_large_multi, "RV_MANY_CHAIN_LARGE_MULTI_MIN", &rv_many::chain_large_multi_min, RV_PICK_MCHAIN_WMAX, true, MANY_SAMPLE_MAJOR},
    {1, RV_MANY_KMAX + 1, RV_MANY_WIDE_KMAX, true, "RV_MANY_CHAIN_WIDE_LARGE", &rv_many::chain_wide_large, "RV_MANY_CHAIN_WIDE_LARGE_MIN", &rv_many::chain_wide_large_min, RV_PICK_WCHAIN_WMAX, true, MANY_SAMPLE_MAJOR},
    // the built-in picker's classes behind the small pairs: pairs above RV_LEAF_N ranks, 3 .. 16 sequences below and above, 17 .. 64 sequences (one switch, RV_MANY_WIDE, for both sizes)
    {0, 2, 2, true, "RV_MANY_LARGE", &rv_many::large, "RV_MANY_LARGE_MIN", &rv_many::large_min, 0, false, MANY_PAIRS},
    {0, 3, RV_MANY_KMAX, false, "RV_MANY_MULTI", &rv_many::multi, nullptr, nullptr, 0, false, MANY_CONTIGUOUS},
    {0, 3, RV_MANY_KMAX, true, "RV_MANY_LARGE_MULTI", &rv_many::large_multi, "RV_MANY_LARGE_MULTI_MIN", &rv_many::large_multi_min, 0, false, MANY_SAMPLE_MAJOR},
    {0, RV_MANY_KMAX + 1, RV_MANY_WIDE_KMAX, false, "RV_MANY_WIDE", &rv_many::wide, nullptr, nullptr, 0, false, MANY_CONTIGUOUS},
    {0, RV_MANY_KMAX + 1, RV_MANY_WIDE_KMAX, true, "RV_MANY_WIDE", &rv_many::wide, "RV_MANY_WIDE_LARGE_MIN", &rv_many::wide_large_min, 0, false, MANY_SAMPLE_MAJOR},
};
constexpr int MANY_NCLASS = (int)(sizeof many_classes / sizeof many_classes[0]);

// whether job `jb` belongs to class `c` (lim: the round limit of the run) -- the rule of every class, stated once; many.takes_shared_launch mirrors it
bool many_class_admits(const rv_many *m, const ManyClass &c, const ManyJob &jb, int minl, int64_t lim) {
    if (m->picker != c.picker || (c.sw && !(m->*c.sw))) return false;
    if (jb.k < c.kmin || jb.k > c.kmax || !jb.clean) return false;
    if (!c.large) { if (jb.ranks > RV_LEAF_N) return false; }      // (a small job always fits a round: lim is not asked)
    else if (jb.ranks <= RV_LEAF_N || jb.ranks > m->large_max || jb.ranks > lim || (c.picker == 1 && jb.ranks > RV_PICK_CHAIN_RANKS)) return false;
    if (c.picker != 1) return true;
    const rv_picker_args &a = m->pargs;
    if (!a.trim || minl <= 0) return false;
    if (a.wscore < 0 || a.wpen < 0 || a.wscore > c.wmax || a.wpen > c.wmax) return false;
    if (a.gcmodel < 0 || a.gcmodel > 2) return false;
    int64_t longest = 0, shortest = INT64_MAX;
    for (int q = 0; q < jb.k; q++) { const int64_t len = m->lens[jb.seq0 + (size_t)q]; longest = std::max(longest, len); shortest = std::min(shortest, len); }
    if (a.seedsize > 0 && a.seedsize <= longest) return false;
    if (a.maxmums > 0 && a.maxmums < (c.by_ranks ? jb.ranks : shortest)) return false;
    return true;
}

// an order of jobs -> rounds: ascending size (ties as given), then as many jobs a round as stay within lim ranks, one at least; round(lo, hi) runs order[lo .. hi)
template <class Round>
int many_rounds(const rv_many *m, std::vector<int> &order, int64_t lim, Round round) {
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return m->jobs[(size_t)a].ranks < m->jobs[(size_t)b].ranks; });
    for (size_t lo = 0; lo < order.size();) {
        size_t hi = lo; int64_t sum = 0;
        while (hi < order.size() && (hi == lo || sum + m->jobs[(size_t)order[hi]].ranks <= lim)) sum += m->jobs[(size_t)order[hi++]].ranks;
        RV_TRY(round(lo, hi));
        lo = hi;
    }
    return 0;
}

// anchors of the handle's last run -> records of `job`, or (job < 0) of the job whose first sequence holds the first member
int many_collect(rv_many *m, rv_index *h, int job, const std::vector<int> &order, const std::vector<int64_t> &abeg, const std::vector<int64_t> &bbeg) {
    int64_t members = 0;
    const int64_t na = rv_anchor_count(h, &members);
    if (na < 0) return -1;
    std::vector<u32> l((size_t)std::max<int64_t>(na, 1));
    std::vector<int64_t> off((size_t)na + 1, 0), pos((size_t)std::max<int64_t>(members, 1));
    RV_TRY(rv_fetch_anchors(h, l.data(), off.data(), pos.data()));
    for (int64_t k = 0; k < na; k++) {
        ManyRec r; r.l = l[(size_t)k]; r.np = (int)(off[(size_t)k + 1] - off[(size_t)k]); r.p0 = (int64_t)m->rpos.size(); r.job = job;
        const int64_t *p = pos.data() + off[(size_t)k];
        if (job >= 0) {
            for (int q = 0; q < r.np; q++) m->rpos.push_back(p[q]);
        } else {
            if (r.np != 2) { rv_set_error("rv_many_run: an anchor of %d members in a pair job", r.np); return -1; }
            const size_t s = (size_t)(std::upper_bound(abeg.begin(), abeg.end(), p[0]) - abeg.begin()) - 1;
            if (s >= order.size()) { rv_set_error("rv_many_run: an anchor outside the text"); return -1; }
            const ManyJob &jb = m->jobs[(size_t)order[s]];
            const int64_t la = m->lens[jb.seq0], lb = m->lens[jb.seq0 + 1];
            const int64_t a = p[0] - abeg[s], b = p[1] - bbeg[s];
            if (a < 0 || a + r.l > la || b < 0 || b + r.l > lb) { rv_set_error("rv_many_run: an anchor outside its job"); return -1; }
            r.job = order[s];
            m->rpos.push_back(a); m->rpos.push_back(b + la + 1);      // stand-alone coordinates of `a$b$`
        }
        m->recs.push_back(r);
    }
    return 0;
}

void many_add_stats(rv_align_stats *t, const rv_align_stats &s) {
    if (!t) return;
    t->steps += s.steps; t->splits += s.splits; t->anchored_bp += s.anchored_bp; t->levels += s.levels;
    if (s.maxdepth > t->maxdepth) t->maxdepth = s.maxdepth;
    t->scanned_ranks += s.scanned_ranks; t->t_scan += s.t_scan; t->t_host += s.t_host; t->t_split += s.t_split; t->t_bubble += s.t_bubble;
}

// the index build of a round: the jobs [0, nsmall) a wavefront each, the others a workgroup each
int many_build(rv_many *m, hipStream_t q, const ManyDevJob *djobs, size_t J, size_t nsmall, const uint8_t *dT, u32 *d_max, u32 *d_err) {
    if (nsmall) {
        hipLaunchKernelGGL((k_many_build<CAP_S, 64>), dim3((unsigned)ceil_div((int64_t)nsmall, MT / 64)), dim3(MT), 0, q, djobs, (int)nsmall, dT,
                           m->dSA.as<sa_t>(), m->dLCP.as<lcp_t>(), m->dBWT.as<uint8_t>(), d_max, d_err);
        RV_LAUNCH_CHECK();
        m->info[4]++;
    }
    if (nsmall < J) {
        hipLaunchKernelGGL((k_many_build<CAP_L, MT>), dim3((unsigned)(J - nsmall)), dim3(MT), 0, q, djobs + nsmall, (int)(J - nsmall), dT,
                           m->dSA.as<sa_t>(), m->dLCP.as<lcp_t>(), m->dBWT.as<uint8_t>(), d_max, d_err);
        RV_LAUNCH_CHECK();
        m->info[4]++;
    }
    return 0;
}

// one round of the shared launches: the jobs order[lo .. hi) (ascending size); large: jobs above RV_LEAF_N ranks (RV_MANY_LARGE); redo != NULL: the
// round of picker kind 1 (RV_MANY_CHAIN; with large: RV_MANY_CHAIN_LARGE) -- its leaf launches are k_leaf_chain's, the picks of the level pipeline k_pick_chain's, and
// the jobs a launch of any level flags come back in *redo for the ordinary path
int many_round(rv_many *m, const std::vector<int> &order, size_t lo, size_t hi, int minl, int minn, rv_align_stats *total, bool large, std::vector<int> *redo = nullptr) {
    RV_TRY(many_handle(m, &m->hs));
    rv_index *h = m->hs;
    const size_t J = hi - lo;
    RV_TRY(rv_reset(h));
    if (redo) {
        RV_TRY(m->dFlag.reserve(J * sizeof(u32)));
        RV_HIP(hipMemsetAsync(m->dFlag.p, 0, J * sizeof(u32), h->ws.stream));
        if (m->chain_flag > 0) {      // test hook: every chain_flag-th job of the round counts as flagged by the kernel, whatever the kernel does with it
            std::vector<u32> pre(J, 0u);
            for (size_t s = 0; s < J; s += (size_t)m->chain_flag) pre[s] = 16u;
            RV_HIP(hipMemcpyAsync(m->dFlag.p, pre.data(), J * sizeof(u32), hipMemcpyHostToDevice, h->ws.stream));
            RV_HIP(hipStreamSynchronize(h->ws.stream));
        }
    }
    if (!redo) RV_TRY(rv_leaf_chain_route(h, nullptr, nullptr));
    // text: every first sequence, then every second one
    std::vector<int> ord(order.begin() + (ptrdiff_t)lo, order.begin() + (ptrdiff_t)hi);
    std::vector<int64_t> abeg(J), bbeg(J), la(J), lb(J);
    int64_t ta = 0, tb = 0;
    for (size_t s = 0; s < J; s++) {
        const ManyJob &jb = m->jobs[(size_t)ord[s]];
        la[s] = m->lens[jb.seq0]; lb[s] = m->lens[jb.seq0 + 1];
        abeg[s] = ta; ta += la[s] + 1; bbeg[s] = tb; tb += lb[s] + 1;
    }
    std::vector<char> buf((size_t)std::max(ta, tb));
    for (int side = 0; side < 2; side++) {
        int64_t at = 0;
        for (size_t s = 0; s < J; s++) {
            const ManyJob &jb = m->jobs[(size_t)ord[s]];
            const int64_t len = m->lens[jb.seq0 + (size_t)side];
            memcpy(buf.data() + at, m->in.data() + m->starts[jb.seq0 + (size_t)side], (size_t)len);
            buf[(size_t)(at + len)] = '$';
            at += len + 1;
        }
        RV_TRY(rv_add_sample(h));
        RV_TRY(rv_add_sequences(h, buf.data(), at, side == 0 ? la.data() : lb.data(), (int64_t)J));
    }
    for (size_t s = 0; s < J; s++) bbeg[s] += ta;
    const int64_t n = ta + tb;
    RV_TRY(rv_upload(h));
    if (redo) {      // the chain route: flags per job, a root or sub-index of any level finds its job among the text begins
        std::vector<int64_t> beg(abeg);
        beg.insert(beg.end(), bbeg.begin(), bbeg.end());
        RV_TRY(m->dBeg.reserve(2 * J * sizeof(int64_t)));
        RV_HIP(hipMemcpyAsync(m->dBeg.p, beg.data(), 2 * J * sizeof(int64_t), hipMemcpyHostToDevice, h->ws.stream));
        RV_HIP(hipStreamSynchronize(h->ws.stream));
        RV_TRY(rv_leaf_chain_route(h, &m->pargs, m->dFlag.as<u32>(), beg.data(), m->dBeg.as<int64_t>(), (int)J));
    }
    // jobs, segment offsets, frontier tables
    std::vector<ManyDevJob> dj(J);
    std::vector<int64_t> meta(6 * J), node_first(J + 1), nodes(4 * J);
    int64_t off = 0;
    size_t nsmall = 0;
    for (size_t s = 0; s < J; s++) {
        const int64_t r = la[s] + lb[s] + 2;
        dj[s].abeg = abeg[s]; dj[s].bbeg = bbeg[s]; dj[s].off = off; dj[s].la = (int32_t)la[s]; dj[s].lb = (int32_t)lb[s];
        int64_t *m6 = meta.data() + 6 * s;
        m6[0] = off; m6[1] = r; m6[2] = 0; m6[3] = 2; m6[4] = 0; m6[5] = -1;
        node_first[s] = (int64_t)(2 * s);
        nodes[4 * s] = abeg[s]; nodes[4 * s + 1] = abeg[s] + la[s]; nodes[4 * s + 2] = bbeg[s]; nodes[4 * s + 3] = bbeg[s] + lb[s];
        if (r <= m->wave_max && r <= CAP_S) nsmall = s + 1;      // (ascending sizes: the small class is a prefix)
        off += r;
    }
    node_first[J] = (int64_t)(2 * J);
    if (off != n) { rv_set_error("rv_many_run: the jobs' ranks do not add up to the text"); return -1; }
    hipStream_t q = h->ws.stream;
    RV_TRY(m->dJobs.reserve(J * sizeof(ManyDevJob)));
    RV_TRY(m->dSA.reserve((size_t)(n + 64) * sizeof(sa_t)));
    RV_TRY(m->dLCP.reserve((size_t)(n + 64) * sizeof(lcp_t)));
    RV_TRY(m->dBWT.reserve((size_t)n + 64));
    RV_TRY(m->dCnt.reserve(64));
    RV_HIP(hipMemcpyAsync(m->dJobs.p, dj.data(), J * sizeof(ManyDevJob), hipMemcpyHostToDevice, q));
    RV_HIP(hipMemsetAsync(m->dCnt.p, 0, 64, q));
    u32 *d_max = m->dCnt.as<u32>(), *d_err = d_max + 1;
    const ManyDevJob *djobs = m->dJobs.as<ManyDevJob>();
    const uint8_t *dT = h->dT0.as<uint8_t>();
    if (large) {
        RV_TRY(rv_many_large_build(h->ws, m->large_bufs, djobs, (int64_t)J, n, la[J - 1] + lb[J - 1] + 2, dT, m->dSA.as<sa_t>(), m->dLCP.as<lcp_t>(), m->dBWT.as<uint8_t>(), d_max, &m->info[4]));
    } else RV_TRY(many_build(m, q, djobs, J, nsmall, dT, d_max, d_err));
    u32 cnt[2] = {0, 0};
    RV_TRY(rv_read_back(h->ws, cnt, d_max, 8));
    if (cnt[1]) { rv_set_error("rv_many_run: the index build refused a job (error bits %u)", cnt[1]); return -1; }
    if (m->keep) {
        // test hook: SA / LCP of every job in job-local positions
        std::vector<sa_t> sa((size_t)n); std::vector<lcp_t> lc((size_t)n);
        RV_HIP(hipMemcpy(sa.data(), m->dSA.p, (size_t)n * sizeof(sa_t), hipMemcpyDeviceToHost));
        RV_HIP(hipMemcpy(lc.data(), m->dLCP.p, (size_t)n * sizeof(lcp_t), hipMemcpyDeviceToHost));
        const size_t base = m->keep_sa.size();
        m->keep_sa.resize(base + (size_t)n); m->keep_lcp.resize(base + (size_t)n);
        for (size_t s = 0; s < J; s++) {
            m->jobs[(size_t)ord[s]].arr_off = (int64_t)base + dj[s].off;
            for (int64_t r = 0; r < la[s] + lb[s] + 2; r++) {
                const int64_t p = (int64_t)sa[(size_t)(dj[s].off + r)];
                m->keep_sa[base + (size_t)(dj[s].off + r)] = (sa_t)(p >= bbeg[s] ? p - bbeg[s] + la[s] + 1 : p - abeg[s]);
                m->keep_lcp[base + (size_t)(dj[s].off + r)] = lc[(size_t)(dj[s].off + r)];
            }
        }
    }
    // the segments as a frontier of J roots; every root is leaf-sized: one leaf launch (large: the level pipeline, leaves as the children shrink)
    RV_TRY(rv_frontier_import(h, minl, minn, cnt[0], 0, (int)J, meta.data(), node_first.data(), nodes.data(), n, m->dSA.p, m->dLCP.p, m->dBWT.p, 1));
    rv_align_stats st;
    memset(&st, 0, sizeof st);
    RV_TRY(rv_align_builtin_resume(h, &st));
    many_add_stats(total, st);
    const size_t rec0 = m->recs.size();
    RV_TRY(many_collect(m, h, -1, ord, abeg, bbeg));
    m->info[4] += st.levels + (m->recs.size() > rec0 ? 2 : 0);      // leaf launches (large: levels), and the two of the lower-casing when there are anchors
    std::vector<u32> flag;
    size_t nflag = 0;
    if (redo) {
        // the jobs the kernel did not finish: their anchors are dropped, their text is not taken from the round
        // (every job of a small round is a root of its one chain leaf launch; every job of a large round is above RV_LEAF_N ranks, so the level pipeline's
        // chain pick was asked for each of the J roots at least -- or the host's picker, at a level without device tables -- and never the longest match)
        if (!large && rv_leaf_chain_roots(h) != (int64_t)J) { rv_set_error("rv_many_run: the chain leaf launch took %lld of the round's %lld jobs", (long long)rv_leaf_chain_roots(h), (long long)J); return -1; }
        const int *hflag = nullptr;
        const int nhflag = rv_leaf_chain_host_flags(h, &hflag);
        if (large && rv_pick_chain_subs(h) < (int64_t)J) { rv_set_error("rv_many_run: the chain pick took %lld sub-indices of a round of %lld jobs", (long long)rv_pick_chain_subs(h), (long long)J); return -1; }
        flag.resize(J);
        RV_HIP(hipMemcpy(flag.data(), m->dFlag.p, J * sizeof(u32), hipMemcpyDeviceToHost));
        for (int k = 0; k < nhflag; k++) if (hflag[k] >= 0 && (size_t)hflag[k] < J) flag[(size_t)hflag[k]] |= 128u;
        std::vector<char> out((size_t)m->jobs.size(), 0);
        for (size_t s = 0; s < J; s++) if (flag[s]) { out[(size_t)ord[s]] = 1; redo->push_back(ord[s]); nflag++; many_count_flags(m, flag[s]); }
        if (nflag) m->recs.erase(std::remove_if(m->recs.begin() + (ptrdiff_t)rec0, m->recs.end(), [&](const ManyRec &r) { return out[(size_t)r.job] != 0; }), m->recs.end());
    }
    // final text of every job: a$b$
    std::vector<char> txt((size_t)n);
    RV_TRY(rv_ensure_working_text(h));
    RV_HIP(hipStreamSynchronize(h->ws.stream));
    RV_HIP(hipMemcpy(txt.data(), h->dT.p, (size_t)n, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < J; s++) {
        if (nflag && flag[s]) continue;
        ManyJob &jb = m->jobs[(size_t)ord[s]];
        jb.text_off = (int64_t)m->out_text.size();
        jb.shared = true;
        m->out_text.insert(m->out_text.end(), txt.begin() + (ptrdiff_t)abeg[s], txt.begin() + (ptrdiff_t)(abeg[s] + la[s] + 1));
        m->out_text.insert(m->out_text.end(), txt.begin() + (ptrdiff_t)bbeg[s], txt.begin() + (ptrdiff_t)(bbeg[s] + lb[s] + 1));
    }
    m->info[1] += (int64_t)(J - nflag); m->info[3]++;
    return 0;
}

// one round of jobs of three and more sequences (RV_MANY_MULTI): the jobs order[lo .. hi) (ascending size).  Every job is laid out
// contiguously, s0$s1$..s(k-1)$, job after job: a job's ranks lie where its text lies, and a position minus the job's begin is its
// stand-alone coordinate.  k_many_build sees such a job as its first sequence and "the rest" (the side bit of the BWT byte means
// nothing here); k_leaf_multi then finishes every job in one workgroup and lower-cases its text.  No handle is involved beyond
// the stream and the read-back buffer of the shared one: the launches of a round do not depend on the number of jobs.
// kmax: the sample bound of the round's class and the form of k_leaf_multi that takes it -- RV_MANY_KMAX, or RV_MANY_WIDE_KMAX for the
// rounds of jobs of 17 .. 64 sequences (RV_MANY_WIDE).  redo != NULL: the round of picker kind 1 (RV_MANY_CHAIN_MULTI with kmax = RV_MANY_KMAX, RV_MANY_CHAIN_WIDE
// with kmax = RV_MANY_WIDE_KMAX) -- its leaf launch is that form of k_leaf_multi_chain, and the jobs that kernel flags come back in *redo for the ordinary path: their anchors are dropped, their text is not taken
int many_round_multi(rv_many *m, const std::vector<int> &order, size_t lo, size_t hi, int minl, int minn, rv_align_stats *total, int kmax, std::vector<int> *redo = nullptr) {
    RV_TRY(many_handle(m, &m->hs));
    rv_index *h = m->hs;
    const size_t J = hi - lo;
    std::vector<ManyDevJob> dj(J);
    std::vector<RvLeafMultiJob> mj(J);
    int64_t n = 0;
    size_t nsmall = 0;
    for (size_t s = 0; s < J; s++) {
        const ManyJob &jb = m->jobs[(size_t)order[lo + s]];
        if (jb.k < 3 || jb.k > kmax || jb.ranks > CAP_L) { rv_set_error("rv_many_run: a job of %d sequences in a round of at most %d", jb.k, kmax); return -1; }
        n += jb.ranks;
    }
    std::vector<char> txt((size_t)n);
    int64_t at = 0;
    for (size_t s = 0; s < J; s++) {
        const ManyJob &jb = m->jobs[(size_t)order[lo + s]];
        const int64_t la = m->lens[jb.seq0];
        dj[s].abeg = at; dj[s].bbeg = at + la + 1; dj[s].off = at; dj[s].la = (int32_t)la; dj[s].lb = (int32_t)(jb.ranks - la - 2);
        mj[s].beg = at; mj[s].n = (int32_t)jb.ranks; mj[s].pad = 0;
        if (jb.ranks <= m->wave_max && jb.ranks <= CAP_S) nsmall = s + 1;      // (ascending sizes: the small class is a prefix)
        for (int q = 0; q < jb.k; q++) {
            const int64_t len = m->lens[jb.seq0 + (size_t)q];
            memcpy(txt.data() + at, m->in.data() + m->starts[jb.seq0 + (size_t)q], (size_t)len);
            txt[(size_t)(at + len)] = '$';
            at += len + 1;
        }
    }
    if (at != n) { rv_set_error("rv_many_run: the jobs' ranks do not add up to the text"); return -1; }
    hipStream_t q = h->ws.stream;
    // anchors cover disjoint text, and a member at least one position: at most n members, n / 2 anchors
    const u32 acap = (u32)(n / 2 + 1), mcap = (u32)n;
    RV_TRY(m->dJobs.reserve(J * sizeof(ManyDevJob)));
    RV_TRY(m->dMJobs.reserve(J * sizeof(RvLeafMultiJob)));
    RV_TRY(m->dTxt.reserve((size_t)n + 64));
    RV_TRY(m->dSA.reserve((size_t)(n + 64) * sizeof(sa_t)));
    RV_TRY(m->dLCP.reserve((size_t)(n + 64) * sizeof(lcp_t)));
    RV_TRY(m->dBWT.reserve((size_t)n + 64));
    RV_TRY(m->dAn.reserve((size_t)acap * sizeof(RvLeafMultiAnchor)));
    RV_TRY(m->dAnPos.reserve((size_t)mcap * sizeof(uint16_t)));
    RV_TRY(m->dCnt.reserve(64));
    RV_HIP(hipMemcpyAsync(m->dJobs.p, dj.data(), J * sizeof(ManyDevJob), hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(m->dMJobs.p, mj.data(), J * sizeof(RvLeafMultiJob), hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(m->dTxt.p, txt.data(), (size_t)n, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemsetAsync(m->dCnt.p, 0, 64, q));
    // dCnt: [0] max LCP, [1] error bits of the build, [2] of the leaf kernel, [4..5] anchors << 32 | members, [6..13] statistics
    u32 *d_max = m->dCnt.as<u32>(), *d_err = d_max + 1;
    RV_TRY(many_build(m, q, m->dJobs.as<ManyDevJob>(), J, nsmall, m->dTxt.as<uint8_t>(), d_max, d_err));
    RvLeafMultiArgs a;
    a.jobs = m->dMJobs.as<RvLeafMultiJob>();
    a.SA = m->dSA.as<sa_t>(); a.LCP = m->dLCP.as<lcp_t>(); a.BWT = m->dBWT.as<uint8_t>(); a.T = m->dTxt.as<uint8_t>();
    a.minl = minl; a.minn = minn; a.stage_cap = (u32)std::min<int64_t>(m->stage, 256);
    a.count = (unsigned long long *)(d_max + 4); a.anchor_cap = acap; a.member_cap = mcap;
    a.anchors = m->dAn.as<RvLeafMultiAnchor>(); a.an_pos = m->dAnPos.as<uint16_t>();
    a.stats = (unsigned long long *)(d_max + 6); a.err = d_max + 2;
    if (redo) {
        for (auto &o : m->fwd) if (o.first == "RV_LEAF_ACAP" && o.second >= 0) a.stage_cap = (u32)std::min<int64_t>(a.stage_cap, o.second);      // (test hook, as for k_leaf_chain)
        std::vector<u32> pre(J, 0u);
        if (m->chain_flag > 0) for (size_t s = 0; s < J; s += (size_t)m->chain_flag) pre[s] = 16u;      // test hook: every chain_flag-th job of the round counts as flagged
        RV_TRY(m->dFlag.reserve(J * sizeof(u32)));
        RV_HIP(hipMemcpyAsync(m->dFlag.p, pre.data(), J * sizeof(u32), hipMemcpyHostToDevice, q));
        RV_HIP(hipStreamSynchronize(q));
        RvLeafMultiChainArgs c;
        c.wscore = (int32_t)m->pargs.wscore; c.wpen = (int32_t)m->pargs.wpen; c.gcmodel = m->pargs.gcmodel; c.flags = m->dFlag.as<u32>();
        RV_TRY(rv_leaf_multi_chain_launch(q, a, c, (int)J, kmax));
    } else
    RV_TRY(rv_leaf_multi_launch(q, a, (int)J, kmax));
    m->info[4]++;
    u32 cnt[16];
    RV_TRY(rv_read_back(h->ws, cnt, d_max, sizeof cnt));
    if (cnt[1]) { rv_set_error("rv_many_run: the index build refused a job (error bits %u)", cnt[1]); return -1; }
    if (cnt[2]) { rv_set_error("rv_many_run: the leaf kernel for jobs of several sequences failed (error bits %u: 4 stack, 8 intervals, 16 job, 32 output)", cnt[2]); return -1; }
    unsigned long long both, st4[4];
    memcpy(&both, cnt + 4, 8); memcpy(st4, cnt + 6, 32);
    const size_t na = (size_t)(both >> 32), nm = (size_t)(both & 0xFFFFFFFFull);
    if (na > acap || nm > mcap) { rv_set_error("rv_many_run: more anchors than the text has room for"); return -1; }
    std::vector<RvLeafMultiAnchor> an(std::max<size_t>(na, 1)); std::vector<uint16_t> ap(std::max<size_t>(nm, 1));
    std::vector<sa_t> sa; std::vector<lcp_t> lc;
    if (na) RV_HIP(hipMemcpyAsync(an.data(), m->dAn.p, na * sizeof(RvLeafMultiAnchor), hipMemcpyDeviceToHost, q));
    if (nm) RV_HIP(hipMemcpyAsync(ap.data(), m->dAnPos.p, nm * sizeof(uint16_t), hipMemcpyDeviceToHost, q));
    std::vector<u32> flag;
    size_t nflag = 0;
    if (redo) { flag.resize(J); RV_HIP(hipMemcpyAsync(flag.data(), m->dFlag.p, J * sizeof(u32), hipMemcpyDeviceToHost, q)); }
    if (m->keep) {
        sa.resize((size_t)n); lc.resize((size_t)n);
        RV_HIP(hipMemcpyAsync(sa.data(), m->dSA.p, (size_t)n * sizeof(sa_t), hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(lc.data(), m->dLCP.p, (size_t)n * sizeof(lcp_t), hipMemcpyDeviceToHost, q));
    }
    const size_t tbase = m->out_text.size();
    m->out_text.resize(tbase + (size_t)n);
    RV_HIP(hipMemcpyAsync(m->out_text.data() + tbase, m->dTxt.p, (size_t)n, hipMemcpyDeviceToHost, q));
    RV_HIP(hipStreamSynchronize(q));
    if (redo) for (size_t s = 0; s < J; s++) if (flag[s]) { redo->push_back(order[lo + s]); nflag++; many_count_flags(m, flag[s]); }
    for (size_t k = 0; k < na; k++) {
        const RvLeafMultiAnchor &r = an[k];
        if (r.job >= J || r.n < 2 || r.n > (u32)kmax || (size_t)r.moff + r.n > nm) { rv_set_error("rv_many_run: a malformed anchor"); return -1; }
        if (nflag && flag[r.job]) continue;      // (a job the kernel did not finish)
        const int64_t ranks = mj[r.job].n;
        ManyRec rec; rec.job = order[lo + r.job]; rec.l = r.l; rec.np = (int)r.n; rec.p0 = (int64_t)m->rpos.size();
        for (u32 x = 0; x < r.n; x++) {
            const int64_t p = ap[(size_t)r.moff + x];
            if (p + r.l > ranks) { rv_set_error("rv_many_run: an anchor outside its job"); return -1; }
            m->rpos.push_back(p);
        }
        m->recs.push_back(rec);
    }
    const size_t kbase = m->keep_sa.size();
    if (m->keep) {
        // test hook: SA / LCP of every job in job-local positions
        m->keep_sa.resize(kbase + (size_t)n); m->keep_lcp.resize(kbase + (size_t)n);
        for (size_t s = 0; s < J; s++)
            for (int64_t r = mj[s].beg; r < mj[s].beg + mj[s].n; r++) { m->keep_sa[kbase + (size_t)r] = (sa_t)(sa[(size_t)r] - (sa_t)mj[s].beg); m->keep_lcp[kbase + (size_t)r] = lc[(size_t)r]; }
    }
    for (size_t s = 0; s < J; s++) {
        if (nflag && flag[s]) continue;
        ManyJob &jb = m->jobs[(size_t)order[lo + s]];
        jb.text_off = (int64_t)tbase + mj[s].beg; jb.shared = true;
        if (m->keep) jb.arr_off = (int64_t)kbase + mj[s].beg;
    }
    rv_align_stats st;
    memset(&st, 0, sizeof st);
    st.steps = (int64_t)st4[0]; st.splits = (int64_t)st4[1]; st.anchored_bp = (int64_t)st4[2]; st.maxdepth = (int)st4[3]; st.levels = 1; st.scanned_ranks = n;
    many_add_stats(total, st);
    m->info[1] += (int64_t)(J - nflag); m->info[3]++;
    return 0;
}

// a sample-major round (RV_MANY_LARGE_MULTI): where its jobs lie.  dj[s]: job ord[s] (begins in the shared text, local prefix ends); send[q]: the
// '$' behind the last sequence of sample q (the handle's nsep[q]); sbeg[q] / sslot[q]: begin and slot of the sequences of sample q, ascending
struct ManyRoundK {
    std::vector<int> ord;
    std::vector<ManyDevJobK> dj;
    std::vector<int64_t> send;
    std::vector<std::vector<int64_t>> sbeg;
    std::vector<std::vector<int>> sslot;
    // shared position inside sequence q of slot s -> stand-alone coordinate of the job's text s0$s1$..
    int64_t local(size_t s, int q, int64_t p) const { return p - dj[s].beg[q] + (q ? dj[s].pend[q - 1] : 0); }
    int sample_of(int64_t p) const { return (int)(std::lower_bound(send.begin(), send.end(), p) - send.begin()); }
};

// anchors of the handle's last run over a sample-major round -> records of their jobs.  An anchor's job comes from its first member (search among
// the begins of that member's sample), every member maps back to the job's stand-alone coordinate.  The map is strictly increasing, so the members
// stay in the (sorted) order rv_fetch_anchors gives a stand-alone index.
// picker_order: the round of picker kind 1 -- the members come in the picker's order (the scan's member order), which the map keeps as well; they only
// have to differ
int many_collect_k(rv_many *m, rv_index *h, const ManyRoundK &R, bool picker_order = false) {
    int64_t members = 0;
    const int64_t na = rv_anchor_count(h, &members);
    if (na < 0) return -1;
    std::vector<u32> l((size_t)std::max<int64_t>(na, 1));
    std::vector<int64_t> off((size_t)na + 1, 0), pos((size_t)std::max<int64_t>(members, 1));
    RV_TRY(rv_fetch_anchors(h, l.data(), off.data(), pos.data()));
    const int K = (int)R.send.size();
    for (int64_t k = 0; k < na; k++) {
        ManyRec r; r.l = l[(size_t)k]; r.np = (int)(off[(size_t)k + 1] - off[(size_t)k]); r.p0 = (int64_t)m->rpos.size();
        const int64_t *p = pos.data() + off[(size_t)k];
        if (r.np < 2 || r.np > K) { rv_set_error("rv_many_run: an anchor of %d members in a round of %d samples", r.np, K); return -1; }
        const int q0 = R.sample_of(p[0]);
        if (q0 >= K) { rv_set_error("rv_many_run: an anchor outside the text"); return -1; }
        const size_t at = (size_t)(std::upper_bound(R.sbeg[(size_t)q0].begin(), R.sbeg[(size_t)q0].end(), p[0]) - R.sbeg[(size_t)q0].begin());
        if (at == 0) { rv_set_error("rv_many_run: an anchor outside the text"); return -1; }
        const size_t s = (size_t)R.sslot[(size_t)q0][at - 1];
        const ManyDevJobK &J = R.dj[s];
        int64_t last = -1; u64 seen = 0;
        for (int x = 0; x < r.np; x++) {
            const int q = R.sample_of(p[x]);
            if (q >= J.k) { rv_set_error("rv_many_run: an anchor outside its job"); return -1; }
            const int64_t lo = q ? J.pend[q - 1] : 0, loc = R.local(s, q, p[x]);
            if (loc < lo || loc + r.l > J.pend[q] - 1 || (picker_order ? ((seen >> q) & 1ull) != 0 : loc <= last)) { rv_set_error("rv_many_run: an anchor outside its job"); return -1; }
            seen |= 1ull << q;
            m->rpos.push_back(loc);
            last = loc;
        }
        r.job = R.ord[s];
        m->recs.push_back(r);
    }
    return 0;
}

// one round of jobs of three and more sequences above RV_LEAF_N ranks (RV_MANY_LARGE_MULTI): the jobs order[lo .. hi) (ascending size), k mixed.
// The sample-major text goes into the shared handle (K samples, K the widest job), the index of every job is built at once
// (rv_many_large_build_k), the segments become a level-0 frontier of J roots of k samples each, and the level pipeline finishes them together.
// kmax: the sample bound of the round's class (RV_MANY_KMAX; RV_MANY_WIDE_KMAX for the rounds of jobs of 17 .. 64 sequences, RV_MANY_WIDE).
// redo != NULL: the round of picker kind 1 (RV_MANY_CHAIN_LARGE_MULTI with kmax = RV_MANY_KMAX, RV_MANY_CHAIN_WIDE_LARGE with kmax = RV_MANY_WIDE_KMAX: the
// form of k_pick_multi_chain that takes it) -- the level pipeline runs under the multi-sample chain route
// (rv_multi_chain_route: every sub-index picked by k_pick_multi_chain, or by the host's picker at a level without device tables), and the jobs a launch of
// any level flags come back in *redo for the ordinary path: their anchors are dropped, their text is not taken
int many_round_large_multi(rv_many *m, const std::vector<int> &order, size_t lo, size_t hi, int minl, int minn, rv_align_stats *total, int kmax, std::vector<int> *redo = nullptr) {
    RV_TRY(many_handle(m, &m->hs));
    rv_index *h = m->hs;
    const size_t J = hi - lo;
    RV_TRY(rv_reset(h));
    if (redo) {
        RV_TRY(m->dFlag.reserve(J * sizeof(u32)));
        RV_HIP(hipMemsetAsync(m->dFlag.p, 0, J * sizeof(u32), h->ws.stream));
        if (m->chain_flag > 0) {      // test hook: every chain_flag-th job of the round counts as flagged by the kernel, whatever the kernel does with it
            std::vector<u32> pre(J, 0u);
            for (size_t s = 0; s < J; s += (size_t)m->chain_flag) pre[s] = 16u;
            RV_HIP(hipMemcpyAsync(m->dFlag.p, pre.data(), J * sizeof(u32), hipMemcpyHostToDevice, h->ws.stream));
            RV_HIP(hipStreamSynchronize(h->ws.stream));
        }
    } else RV_TRY(rv_multi_chain_route(h, nullptr, nullptr));
    ManyRoundK R;
    R.ord.assign(order.begin() + (ptrdiff_t)lo, order.begin() + (ptrdiff_t)hi);
    R.dj.resize(J);
    int K = 0;
    for (size_t s = 0; s < J; s++) K = std::max(K, m->jobs[(size_t)R.ord[s]].k);
    if (K < 3 || K > kmax || kmax > RV_MANY_WIDE_KMAX) { rv_set_error("rv_many_run: a round of jobs of %d sequences", K); return -1; }
    R.send.resize((size_t)K); R.sbeg.resize((size_t)K); R.sslot.resize((size_t)K);
    // text: sample q = the q-th sequence of every job that has one
    std::vector<char> buf;
    std::vector<int64_t> lens;
    int64_t n = 0, maxn = 0, nnodes = 0;
    for (int q = 0; q < K; q++) {
        buf.clear(); lens.clear();
        for (size_t s = 0; s < J; s++) {
            const ManyJob &jb = m->jobs[(size_t)R.ord[s]];
            if (q >= jb.k) continue;
            const int64_t len = m->lens[jb.seq0 + (size_t)q];
            R.dj[s].beg[q] = n + (int64_t)buf.size();
            R.sbeg[(size_t)q].push_back(R.dj[s].beg[q]); R.sslot[(size_t)q].push_back((int)s);
            const char *src = m->in.data() + m->starts[jb.seq0 + (size_t)q];
            buf.insert(buf.end(), src, src + len);
            buf.push_back('$');
            lens.push_back(len);
        }
        RV_TRY(rv_add_sample(h));
        RV_TRY(rv_add_sequences(h, buf.data(), (int64_t)buf.size(), lens.data(), (int64_t)lens.size()));
        n += (int64_t)buf.size();
        R.send[(size_t)q] = n - 1;
    }
    RV_TRY(rv_upload(h));
    if (redo) {
        // the chain route: flags per job; a sub-index of any level finds its job in the row of its lowest live sample -- where sequence q of every job
        // begins, ascending (a job without a q-th sequence stands at the begin of the next one that has it)
        // (K <= kmax was checked above: a chain round of more than RV_MANY_KMAX rows exists for the class of the kernel's 64-sample form only)
        if (kmax != RV_MANY_KMAX && kmax != RV_MANY_WIDE_KMAX) { rv_set_error("rv_many_run: a chain round of a class of %d sequences", kmax); return -1; }
        std::vector<int64_t> beg((size_t)K * J);
        for (int q2 = 0; q2 < K; q2++) {
            int64_t nxt = R.send[(size_t)q2];
            for (size_t s = J; s-- > 0;) {
                if (q2 < m->jobs[(size_t)R.ord[s]].k) nxt = R.dj[s].beg[q2];
                beg[(size_t)q2 * J + s] = nxt;
            }
        }
        RV_TRY(m->dBeg.reserve(beg.size() * sizeof(int64_t)));
        RV_HIP(hipMemcpyAsync(m->dBeg.p, beg.data(), beg.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->ws.stream));
        RV_HIP(hipStreamSynchronize(h->ws.stream));
        RV_TRY(rv_multi_chain_route(h, &m->pargs, m->dFlag.as<u32>(), beg.data(), m->dBeg.as<int64_t>(), (int)J, K, kmax));
    }
    // jobs, segment offsets, frontier tables
    std::vector<int64_t> meta(6 * J), node_first(J + 1);
    int64_t off = 0;
    for (size_t s = 0; s < J; s++) {
        const ManyJob &jb = m->jobs[(size_t)R.ord[s]];
        ManyDevJobK &d = R.dj[s];
        d.off = off; d.k = jb.k; d.n = (int32_t)jb.ranks;
        int64_t pe = 0;
        for (int q = 0; q < RV_MANY_WIDE_KMAX; q++) {
            if (q < jb.k) pe += m->lens[jb.seq0 + (size_t)q] + 1; else d.beg[q] = 0;
            d.pend[q] = (int32_t)pe;
        }
        if (pe != jb.ranks) { rv_set_error("rv_many_run: the lengths of a job do not add up to its ranks"); return -1; }
        int64_t *m6 = meta.data() + 6 * s;
        m6[0] = off; m6[1] = jb.ranks; m6[2] = 0; m6[3] = jb.k; m6[4] = 0; m6[5] = -1;
        node_first[s] = nnodes; nnodes += jb.k;
        maxn = std::max(maxn, jb.ranks);
        off += jb.ranks;
    }
    node_first[J] = nnodes;
    if (off != n) { rv_set_error("rv_many_run: the jobs' ranks do not add up to the text"); return -1; }
    std::vector<int64_t> nodes((size_t)(2 * nnodes));
    for (size_t s = 0; s < J; s++)
        for (int q = 0; q < R.dj[s].k; q++) {
            const size_t x = (size_t)(2 * (node_first[s] + q));
            nodes[x] = R.dj[s].beg[q]; nodes[x + 1] = R.dj[s].beg[q] + (R.dj[s].pend[q] - (q ? R.dj[s].pend[q - 1] : 0) - 1);
        }
    hipStream_t q = h->ws.stream;
    RV_TRY(m->dKJobs.reserve(J * sizeof(ManyDevJobK)));
    RV_TRY(m->dSA.reserve((size_t)(n + 64) * sizeof(sa_t)));
    RV_TRY(m->dLCP.reserve((size_t)(n + 64) * sizeof(lcp_t)));
    RV_TRY(m->dBWT.reserve((size_t)n + 64));
    RV_TRY(m->dCnt.reserve(64));
    RV_HIP(hipMemcpyAsync(m->dKJobs.p, R.dj.data(), J * sizeof(ManyDevJobK), hipMemcpyHostToDevice, q));
    RV_HIP(hipMemsetAsync(m->dCnt.p, 0, 64, q));
    u32 *d_max = m->dCnt.as<u32>();
    RV_TRY(rv_many_large_build_k(h->ws, m->large_bufs, m->dKJobs.as<ManyDevJobK>(), (int64_t)J, n, maxn, h->dT0.as<uint8_t>(), n, m->dSA.as<sa_t>(), m->dLCP.as<lcp_t>(),
                                 m->dBWT.as<uint8_t>(), d_max, &m->info[4]));
    u32 cnt[2] = {0, 0};
    RV_TRY(rv_read_back(h->ws, cnt, d_max, 8));
    if (cnt[1]) { rv_set_error("rv_many_run: the index build refused a job (error bits %u)", cnt[1]); return -1; }
    if (m->keep) {
        // test hook: SA / LCP of every job in job-local positions
        std::vector<sa_t> sa((size_t)n); std::vector<lcp_t> lc((size_t)n);
        RV_HIP(hipMemcpy(sa.data(), m->dSA.p, (size_t)n * sizeof(sa_t), hipMemcpyDeviceToHost));
        RV_HIP(hipMemcpy(lc.data(), m->dLCP.p, (size_t)n * sizeof(lcp_t), hipMemcpyDeviceToHost));
        const size_t base = m->keep_sa.size();
        m->keep_sa.resize(base + (size_t)n); m->keep_lcp.resize(base + (size_t)n);
        for (size_t s = 0; s < J; s++) {
            m->jobs[(size_t)R.ord[s]].arr_off = (int64_t)base + R.dj[s].off;
            for (int64_t r = R.dj[s].off; r < R.dj[s].off + R.dj[s].n; r++) {
                const int64_t p = (int64_t)sa[(size_t)r];
                const int sq = R.sample_of(p);
                if (sq >= R.dj[s].k) { rv_set_error("rv_many_run: a suffix outside its job"); return -1; }
                m->keep_sa[base + (size_t)r] = (sa_t)R.local(s, sq, p);
                m->keep_lcp[base + (size_t)r] = lc[(size_t)r];
            }
        }
    }
    RV_TRY(rv_frontier_import(h, minl, minn, cnt[0], 0, (int)J, meta.data(), node_first.data(), nodes.data(), n, m->dSA.p, m->dLCP.p, m->dBWT.p, 1));
    rv_align_stats st;
    memset(&st, 0, sizeof st);
    RV_TRY(rv_align_builtin_resume(h, &st));
    many_add_stats(total, st);
    const size_t rec0 = m->recs.size();
    RV_TRY(many_collect_k(m, h, R, redo != nullptr));
    m->info[4] += st.levels + (m->recs.size() > rec0 ? 2 : 0);      // one per level, and the two of the lower-casing when there are anchors
    std::vector<u32> flag;
    size_t nflag = 0;
    if (redo) {
        // the jobs a kernel (or the host's picker) did not finish: their anchors are dropped, their text is not taken from the round.  Every job is a root of
        // level 0 at least: the picker -- never the longest match -- was asked for each of them
        const int *hflag = nullptr;
        const int nhflag = rv_leaf_chain_host_flags(h, &hflag);
        if (rv_pick_chain_subs(h) < (int64_t)J) { rv_set_error("rv_many_run: the chain pick took %lld sub-indices of a round of %lld jobs", (long long)rv_pick_chain_subs(h), (long long)J); return -1; }
        flag.resize(J);
        RV_HIP(hipMemcpy(flag.data(), m->dFlag.p, J * sizeof(u32), hipMemcpyDeviceToHost));
        for (int k = 0; k < nhflag; k++) if (hflag[k] >= 0 && (size_t)hflag[k] < J) flag[(size_t)hflag[k]] |= 128u;
        std::vector<char> out((size_t)m->jobs.size(), 0);
        for (size_t s = 0; s < J; s++) if (flag[s]) { out[(size_t)R.ord[s]] = 1; redo->push_back(R.ord[s]); nflag++; many_count_flags(m, flag[s]); }
        if (nflag) m->recs.erase(std::remove_if(m->recs.begin() + (ptrdiff_t)rec0, m->recs.end(), [&](const ManyRec &r) { return out[(size_t)r.job] != 0; }), m->recs.end());
    }
    // final text of every job, gathered from its k places
    std::vector<char> txt((size_t)n);
    RV_TRY(rv_ensure_working_text(h));
    RV_HIP(hipStreamSynchronize(h->ws.stream));
    RV_HIP(hipMemcpy(txt.data(), h->dT.p, (size_t)n, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < J; s++) {
        if (nflag && flag[s]) continue;
        ManyJob &jb = m->jobs[(size_t)R.ord[s]];
        jb.text_off = (int64_t)m->out_text.size();
        jb.shared = true;
        for (int sq = 0; sq < jb.k; sq++) {
            const int64_t b = R.dj[s].beg[sq], len1 = R.dj[s].pend[sq] - (sq ? R.dj[s].pend[sq - 1] : 0);
            m->out_text.insert(m->out_text.end(), txt.begin() + (ptrdiff_t)b, txt.begin() + (ptrdiff_t)(b + len1));
        }
    }
    m->info[1] += (int64_t)(J - nflag); m->info[3]++;
    return 0;
}

// a job the shared launches do not take: construct() + rv_align_builtin on the reused handle, every sequence a sample
int many_ordinary(rv_many *m, int job, int minl, int minn, rv_align_stats *total) {
    RV_TRY(many_handle(m, &m->ho));
    rv_index *h = m->ho;
    ManyJob &jb = m->jobs[(size_t)job];
    RV_TRY(rv_reset(h));
    for (int s = 0; s < jb.k; s++) {
        RV_TRY(rv_add_sample(h));
        RV_TRY(rv_add_sequence(h, m->in.data() + m->starts[jb.seq0 + (size_t)s], m->lens[jb.seq0 + (size_t)s], nullptr, nullptr));
    }
    RV_TRY(rv_construct(h, 0, nullptr, nullptr, 0));
    RV_TRY(rv_set_picker(h, m->picker, m->picker ? &m->pargs : nullptr));
    rv_align_stats st;
    memset(&st, 0, sizeof st);
    RV_TRY(rv_align_builtin(h, minl, minn, &st));
    many_add_stats(total, st);
    static const std::vector<int> none; static const std::vector<int64_t> none64;
    RV_TRY(many_collect(m, h, job, none, none64, none64));
    jb.text_off = (int64_t)m->out_text.size();
    jb.shared = false;
    m->out_text.resize(m->out_text.size() + (size_t)jb.ranks);
    if (rv_get_array(h, RV_T, m->out_text.data() + jb.text_off, jb.ranks) != jb.ranks) return -1;
    m->info[2]++;
    return 0;
}

int many_run(rv_many *m, int minl, int minn, rv_align_stats *total) {
    RV_HIP(hipSetDevice(m->device));
    m->ran = false; m->scanned = false; m->chained = false;
    m->mt_first.clear(); m->mt_l.clear(); m->mt_n.clear(); m->mt_off.clear(); m->mt_so.clear(); m->mt_pos.clear();
    m->recs.clear(); m->rpos.clear(); m->out_text.clear(); m->keep_sa.clear(); m->keep_lcp.clear();
    for (int k = 0; k < 5; k++) m->info[k] = 0;
    for (int k = 0; k < 8; k++) m->flagged[k] = 0;
    if (total) memset(total, 0, sizeof *total);
    const int nj = (int)m->jobs.size();
    m->info[0] = nj;
    // rounds: a round's text stays below the 32-bit library's position limit (and a bound on the device memory of a round)
    const int64_t lim = std::max<int64_t>(std::min<int64_t>(m->round_max, (int64_t)INT_MAX - 4096), 1);
    // every job's class (MANY_NCLASS: none), the classes with fewer jobs than their threshold dropped
    std::vector<int> cls((size_t)nj, MANY_NCLASS);
    int64_t count[MANY_NCLASS + 1] = {};
    for (int j = 0; j < nj; j++) {
        for (int c = 0; c < MANY_NCLASS && cls[(size_t)j] == MANY_NCLASS; c++) if (many_class_admits(m, many_classes[c], m->jobs[(size_t)j], minl, lim)) cls[(size_t)j] = c;
        count[cls[(size_t)j]]++;
    }
    bool take[MANY_NCLASS + 1] = {};
    for (int c = 0; c < MANY_NCLASS; c++) take[c] = count[c] > 0 && (!many_classes[c].min || count[c] >= m->*many_classes[c].min);
    std::vector<int> orders[MANY_NCLASS], rest;
    for (int j = 0; j < nj; j++) {
        m->jobs[(size_t)j].arr_off = -1;
        (take[cls[(size_t)j]] ? orders[cls[(size_t)j]] : rest).push_back(j);
    }
    for (int c = 0; c < MANY_NCLASS; c++) {
        const ManyClass &C = many_classes[c];
        std::vector<int> &ord = orders[c], *redo = C.picker == 1 ? &rest : nullptr;      // (a kind-1 round gives the jobs its kernels flag back)
        RV_TRY(many_rounds(m, ord, lim, [&](size_t lo, size_t hi) {
            return C.round == MANY_PAIRS ? many_round(m, ord, lo, hi, minl, minn, total, C.large, redo)
                 : C.round == MANY_CONTIGUOUS ? many_round_multi(m, ord, lo, hi, minl, minn, total, C.kmax, redo)
                 : many_round_large_multi(m, ord, lo, hi, minl, minn, total, C.kmax, redo);
        }));
    }
    if (m->picker == 1) std::sort(rest.begin(), rest.end());      // (flagged jobs came back behind the others; the built-in classes never add to `rest`)
    for (int j : rest) RV_TRY(many_ordinary(m, j, minl, minn, total));
    // the anchors job by job
    m->an_first.assign((size_t)nj + 1, 0);
    for (const ManyRec &r : m->recs) m->an_first[(size_t)r.job + 1]++;
    for (int j = 0; j < nj; j++) m->an_first[(size_t)j + 1] += m->an_first[(size_t)j];
    const size_t na = m->recs.size();
    std::vector<int64_t> at(m->an_first.begin(), m->an_first.end() - 1);
    std::vector<size_t> where(na);
    for (size_t k = 0; k < na; k++) where[(size_t)at[(size_t)m->recs[k].job]++] = k;
    m->an_l.resize(na); m->an_off.assign(na + 1, 0); m->an_pos.clear(); m->an_pos.reserve(m->rpos.size());
    for (size_t k = 0; k < na; k++) {
        const ManyRec &r = m->recs[where[k]];
        m->an_l[k] = r.l;
        for (int q = 0; q < r.np; q++) m->an_pos.push_back(m->rpos[(size_t)r.p0 + (size_t)q]);
        m->an_off[k + 1] = (int64_t)m->an_pos.size();
    }
    m->recs.clear(); m->rpos.clear();
    m->ran = true;
    return 0;
}

// ---- rv_many_scan: the match lists of every job instead of a finished recursion ----
// The jobs the shared launches take: 2 .. RV_MANY_WIDE_KMAX sequences, at most RV_LEAF_N ranks, no NUL byte (many.takes_shared_scan mirrors it).  No
// switch and no threshold for these.
bool many_scan_admits(const rv_many *m, const ManyJob &jb) {
    return !m->scan_ordinary && jb.k >= 2 && jb.k <= RV_MANY_WIDE_KMAX && jb.clean && jb.ranks <= RV_LEAF_N;
}
// ... and with RV_MANY_SCAN_LARGE on (many.takes_shared_scan(.., large=True)): the same above RV_LEAF_N ranks up to RV_MANY_LARGE_MAX, where the job fits
// a round (lim: many_scan's round limit) -- in a call with at least RV_MANY_SCAN_LARGE_MIN of them.  One class for every k: see many_round_scan
bool many_scan_large_admits(const rv_many *m, const ManyJob &jb, int64_t lim) {
    return !m->scan_ordinary && m->scan_large && jb.k >= 2 && jb.k <= RV_MANY_WIDE_KMAX && jb.clean && jb.ranks > RV_LEAF_N && jb.ranks <= m->large_max && jb.ranks <= lim;
}
bool many_scan_pair_kind(int kind, int k) { return kind == 0 || (kind == 2 && k == 2); }

// one round of the scan: the jobs order[lo .. hi) (ascending size), every one contiguous in the round's text as in many_round_multi -- pair jobs too: to
// k_many_build a job is its first sequence and "the rest", so the side bit of its BWT bytes says "behind the job's first '$'" for every k.  Then the count
// pass, the sums and the write pass of rv_many_scan.hip over the built segments.  Two copies come back: the sums at the jobs' first ranks with the error
// words behind them, and the records with the write pass' error word behind them.
// large: a round of jobs above RV_LEAF_N ranks (RV_MANY_SCAN_LARGE).  The same layout, the same tables and the same passes; only the index build differs:
// rv_many_large_build_c, the segmented prefix doubling on the round's text in place (segment j is [off_j, off_j + n_j) in elements and in ranks alike,
// so its descriptor is the offset, the size and the first sequence's length).  One round class for every k of 2 .. 64: a build is a long chain of
// launches -- radix passes times doubling rounds --, and a class per k range would pay it once per class in a mixed call.
int many_round_scan(rv_many *m, const std::vector<int> &order, size_t lo, size_t hi, int minl, int minn, int kind, bool large) {
    RV_TRY(many_handle(m, &m->hs));
    rv_index *h = m->hs;
    const size_t J = hi - lo;
    int64_t n = 0;
    size_t nseq = 0, nsmall = 0;
    for (size_t s = 0; s < J; s++) {
        const ManyJob &jb = m->jobs[(size_t)order[lo + s]];
        if (jb.k < 2 || jb.k > RV_MANY_WIDE_KMAX || (large ? jb.ranks <= CAP_L || jb.ranks > INT32_MAX : jb.ranks > CAP_L)) { rv_set_error("rv_many_scan: a job of %d sequences and %lld ranks in a shared round", jb.k, (long long)jb.ranks); return -1; }
        n += jb.ranks; nseq += (size_t)jb.k;
    }
    if (n > RV_MANY_SCAN_RANKS) { rv_set_error("rv_many_scan: a round of %lld ranks", (long long)n); return -1; }
    // the tables of the round in one upload: off[J + 1], beg[nseq] (64 bits) | sfirst[J + 1], loc[nseq] (32 bits)
    const size_t n64 = J + 1 + nseq, n32 = J + 1 + nseq;
    std::vector<int64_t> tab(n64 + (n32 + 1) / 2, 0);
    int64_t *t_off = tab.data(), *t_beg = t_off + J + 1;
    int32_t *t_sf = (int32_t *)(tab.data() + n64), *t_loc = t_sf + J + 1;
    std::vector<ManyDevJob> dj(large ? 0 : J);
    std::vector<ManyDevJobC> djc(large ? J : 0);
    std::vector<char> txt((size_t)n);
    int64_t at = 0, maxn = 0;
    size_t sq = 0;
    for (size_t s = 0; s < J; s++) {
        const ManyJob &jb = m->jobs[(size_t)order[lo + s]];
        const int64_t la = m->lens[jb.seq0];
        if (large) { djc[s].off = at; djc[s].n = (int32_t)jb.ranks; djc[s].la = (int32_t)la; maxn = std::max(maxn, jb.ranks); }
        else { dj[s].abeg = at; dj[s].bbeg = at + la + 1; dj[s].off = at; dj[s].la = (int32_t)la; dj[s].lb = (int32_t)(jb.ranks - la - 2); }
        t_off[s] = at; t_sf[s] = (int32_t)sq;
        if (jb.ranks <= m->wave_max && jb.ranks <= CAP_S) nsmall = s + 1;      // (ascending sizes: the small class is a prefix)
        const int64_t job0 = at;
        for (int q = 0; q < jb.k; q++) {
            const int64_t len = m->lens[jb.seq0 + (size_t)q];
            t_beg[sq] = at; t_loc[sq] = (int32_t)(at - job0); sq++;
            memcpy(txt.data() + at, m->in.data() + m->starts[jb.seq0 + (size_t)q], (size_t)len);
            txt[(size_t)(at + len)] = '$';
            at += len + 1;
        }
    }
    t_off[J] = at; t_sf[J] = (int32_t)sq;
    if (at != n || sq != nseq) { rv_set_error("rv_many_scan: the jobs' ranks do not add up to the text"); return -1; }
    hipStream_t q = h->ws.stream;
    const size_t first_bytes = (J + 1) * sizeof(u64), words_bytes = 16;      // words: [0] max LCP, [1] error bits of the build, [2] of the count pass
    const size_t jobs_bytes = large ? J * sizeof(ManyDevJobC) : J * sizeof(ManyDevJob);
    RV_TRY(m->dJobs.reserve(jobs_bytes));
    RV_TRY(m->dScanTab.reserve(tab.size() * sizeof(int64_t)));
    RV_TRY(m->dTxt.reserve((size_t)n + 64));
    RV_TRY(m->dSA.reserve((size_t)(n + 64) * sizeof(sa_t)));
    RV_TRY(m->dLCP.reserve((size_t)(n + 64) * sizeof(lcp_t)));
    RV_TRY(m->dBWT.reserve((size_t)n + 64));
    RV_TRY(m->dScanCnt.reserve((size_t)(n + 1) * sizeof(u64)));
    RV_TRY(m->dScanFirst.reserve(first_bytes + words_bytes));
    RV_HIP(hipMemcpyAsync(m->dJobs.p, large ? (const void *)djc.data() : (const void *)dj.data(), jobs_bytes, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(m->dScanTab.p, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(m->dTxt.p, txt.data(), (size_t)n, hipMemcpyHostToDevice, q));
    u32 *d_words = (u32 *)((char *)m->dScanFirst.p + first_bytes);
    RV_HIP(hipMemsetAsync(d_words, 0, words_bytes, q));
    if (large) {
        RV_HIP(hipMemsetAsync(m->dTxt.as<uint8_t>() + n, 0, 64, q));      // (the build reads eight bytes at a time, on the text in place)
        RV_TRY(rv_many_large_build_c(h->ws, m->large_bufs, m->dJobs.as<ManyDevJobC>(), (int64_t)J, n, maxn, m->dTxt.as<uint8_t>(), m->dSA.as<sa_t>(), m->dLCP.as<lcp_t>(),
                                     m->dBWT.as<uint8_t>(), d_words, &m->info[4]));
    } else RV_TRY(many_build(m, q, m->dJobs.as<ManyDevJob>(), J, nsmall, m->dTxt.as<uint8_t>(), d_words, d_words + 1));
    RvManyScanRound R;
    R.SA = m->dSA.as<sa_t>(); R.LCP = m->dLCP.as<lcp_t>(); R.BWT = m->dBWT.as<uint8_t>(); R.m = n;
    R.off = m->dScanTab.as<int64_t>(); R.beg = R.off + J + 1;
    R.sfirst = (const int32_t *)(m->dScanTab.as<int64_t>() + n64); R.loc = R.sfirst + J + 1;
    R.njobs = (int)J; R.nbeg = (int)nseq; R.minl = minl; R.minn = minn; R.minn_k = m->kc ? 1 : 0; R.kind = kind; R.err = d_words + 2;
    RV_TRY(rv_many_scan_count(h->ws, R, m->dScanCnt.as<u64>(), m->dScanFirst.as<u64>(), &m->info[4]));
    std::vector<u64> first(J + 3, 0);
    RV_TRY(rv_read_back(h->ws, first.data(), m->dScanFirst.p, first_bytes + words_bytes));
    u32 words[4];
    memcpy(words, first.data() + J + 1, sizeof words);
    if (words[1]) { rv_set_error("rv_many_scan: the index build refused a job (error bits %u)", words[1]); return -1; }
    if (words[2]) { rv_set_error("rv_many_scan: the count pass met a descriptor outside the round (error bits %u: 1 job, 2 position)", words[2]); return -1; }
    const u64 mmask = ((u64)1 << RV_MANY_SCAN_MBITS) - 1;
    const u64 nrec = first[J] >> RV_MANY_SCAN_MBITS, nmem = first[J] & mmask;
    if (nrec > (u64)n || nmem > (u64)n * 64) { rv_set_error("rv_many_scan: more records than the round has room for"); return -1; }
    // records | pos | so | the write pass' error word
    const size_t o_pos = (size_t)nrec * sizeof(RvManyScanRec), o_so = o_pos + (size_t)nmem * sizeof(u32), o_err = (o_so + (size_t)nmem * sizeof(uint16_t) + 3) & ~(size_t)3;
    std::vector<u64> out;      // (64-bit words: the records are read in place)
    std::vector<sa_t> sa; std::vector<lcp_t> lc;
    if (nrec) {
        RV_TRY(m->dScanOut.reserve(o_err + 4));
        char *d_out = (char *)m->dScanOut.p;
        RV_HIP(hipMemsetAsync(d_out + o_err, 0, 4, q));
        R.err = (u32 *)(d_out + o_err);
        RV_TRY(rv_many_scan_write(h->ws, R, m->dScanCnt.as<u64>(), (RvManyScanRec *)d_out, nrec, (uint16_t *)(d_out + o_so), (u32 *)(d_out + o_pos), nmem, &m->info[4]));
    }
    // rv_many_kchain: the chains on the device, from the records where the write pass has left them.  What comes back is the paths and a word per job;
    // the records themselves only where a job is flagged for the host
    const bool dev_chain = m->kc && !m->kc_host;
    std::vector<u64> kjob;      // cfirst[J + 1] | end[J] | flag[J] (32 bits) | error word
    std::vector<u64> kout;      // score[nodes] | l[nodes] | pos[nodes x k]
    u64 knodes = 0, kmem = 0;
    bool any_flag = false;
    const size_t kj_end = (J + 1) * sizeof(u64), kj_flag = kj_end + J * sizeof(int64_t), kj_err = kj_flag + ((J + 1) / 2) * 8, kj_bytes = kj_err + 8;
    if (dev_chain) {
        char *d_out = (char *)m->dScanOut.p;
        RV_TRY(m->dKcStage.reserve((size_t)std::max<u64>(nrec, 1) * (sizeof(int64_t) + sizeof(u32))));
        RV_TRY(m->dKcJob.reserve(kj_bytes));
        char *d_job = (char *)m->dKcJob.p;
        RvKchainRound K;
        K.rec = nrec ? (const RvManyScanRec *)d_out : nullptr; K.so = nrec ? (const uint16_t *)(d_out + o_so) : nullptr; K.pos = nrec ? (const u32 *)(d_out + o_pos) : nullptr;
        K.nrec = nrec; K.nmem = nmem; K.first = m->dScanFirst.as<u64>();
        K.stage_score = m->dKcStage.as<int64_t>(); K.stage_rec = (u32 *)(K.stage_score + std::max<u64>(nrec, 1));
        K.nodes = m->dScanCnt.as<u64>();      // (the write pass has read its sums: the room is free, and a word per rank is what the chain's sum wants)
        K.end = (int64_t *)(d_job + kj_end); K.flag = (u32 *)(d_job + kj_flag); K.err = (u32 *)(d_job + kj_err);
        RV_HIP(hipMemsetAsync(K.nodes, 0, (size_t)(n + 1) * sizeof(u64), q));
        RV_HIP(hipMemsetAsync(K.err, 0, 8, q));
        RV_TRY(rv_many_kchain_run(h->ws, R, K, *m->kc, &m->info[4]));
        RV_TRY(rv_exclusive_sum_u64(h->ws, K.nodes, K.nodes, n + 1));
        m->info[4] += n + 1 <= 2048 ? 1 : n + 1 <= (int64_t)2048 * 2048 ? 3 : 5;
        RV_TRY(rv_many_kchain_first(h->ws, R, K, (u64 *)d_job, &m->info[4]));
        kjob.assign(kj_bytes / 8, 0);
        RV_TRY(rv_read_back(h->ws, kjob.data(), d_job, kj_bytes));
        u32 kerr = 0;
        memcpy(&kerr, (const char *)kjob.data() + kj_err, 4);
        if (kerr) { rv_set_error("rv_many_kchain: the chain kernel met a job outside its room (error bits %u: 1 descriptor, 2 member, 4 path)", kerr); return -1; }
        knodes = kjob[J] >> RV_MANY_SCAN_MBITS; kmem = kjob[J] & mmask;
        if (knodes > nrec || kmem > nmem) { rv_set_error("rv_many_kchain: more nodes than the round has records"); return -1; }
        const u32 *kflag = (const u32 *)((const char *)kjob.data() + kj_flag);
        for (size_t s = 0; s < J; s++) any_flag = any_flag || kflag[s] != 0;
        if (knodes) {
            const size_t ko_l = (size_t)knodes * sizeof(int64_t), ko_pos = ko_l + (size_t)knodes * sizeof(u32), ko_bytes = ko_pos + (size_t)kmem * sizeof(u32);
            RV_TRY(m->dKcOut.reserve(ko_bytes));
            char *d_ko = (char *)m->dKcOut.p;
            RV_TRY(rv_many_kchain_write(h->ws, R, K, (const u64 *)d_job, (u32 *)(d_ko + ko_l), (int64_t *)d_ko, (u32 *)(d_ko + ko_pos), knodes, kmem, &m->info[4]));
            kout.assign((ko_bytes + 7) / 8, 0);
            RV_HIP(hipMemcpyAsync(kout.data(), d_ko, ko_bytes, hipMemcpyDeviceToHost, q));
            RV_HIP(hipMemcpyAsync(kjob.data() + kj_err / 8, K.err, 8, hipMemcpyDeviceToHost, q));
        }
    }
    const bool fetch = nrec && (!dev_chain || any_flag);
    out.assign(((fetch ? o_err : 0) + 4 + 7) / 8, 0);
    const size_t h_err = fetch ? o_err : 0;      // where the write pass' error word lands
    if (fetch) RV_HIP(hipMemcpyAsync(out.data(), (char *)m->dScanOut.p, o_err + 4, hipMemcpyDeviceToHost, q));
    else if (nrec) RV_HIP(hipMemcpyAsync(out.data(), (char *)m->dScanOut.p + o_err, 4, hipMemcpyDeviceToHost, q));
    if (m->keep) {
        sa.resize((size_t)n); lc.resize((size_t)n);
        RV_HIP(hipMemcpyAsync(sa.data(), m->dSA.p, (size_t)n * sizeof(sa_t), hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(lc.data(), m->dLCP.p, (size_t)n * sizeof(lcp_t), hipMemcpyDeviceToHost, q));
    }
    RV_HIP(hipStreamSynchronize(q));
    const char *hout = (const char *)out.data();
    u32 werr = 0;
    memcpy(&werr, hout + h_err, 4);
    if (werr) { rv_set_error("rv_many_scan: the write pass did not find what the count pass counted (error bits %u: 1 job, 2 position, 4 room)", werr); return -1; }
    const RvManyScanRec *rec = (const RvManyScanRec *)hout;
    const u32 *hpos = (const u32 *)(hout + o_pos);
    const uint16_t *hso = (const uint16_t *)(hout + o_so);
    const size_t kbase = m->keep_sa.size();
    if (m->keep) { m->keep_sa.resize(kbase + (size_t)n); m->keep_lcp.resize(kbase + (size_t)n); }
    const u32 *kflag = dev_chain ? (const u32 *)((const char *)kjob.data() + kj_flag) : nullptr;
    if (dev_chain) {
        u32 kerr = 0;
        memcpy(&kerr, (const char *)kjob.data() + kj_err, 4);
        if (kerr) { rv_set_error("rv_many_kchain: the write kernel met a node outside its room (error bits %u: 1 descriptor, 2 member, 4 path)", kerr); return -1; }
    }
    for (size_t s = 0; s < J; s++) {
        ManyJob &jb = m->jobs[(size_t)order[lo + s]];
        if (dev_chain) {
            // the job's path: nodes kjob[s] .. kjob[s + 1] of the round's CSR, or a flag word
            if (kflag[s]) many_count_flags(m, kflag[s]);
            else {
                const u64 n0 = kjob[s] >> RV_MANY_SCAN_MBITS, n1 = kjob[s + 1] >> RV_MANY_SCAN_MBITS, p0 = kjob[s] & mmask, p1 = kjob[s + 1] & mmask;
                if (n0 > n1 || n1 > knodes || p1 - p0 != (n1 - n0) * (u64)jb.k || p1 > kmem) { rv_set_error("rv_many_kchain: the sums of the chains do not add up"); return -1; }
                ManyKchainSlice &ks = m->kc_job[(size_t)order[lo + s]];
                ks.done = true; ks.node0 = (int64_t)m->kc_l.size(); ks.pos0 = (int64_t)m->kc_pos.size(); ks.nnodes = (int64_t)(n1 - n0);
                ks.end = ((const int64_t *)((const char *)kjob.data() + kj_end))[s];
                const int64_t *ksc = (const int64_t *)kout.data();
                const u32 *kl = (const u32 *)(ksc + knodes), *kp = kl + knodes;
                for (u64 x = n0; x < n1; x++) {
                    m->kc_l.push_back(kl[x]); m->kc_score.push_back(ksc[x]);
                    for (int d = 0; d < jb.k; d++) {
                        const int64_t p = (int64_t)kp[p0 + (x - n0) * (u64)jb.k + (u64)d];
                        if (p + kl[x] > m->lens[jb.seq0 + (size_t)d]) { rv_set_error("rv_many_kchain: a node outside its sequence"); return -1; }
                        m->kc_pos.push_back(p);
                    }
                }
            }
        }
        if (dev_chain && !kflag[s]) {      // (its records stay on the device)
            jb.shared = true;
            if (m->keep) {
                jb.arr_off = (int64_t)kbase + t_off[s];
                for (int64_t r = t_off[s]; r < t_off[s + 1]; r++) { m->keep_sa[kbase + (size_t)r] = (sa_t)(sa[(size_t)r] - (sa_t)t_off[s]); m->keep_lcp[kbase + (size_t)r] = lc[(size_t)r]; }
            }
            continue;
        }
        const u64 r0 = first[s] >> RV_MANY_SCAN_MBITS, r1 = first[s + 1] >> RV_MANY_SCAN_MBITS, m0 = first[s] & mmask, m1 = first[s + 1] & mmask;
        if (r0 > r1 || r1 > nrec || m0 > m1 || m1 > nmem) { rv_set_error("rv_many_scan: the sums of the round do not increase"); return -1; }
        ManyScanSlice &sl = m->sc_job[(size_t)order[lo + s]];
        sl.rec0 = (int64_t)m->sc_l.size(); sl.nrec = (int64_t)(r1 - r0); sl.mem0 = (int64_t)m->sc_pos.size(); sl.nmem = (int64_t)(m1 - m0);
        u64 mo = m0;
        for (u64 r = r0; r < r1; r++) {
            if (rec[r].moff != mo || rec[r].n < 2 || rec[r].n > (u32)jb.k || mo + rec[r].n > m1) { rv_set_error("rv_many_scan: a malformed record"); return -1; }
            m->sc_l.push_back(rec[r].l); m->sc_n.push_back((int32_t)rec[r].n);
            for (u32 x = 0; x < rec[r].n; x++) {
                if (hso[mo + x] >= (uint16_t)jb.k || (int64_t)hpos[mo + x] + rec[r].l > jb.ranks) { rv_set_error("rv_many_scan: a match outside its job"); return -1; }
                m->sc_so.push_back(hso[mo + x]); m->sc_pos.push_back((int64_t)hpos[mo + x]);
            }
            mo += rec[r].n;
        }
        if (mo != m1) { rv_set_error("rv_many_scan: a malformed record"); return -1; }
        jb.shared = true;
        if (m->keep) {
            // test hook: SA / LCP of every job in job-local positions
            jb.arr_off = (int64_t)kbase + t_off[s];
            for (int64_t r = t_off[s]; r < t_off[s + 1]; r++) { m->keep_sa[kbase + (size_t)r] = (sa_t)(sa[(size_t)r] - (sa_t)t_off[s]); m->keep_lcp[kbase + (size_t)r] = lc[(size_t)r]; }
        }
    }
    m->info[1] += (int64_t)J; m->info[3]++;
    return 0;
}

// a job the shared launches do not take: construct() + rv_getmums / rv_getmultimums on the reused handle, every sequence a sample
int many_scan_ordinary(rv_many *m, int job, int minl, int minn, int kind) {
    RV_TRY(many_handle(m, &m->ho));
    rv_index *h = m->ho;
    ManyJob &jb = m->jobs[(size_t)job];
    RV_TRY(rv_reset(h));
    for (int s = 0; s < jb.k; s++) {
        RV_TRY(rv_add_sample(h));
        RV_TRY(rv_add_sequence(h, m->in.data() + m->starts[jb.seq0 + (size_t)s], m->lens[jb.seq0 + (size_t)s], nullptr, nullptr));
    }
    RV_TRY(rv_construct(h, 0, nullptr, nullptr, 0));
    ManyScanSlice &sl = m->sc_job[(size_t)job];
    sl.rec0 = (int64_t)m->sc_l.size(); sl.mem0 = (int64_t)m->sc_pos.size();
    // (rv_getmultimums refuses an index of two samples, as the reference's has no SO then; on such an index its records are getmums' -- one interval
    // of two ranks per MUM, the same side test and left-maximality -- with the members in SA order)
    if (m->kc) minn = jb.k;
    const bool by_rank = !many_scan_pair_kind(kind, jb.k) && jb.k == 2;
    if (by_rank && minn > 2) {
        // (an interval of a pair index has two members)
    } else if (many_scan_pair_kind(kind, jb.k) || by_rank) {
        const int64_t nm = rv_getmums(h, minl);
        if (nm < 0) return -1;
        std::vector<u32> l((size_t)std::max<int64_t>(nm, 1));
        std::vector<int64_t> a((size_t)std::max<int64_t>(nm, 1)), b((size_t)std::max<int64_t>(nm, 1));
        RV_TRY(rv_fetch_mums(h, l.data(), a.data(), b.data(), nm));
        std::vector<int64_t> sbeg((size_t)jb.k);      // where the job's sequences begin in its text s0$s1$..
        int64_t at = 0;
        for (int s = 0; s < jb.k; s++) { sbeg[(size_t)s] = at; at += m->lens[jb.seq0 + (size_t)s] + 1; }
        std::vector<int64_t> inv;
        if (by_rank && nm > 0) {
            std::vector<sa_t> sa((size_t)jb.ranks);
            if (rv_get_array(h, RV_SA, sa.data(), jb.ranks) != jb.ranks) return -1;
            inv.assign((size_t)jb.ranks, 0);
            for (int64_t r = 0; r < jb.ranks; r++) {
                if ((int64_t)sa[(size_t)r] < 0 || (int64_t)sa[(size_t)r] >= jb.ranks) { rv_set_error("rv_many_scan: a suffix array entry outside its job"); return -1; }
                inv[(size_t)sa[(size_t)r]] = r;
            }
        }
        for (int64_t x = 0; x < nm; x++) {
            int64_t pa = std::min(a[(size_t)x], b[(size_t)x]), pb = std::max(a[(size_t)x], b[(size_t)x]);
            if (pa < 0 || pb >= jb.ranks) { rv_set_error("rv_many_scan: a match outside its job"); return -1; }
            if (by_rank && inv[(size_t)pa] > inv[(size_t)pb]) std::swap(pa, pb);
            m->sc_l.push_back(l[(size_t)x]); m->sc_n.push_back(2);
            m->sc_so.push_back((uint16_t)((std::upper_bound(sbeg.begin(), sbeg.end(), pa) - sbeg.begin()) - 1)); m->sc_pos.push_back(pa);
            m->sc_so.push_back((uint16_t)((std::upper_bound(sbeg.begin(), sbeg.end(), pb) - sbeg.begin()) - 1)); m->sc_pos.push_back(pb);
        }
    } else {
        int64_t members = 0;
        const int64_t nm = rv_getmultimums(h, minl, minn, 0, &members);
        if (nm < 0) return -1;
        std::vector<u32> l((size_t)std::max<int64_t>(nm, 1));
        std::vector<int32_t> cn((size_t)std::max<int64_t>(nm, 1));
        std::vector<int64_t> off((size_t)nm + 1, 0), pos((size_t)std::max<int64_t>(members, 1));
        std::vector<uint16_t> so((size_t)std::max<int64_t>(members, 1));
        RV_TRY(rv_fetch_multi(h, l.data(), cn.data(), off.data(), so.data(), pos.data()));
        for (int64_t x = 0; x < nm; x++) {
            if (off[(size_t)x + 1] - off[(size_t)x] != cn[(size_t)x]) { rv_set_error("rv_many_scan: a match of %d members with %lld positions", cn[(size_t)x], (long long)(off[(size_t)x + 1] - off[(size_t)x])); return -1; }
            m->sc_l.push_back(l[(size_t)x]); m->sc_n.push_back(cn[(size_t)x]);
        }
        m->sc_so.insert(m->sc_so.end(), so.begin(), so.begin() + (ptrdiff_t)members);
        m->sc_pos.insert(m->sc_pos.end(), pos.begin(), pos.begin() + (ptrdiff_t)members);
    }
    sl.nrec = (int64_t)m->sc_l.size() - sl.rec0; sl.nmem = (int64_t)m->sc_pos.size() - sl.mem0;
    jb.shared = false;
    m->info[2]++;
    return 0;
}

// a switch of RV_OPTION_LIST as rv_many_option has taken it for the internal handles: the last value given, or the default
int64_t many_fwd_option(const rv_many *m, const char *name, int64_t def) {
    for (const auto &o : m->fwd) if (o.first == name) def = o.second;
    return def;
}

// a list rv_many_kchain has to chain outside the rounds: rv_kchain's arguments and where the path goes
struct ManyKchainSrc {
    int k; int64_t nrec; const u32 *l; const int32_t *n; const int64_t *off; const uint16_t *so; const int64_t *pos; const int64_t *lens;
    ManyKchainSlice *out;
};

void many_kchain_store(rv_many *m, const ManyKchainSrc &s, int64_t nn, const u32 *ol, const int64_t *osc, const int64_t *opos, int64_t end) {
    ManyKchainSlice &ks = *s.out;
    ks.done = true; ks.node0 = (int64_t)m->kc_l.size(); ks.pos0 = (int64_t)m->kc_pos.size(); ks.nnodes = nn; ks.end = end;
    m->kc_l.insert(m->kc_l.end(), ol, ol + nn);
    m->kc_score.insert(m->kc_score.end(), osc, osc + nn);
    m->kc_pos.insert(m->kc_pos.end(), opos, opos + nn * s.k);
}

// The lists no round has chained.  With RV_MANY_KCHAIN_HOST, or RV_MANY_KCHAIN_BIG at 0, rv_kchain on each.  Otherwise one preparation per list
// (kc_prepare); the lists it admits with at least RV_KCHAIN_BIG_MIN kept points are chained together by the device programme (rv_kchain_big.hip), the
// rest by the host programme; one backtrack for both.
int many_kchain_rest(rv_many *m, const std::vector<ManyKchainSrc> &src, const RvKchainArgs &A) {
    const bool big = !m->kc_host && many_fwd_option(m, "RV_MANY_KCHAIN_BIG", 1) != 0;
    const int64_t big_min = std::min<int64_t>(std::max<int64_t>(many_fwd_option(m, "RV_KCHAIN_BIG_MIN", RV_KCHAIN_BIG_MIN_DEFAULT), 1), RV_KCHAIN_CAP + 1);
    std::vector<u32> ol;
    std::vector<int64_t> opos, osc;
    auto room = [&](const ManyKchainSrc &s) {
        const size_t nr = (size_t)std::max<int64_t>(s.nrec, 1);
        if (ol.size() < nr) { ol.resize(nr); osc.resize(nr); }
        if (opos.size() < nr * (size_t)s.k) opos.resize(nr * (size_t)s.k);
    };
    if (!big) {
        for (const ManyKchainSrc &s : src) {
            room(s);
            int64_t end = 0;
            const int64_t nn = rv_kchain(s.k, s.nrec, s.l, s.n, s.off, s.so, s.pos, s.lens, A.maxmums, A.wpen, A.wscore, A.gcmodel, ol.data(), opos.data(), osc.data(), &end);
            if (nn < 0) return -1;
            many_kchain_store(m, s, nn, ol.data(), osc.data(), opos.data(), end);
        }
        return 0;
    }
    std::vector<KcPrep> prep(src.size());
    std::vector<const KcPrep *> dev;
    std::vector<size_t> dev_src;
    std::vector<int64_t> score;
    std::vector<int> back;
    for (size_t x = 0; x < src.size(); x++) {
        const ManyKchainSrc &s = src[x];
        room(s);
        KcPrep &pp = prep[x];
        RV_TRY(kc_prepare(s.k, s.nrec, s.l, s.n, s.off, s.pos, s.lens, A.maxmums, A.wpen, A.wscore, pp));
        if (pp.m == 0) { many_kchain_store(m, s, 0, ol.data(), osc.data(), opos.data(), kc_empty_end(pp, A.wpen, A.gcmodel)); continue; }
        if (!pp.refuse && pp.m >= big_min) { dev.push_back(&pp); dev_src.push_back(x); continue; }
        RV_TRY(kc_programme_host(pp, A.wpen, A.wscore, A.gcmodel, score, back));
        int64_t end = 0;
        const int64_t nn = kc_backtrack(pp, score, back, ol.data(), opos.data(), osc.data(), &end);
        if (nn < 0) return -1;
        many_kchain_store(m, s, nn, ol.data(), osc.data(), opos.data(), end);
        pp = KcPrep();
    }
    if (dev.empty()) return 0;
    RV_TRY(many_handle(m, &m->hs));
    std::vector<std::vector<int64_t>> dscore;
    std::vector<std::vector<int>> dback;
    RV_TRY(rv_kchain_big_run(m->hs->ws, m->kc_big_bufs, dev, A.wpen, A.wscore, A.gcmodel, dscore, dback, &m->kc_big[1]));
    for (size_t y = 0; y < dev.size(); y++) {
        const ManyKchainSrc &s = src[dev_src[y]];
        int64_t end = 0;
        const int64_t nn = kc_backtrack(*dev[y], dscore[y], dback[y], ol.data(), opos.data(), osc.data(), &end);
        if (nn < 0) return -1;
        many_kchain_store(m, s, nn, ol.data(), osc.data(), opos.data(), end);
    }
    m->kc_big[0] += (int64_t)dev.size();
    m->info[4] += m->kc_big[1];
    return 0;
}

// the results of rv_many_kchain / rv_many_kchain_lists from the slices, list by list (k: sequences of each)
void many_kchain_collect(rv_many *m, const std::vector<ManyKchainSlice> &slices, const std::vector<int> &ks) {
    const size_t nj = slices.size();
    m->kch_first.assign(nj + 1, 0); m->kch_end.assign(nj, 0);
    m->kch_l.clear(); m->kch_score.clear(); m->kch_pos.clear();
    for (size_t j = 0; j < nj; j++) {
        const ManyKchainSlice &ks_ = slices[j];
        m->kch_first[j + 1] = m->kch_first[j] + ks_.nnodes; m->kch_end[j] = ks_.end;
        m->kch_l.insert(m->kch_l.end(), m->kc_l.begin() + (ptrdiff_t)ks_.node0, m->kc_l.begin() + (ptrdiff_t)(ks_.node0 + ks_.nnodes));
        m->kch_score.insert(m->kch_score.end(), m->kc_score.begin() + (ptrdiff_t)ks_.node0, m->kc_score.begin() + (ptrdiff_t)(ks_.node0 + ks_.nnodes));
    }
    for (size_t j = 0; j < nj; j++) {
        const ManyKchainSlice &ks_ = slices[j];
        m->kch_pos.insert(m->kch_pos.end(), m->kc_pos.begin() + (ptrdiff_t)ks_.pos0, m->kc_pos.begin() + (ptrdiff_t)(ks_.pos0 + ks_.nnodes * ks[j]));
    }
}

// kc: rv_many_kchain -- the scan of kind 1 with minn = k per job, every list chained (on the device where it lies, or by many_kchain_rest) instead of handed out
int many_scan(rv_many *m, int minl, int minn, int kind, const RvKchainArgs *kc = nullptr) {
    RV_HIP(hipSetDevice(m->device));
    m->ran = false; m->scanned = false; m->chained = false;
    m->kc = kc; m->kc_host = kc && many_fwd_option(m, "RV_MANY_KCHAIN_HOST", 0) != 0;
    struct KcReset { rv_many *m; ~KcReset() { m->kc = nullptr; } } kc_reset{m};
    m->kc_job.assign(kc ? m->jobs.size() : 0, ManyKchainSlice());
    m->kc_l.clear(); m->kc_score.clear(); m->kc_pos.clear();
    m->an_first.clear(); m->an_l.clear(); m->an_off.clear(); m->an_pos.clear(); m->out_text.clear(); m->keep_sa.clear(); m->keep_lcp.clear();
    m->sc_l.clear(); m->sc_n.clear(); m->sc_so.clear(); m->sc_pos.clear();
    for (int k = 0; k < 5; k++) m->info[k] = 0;
    for (int k = 0; k < 8; k++) m->flagged[k] = 0;
    m->kc_big[0] = m->kc_big[1] = 0;
    const int nj = (int)m->jobs.size();
    m->info[0] = nj;
    m->sc_job.assign((size_t)nj, ManyScanSlice());
    // rounds: RV_MANY_ROUND positions at most, and few enough for the packed sums of the scan (RV_MANY_SCAN_RANKS: below the segmented build's 2^31 elements)
    const int64_t lim = std::max<int64_t>(std::min<int64_t>(m->round_max, RV_MANY_SCAN_RANKS), 1);
    // (a large job has to fit a round: one that does not goes the ordinary way)
    int64_t nlarge = 0;
    for (const ManyJob &jb : m->jobs) nlarge += many_scan_large_admits(m, jb, lim) ? 1 : 0;
    const bool take_large = nlarge > 0 && nlarge >= m->scan_large_min;
    std::vector<int> order, lorder, rest;
    for (int j = 0; j < nj; j++) {
        const ManyJob &jb = m->jobs[(size_t)j];
        m->jobs[(size_t)j].arr_off = -1;
        (many_scan_admits(m, jb) ? order : take_large && many_scan_large_admits(m, jb, lim) ? lorder : rest).push_back(j);
    }
    // the small rounds, then the large ones (a job above RV_LEAF_N ranks holds more than 2^11 of a round's at most 2^26 ranks: fewer than the build's 2^20 jobs)
    for (int large = 0; large < 2; large++) {
        std::vector<int> &ord = large ? lorder : order;
        RV_TRY(many_rounds(m, ord, lim, [&](size_t lo, size_t hi) { return many_round_scan(m, ord, lo, hi, minl, minn, kind, large != 0); }));
    }
    for (int j : rest) RV_TRY(many_scan_ordinary(m, j, minl, minn, kind));
    if (kc) {
        // the chains job by job; what no round has chained goes to the device programme or to the host
        std::vector<ManyKchainSrc> src;
        std::vector<std::vector<int64_t>> offs;
        for (int j = 0; j < nj; j++) if (!m->kc_job[(size_t)j].done) {
            const ManyJob &jb = m->jobs[(size_t)j];
            const ManyScanSlice &sl = m->sc_job[(size_t)j];
            offs.emplace_back((size_t)sl.nrec + 1, 0);
            std::vector<int64_t> &off = offs.back();
            for (int64_t r = 0; r < sl.nrec; r++) off[(size_t)r + 1] = off[(size_t)r] + m->sc_n[(size_t)(sl.rec0 + r)];
            if (off[(size_t)sl.nrec] != sl.nmem) { rv_set_error("rv_many_kchain: the members of a list do not add up"); return -1; }
            src.push_back({jb.k, sl.nrec, m->sc_l.data() + sl.rec0, m->sc_n.data() + sl.rec0, nullptr, m->sc_so.data() + sl.mem0, m->sc_pos.data() + sl.mem0,
                           m->lens.data() + jb.seq0, &m->kc_job[(size_t)j]});
        }
        for (size_t x = 0; x < src.size(); x++) src[x].off = offs[x].data();
        RV_TRY(many_kchain_rest(m, src, *kc));
        std::vector<int> ks((size_t)nj);
        for (int j = 0; j < nj; j++) ks[(size_t)j] = m->jobs[(size_t)j].k;
        many_kchain_collect(m, m->kc_job, ks);
        m->sc_job.clear(); m->sc_l.clear(); m->sc_n.clear(); m->sc_so.clear(); m->sc_pos.clear();
        m->kc_job.clear(); m->kc_l.clear(); m->kc_score.clear(); m->kc_pos.clear();
        m->chained = true;
        return 0;
    }
    // the lists job by job
    m->mt_first.assign((size_t)nj + 1, 0);
    size_t nmem = 0;
    for (int j = 0; j < nj; j++) { m->mt_first[(size_t)j + 1] = m->mt_first[(size_t)j] + m->sc_job[(size_t)j].nrec; nmem += (size_t)m->sc_job[(size_t)j].nmem; }
    const size_t nrec = (size_t)m->mt_first[(size_t)nj];
    m->mt_l.clear(); m->mt_n.clear(); m->mt_so.clear(); m->mt_pos.clear();
    m->mt_l.reserve(nrec); m->mt_n.reserve(nrec); m->mt_so.reserve(nmem); m->mt_pos.reserve(nmem);
    m->mt_off.assign(nrec + 1, 0);
    for (int j = 0; j < nj; j++) {
        const ManyScanSlice &sl = m->sc_job[(size_t)j];
        m->mt_l.insert(m->mt_l.end(), m->sc_l.begin() + (ptrdiff_t)sl.rec0, m->sc_l.begin() + (ptrdiff_t)(sl.rec0 + sl.nrec));
        m->mt_n.insert(m->mt_n.end(), m->sc_n.begin() + (ptrdiff_t)sl.rec0, m->sc_n.begin() + (ptrdiff_t)(sl.rec0 + sl.nrec));
        m->mt_so.insert(m->mt_so.end(), m->sc_so.begin() + (ptrdiff_t)sl.mem0, m->sc_so.begin() + (ptrdiff_t)(sl.mem0 + sl.nmem));
        m->mt_pos.insert(m->mt_pos.end(), m->sc_pos.begin() + (ptrdiff_t)sl.mem0, m->sc_pos.begin() + (ptrdiff_t)(sl.mem0 + sl.nmem));
    }
    // (a match's members are as many as the positions between its offsets: getmultimums' count field, 2 for getmums)
    for (size_t k = 0; k < nrec; k++) m->mt_off[k + 1] = m->mt_off[k] + m->mt_n[k];
    if ((size_t)m->mt_off[nrec] != nmem) { rv_set_error("rv_many_scan: the members of the lists do not add up"); return -1; }
    m->sc_job.clear(); m->sc_l.clear(); m->sc_n.clear(); m->sc_so.clear(); m->sc_pos.clear();
    m->scanned = true;
    return 0;
}

// rv_many_option: the options that are no class switch or threshold (those are many_classes') -- lo: the least value taken; boolean: any value but 0 is 1
struct ManyOption { const char *name; int64_t rv_many::*field; int64_t lo; bool boolean; };
const ManyOption many_options[] = {
    {"RV_MANY_KEEP", &rv_many::keep, INT64_MIN, false},
    {"RV_MANY_ROUND", &rv_many::round_max, 1, false},
    {"RV_MANY_STAGE", &rv_many::stage, 0, false},
    {"RV_MANY_WAVE_MAX", &rv_many::wave_max, 0, false},
    {"RV_MANY_LARGE_MAX", &rv_many::large_max, 0, false},
    {"RV_MANY_CHAIN_FLAG", &rv_many::chain_flag, 0, false},
    {"RV_MANY_SCAN_ORDINARY", &rv_many::scan_ordinary, 0, true},
    {"RV_MANY_SCAN_LARGE", &rv_many::scan_large, 0, true},
    {"RV_MANY_SCAN_LARGE_MIN", &rv_many::scan_large_min, 0, false},
};
int many_set_option(rv_many *m, const char *name, int64_t rv_many::*field, int64_t lo, bool boolean, int64_t value) {
    if (value < lo && !boolean) {
        if (lo == 0) rv_set_error("%s: negative", name); else rv_set_error("%s: at least %lld", name, (long long)lo);
        return -1;
    }
    m->*field = boolean ? (int64_t)(value != 0) : value;
    return 0;
}

}  // namespace

#define MANY_GUARD(body, fail)                                                                                   \
    try { body }                                                                                                 \
    catch (const std::exception &e) { rv_set_error("rv_many: %s", e.what()); return fail; }                      \
    catch (...) { rv_set_error("rv_many: failed"); return fail; }

extern "C" {

rv_many *rv_many_new(int device) {
    const int nd = rv_device_count();
    if (nd <= 0) { rv_set_error("no HIP device visible: reveal_amd has no CPU fallback"); return nullptr; }
    if (device < 0 || device >= nd) { rv_set_error("device %d out of range (%d visible)", device, nd); return nullptr; }
    MANY_GUARD(rv_many *m = new rv_many(); m->device = device; return m;, nullptr)
}

void rv_many_free(rv_many *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->hs) rv_free(m->hs);
    if (m->ho) rv_free(m->ho);
    m->dJobs.release(); m->dKJobs.release(); m->dSA.release(); m->dLCP.release(); m->dBWT.release(); m->dCnt.release();
    m->dScanTab.release(); m->dScanCnt.release(); m->dScanFirst.release(); m->dScanOut.release();
    m->dKcStage.release(); m->dKcJob.release(); m->dKcOut.release(); m->kc_big_bufs.release();
    m->dTxt.release(); m->dMJobs.release(); m->dAn.release(); m->dAnPos.release(); m->dFlag.release(); m->dBeg.release();
    m->large_bufs.release();
    delete m;
}

int rv_many_option(rv_many *m, const char *name, int64_t value) {
    if (!m || !name) { rv_set_error("rv_many_option: null argument"); return -1; }
    for (const ManyClass &c : many_classes) {
        if (c.sw_name && strcmp(name, c.sw_name) == 0) return many_set_option(m, name, c.sw, 0, true, value);
        if (c.min_name && strcmp(name, c.min_name) == 0) return many_set_option(m, name, c.min, 0, false, value);
    }
    for (const ManyOption &o : many_options) if (strcmp(name, o.name) == 0) return many_set_option(m, name, o.field, o.lo, o.boolean, value);
    RvOptions probe;
    if (!probe.find(name)) { rv_set_error("rv_many_option: unknown option %s", name); return -1; }
    MANY_GUARD(
        m->fwd.push_back({std::string(name), value});
        if (m->hs) RV_TRY(rv_set_option(m->hs, name, value));
        if (m->ho) RV_TRY(rv_set_option(m->ho, name, value));
        return 0;, -1)
}

int rv_many_set_picker(rv_many *m, int kind, const rv_picker_args *args) {
    if (!m) { rv_set_error("rv_many_set_picker: null handle"); return -1; }
    if (kind != 0 && kind != 1) { rv_set_error("rv_many_set_picker: picker kind 0 (built-in) or 1 (the reference's default picker), not %d", kind); return -1; }
    if (kind == 1 && !args) { rv_set_error("rv_many_set_picker: kind 1 needs its options"); return -1; }
    if (kind == 1 && (args->gcmodel < 0 || args->gcmodel > 2)) { rv_set_error("rv_many_set_picker: gap cost model 0 (sumofpairs), 1 (star-avg) or 2 (star-med)"); return -1; }
    m->picker = kind;
    if (kind == 1) m->pargs = *args;
    return 0;
}

int64_t rv_many_add(rv_many *m, const char *const *seqs, const int64_t *lens, int k) {
    if (!m || !seqs || !lens) { rv_set_error("rv_many_add: null argument"); return -1; }
    if (k < 2) { rv_set_error("rv_many_add: a job needs at least two sequences (%d given)", k); return -1; }
    int64_t ranks = 0; bool clean = true;
    for (int s = 0; s < k; s++) {
        if (!seqs[s] || lens[s] < 1) { rv_set_error("rv_many_add: sequence %d of the job is empty", s); return -1; }
        for (int64_t i = 0; i < lens[s]; i++) {
            const uint8_t ch = (uint8_t)seqs[s][i];
            if (ch & 0x80u) { rv_set_error("addsequence: the sequence contains non-ASCII bytes"); return -1; }
            if (ch == 0) clean = false;
        }
        ranks += lens[s] + 1;
    }
    if (m->jobs.size() >= (size_t)INT_MAX - 1) { rv_set_error("rv_many_add: too many jobs"); return -1; }
    MANY_GUARD(
        ManyJob jb; jb.k = k; jb.seq0 = m->lens.size(); jb.ranks = ranks; jb.clean = clean;
        for (int s = 0; s < k; s++) {
            m->starts.push_back((int64_t)m->in.size()); m->lens.push_back(lens[s]);
            m->in.insert(m->in.end(), seqs[s], seqs[s] + lens[s]);
        }
        m->jobs.push_back(jb);
        m->ran = false; m->scanned = false; m->chained = false;
        return (int64_t)m->jobs.size() - 1;, -1)
}

int rv_many_clear(rv_many *m) {
    if (!m) { rv_set_error("rv_many_clear: null handle"); return -1; }
    m->in.clear(); m->lens.clear(); m->starts.clear(); m->jobs.clear();
    m->an_first.clear(); m->an_l.clear(); m->an_off.clear(); m->an_pos.clear(); m->out_text.clear(); m->keep_sa.clear(); m->keep_lcp.clear();
    m->mt_first.clear(); m->mt_l.clear(); m->mt_n.clear(); m->mt_off.clear(); m->mt_so.clear(); m->mt_pos.clear();
    m->kch_first.clear(); m->kch_l.clear(); m->kch_score.clear(); m->kch_pos.clear(); m->kch_end.clear();
    m->ran = false; m->scanned = false; m->chained = false;
    return 0;
}

int rv_many_run(rv_many *m, int minl, int minn, rv_align_stats *total) {
    if (!m) { rv_set_error("rv_many_run: null handle"); return -1; }
    MANY_GUARD(return many_run(m, minl, minn, total);, -1)
}

int rv_many_scan(rv_many *m, int minl, int minn, int kind) {
    if (!m) { rv_set_error("rv_many_scan: null handle"); return -1; }
    if (kind < 0 || kind > 2) { rv_set_error("rv_many_scan: kind 0 (getmums), 1 (getmultimums) or 2 (getmums for the jobs of two sequences, getmultimums for the rest), not %d", kind); return -1; }
    if (minl < 0) { rv_set_error("rv_many_scan: a negative minimal length"); return -1; }
    MANY_GUARD(return many_scan(m, minl, minn, kind);, -1)
}

int rv_many_kchain(rv_many *m, int minl, int64_t maxmums, int64_t wpen, int64_t wscore, int gcmodel) {
    if (!m) { rv_set_error("rv_many_kchain: null handle"); return -1; }
    if (minl < 0 || maxmums < 0) { rv_set_error("rv_many_kchain: a negative minimal length or maxmums"); return -1; }
    if (gcmodel < 0 || gcmodel > 2) { rv_set_error("rv_many_kchain: gap cost model 0 (sumofpairs), 1 (star-avg) or 2 (star-med)"); return -1; }
    if (wpen < 0 || wpen > RV_KCHAIN_WMAX || wscore < 0 || wscore > RV_KCHAIN_WMAX) { rv_set_error("rv_many_kchain: weights of 0 .. 2^20 (64-bit scores)"); return -1; }
    MANY_GUARD(
        RvKchainArgs A;
        A.maxmums = maxmums; A.wpen = wpen; A.wscore = wscore; A.gcmodel = gcmodel;
        A.cap = (int)std::min<int64_t>(std::max<int64_t>(many_fwd_option(m, "RV_KCHAIN_CAP", RV_KCHAIN_CAP), 0), RV_KCHAIN_CAP);
        return many_scan(m, minl, 2, 1, &A);, -1)
}

int rv_many_kchain_big(const rv_many *m, int64_t *out) {
    if (!m || !out) { rv_set_error("rv_many_kchain_big: null argument"); return -1; }
    out[0] = m->kc_big[0]; out[1] = m->kc_big[1];
    return 0;
}

int rv_many_kchain_lists(rv_many *m, int64_t nlists, const int32_t *k, const int64_t *nrec, const uint32_t *l, const int32_t *n, const int64_t *off, const uint16_t *so,
                         const int64_t *pos, const int64_t *lens, int64_t maxmums, int64_t wpen, int64_t wscore, int gcmodel) {
    if (!m || nlists < 0 || (nlists > 0 && (!k || !nrec || !lens || !off))) { rv_set_error("rv_many_kchain_lists: null handle or argument"); return -1; }
    if (maxmums < 0) { rv_set_error("rv_many_kchain_lists: a negative maxmums"); return -1; }
    if (gcmodel < 0 || gcmodel > 2) { rv_set_error("rv_many_kchain_lists: gap cost model 0 (sumofpairs), 1 (star-avg) or 2 (star-med)"); return -1; }
    if (wpen < 0 || wpen > RV_KCHAIN_WMAX || wscore < 0 || wscore > RV_KCHAIN_WMAX) { rv_set_error("rv_many_kchain_lists: weights of 0 .. 2^20 (64-bit scores)"); return -1; }
    MANY_GUARD(
        RV_HIP(hipSetDevice(m->device));
        m->ran = false; m->scanned = false; m->chained = false;
        for (int x = 0; x < 5; x++) m->info[x] = 0;
        for (int x = 0; x < 8; x++) m->flagged[x] = 0;
        m->kc_big[0] = m->kc_big[1] = 0;
        m->info[0] = nlists;
        m->kc_host = many_fwd_option(m, "RV_MANY_KCHAIN_HOST", 0) != 0;
        m->kc_l.clear(); m->kc_score.clear(); m->kc_pos.clear();
        RvKchainArgs A;
        A.maxmums = maxmums; A.wpen = wpen; A.wscore = wscore; A.gcmodel = gcmodel; A.cap = 0;
        std::vector<ManyKchainSlice> slices((size_t)nlists);
        std::vector<ManyKchainSrc> src;
        std::vector<int> ks((size_t)nlists);
        int64_t r0 = 0; int64_t s0 = 0;
        for (int64_t x = 0; x < nlists; x++) {
            if (k[x] < 2 || nrec[x] < 0) { rv_set_error("rv_many_kchain_lists: list %lld has %d sequences and %lld records", (long long)x, k[x], (long long)nrec[x]); return -1; }
            if (nrec[x] > 0 && (!l || !n || !so || !pos)) { rv_set_error("rv_many_kchain_lists: records without their arrays"); return -1; }
            for (int64_t r = r0; r < r0 + nrec[x]; r++) if (off[r] < 0 || off[r] > off[r + 1]) { rv_set_error("rv_many_kchain_lists: offsets that do not ascend"); return -1; }
            // (rv_kchain's offsets index pos / so as given: each list keeps the whole arrays and its own stretch of the records)
            src.push_back({k[x], nrec[x], l ? l + r0 : nullptr, n ? n + r0 : nullptr, off + r0, so, pos, lens + s0, &slices[(size_t)x]});
            ks[(size_t)x] = k[x];
            r0 += nrec[x]; s0 += k[x];
        }
        RV_TRY(many_kchain_rest(m, src, A));
        many_kchain_collect(m, slices, ks);
        m->kc_l.clear(); m->kc_score.clear(); m->kc_pos.clear();
        m->chained = true;
        return 0;, -1)
}

int64_t rv_many_kchain_count(rv_many *m, int64_t *first, int64_t *members) {
    if (!m || !m->chained) { rv_set_error("rv_many_kchain_count: no finished rv_many_kchain (the live result is the last call's)"); return -1; }
    if (first) for (size_t k = 0; k < m->kch_first.size(); k++) first[k] = m->kch_first[k];
    if (members) *members = (int64_t)m->kch_pos.size();
    return (int64_t)m->kch_l.size();
}

int rv_many_kchain_fetch(rv_many *m, uint32_t *l, int64_t *score, int64_t *pos, int64_t *end_score) {
    if (!m || !m->chained || !l || !score || !pos || !end_score) { rv_set_error("rv_many_kchain_fetch: no finished rv_many_kchain, or null argument"); return -1; }
    if (!m->kch_l.empty()) { memcpy(l, m->kch_l.data(), m->kch_l.size() * sizeof(u32)); memcpy(score, m->kch_score.data(), m->kch_score.size() * sizeof(int64_t)); }
    if (!m->kch_pos.empty()) memcpy(pos, m->kch_pos.data(), m->kch_pos.size() * sizeof(int64_t));
    if (!m->kch_end.empty()) memcpy(end_score, m->kch_end.data(), m->kch_end.size() * sizeof(int64_t));
    return 0;
}

int64_t rv_many_match_count(rv_many *m, int64_t *first, int64_t *members) {
    if (m && m->ran) { rv_set_error("rv_many_match_count: the live result is a run's (rv_many_run): it has anchors, no match lists"); return -1; }
    if (!m || !m->scanned) { rv_set_error("rv_many_match_count: no finished scan"); return -1; }
    if (first) for (size_t k = 0; k < m->mt_first.size(); k++) first[k] = m->mt_first[k];
    if (members) *members = (int64_t)m->mt_pos.size();
    return (int64_t)m->mt_l.size();
}

int rv_many_fetch_matches(rv_many *m, uint32_t *l, int32_t *n, int64_t *off, uint16_t *so, int64_t *pos) {
    if (m && m->ran) { rv_set_error("rv_many_fetch_matches: the live result is a run's (rv_many_run): it has anchors, no match lists"); return -1; }
    if (!m || !m->scanned || !l || !n || !off || !so || !pos) { rv_set_error("rv_many_fetch_matches: no finished scan, or null argument"); return -1; }
    if (!m->mt_l.empty()) { memcpy(l, m->mt_l.data(), m->mt_l.size() * sizeof(u32)); memcpy(n, m->mt_n.data(), m->mt_n.size() * sizeof(int32_t)); }
    memcpy(off, m->mt_off.data(), m->mt_off.size() * sizeof(int64_t));
    if (!m->mt_pos.empty()) { memcpy(so, m->mt_so.data(), m->mt_so.size() * sizeof(uint16_t)); memcpy(pos, m->mt_pos.data(), m->mt_pos.size() * sizeof(int64_t)); }
    return 0;
}

int64_t rv_many_anchor_count(rv_many *m, int64_t *first, int64_t *members) {
    if (m && m->scanned) { rv_set_error("rv_many_anchor_count: the live result is a scan's (rv_many_scan): it has matches, no anchors"); return -1; }
    if (!m || !m->ran) { rv_set_error("rv_many_anchor_count: no finished run"); return -1; }
    if (first) for (size_t k = 0; k < m->an_first.size(); k++) first[k] = m->an_first[k];
    if (members) *members = (int64_t)m->an_pos.size();
    return (int64_t)m->an_l.size();
}

int rv_many_fetch(rv_many *m, uint32_t *l, int64_t *off, int64_t *pos) {
    if (m && m->scanned) { rv_set_error("rv_many_fetch: the live result is a scan's (rv_many_scan): it has matches, no anchors"); return -1; }
    if (!m || !m->ran || !l || !off || !pos) { rv_set_error("rv_many_fetch: no finished run, or null argument"); return -1; }
    if (!m->an_l.empty()) memcpy(l, m->an_l.data(), m->an_l.size() * sizeof(u32));
    memcpy(off, m->an_off.data(), m->an_off.size() * sizeof(int64_t));
    if (!m->an_pos.empty()) memcpy(pos, m->an_pos.data(), m->an_pos.size() * sizeof(int64_t));
    return 0;
}

int64_t rv_many_text(rv_many *m, int64_t job, char *out, int64_t cap) {
    if (m && m->scanned) { rv_set_error("rv_many_text: the live result is a scan's (rv_many_scan), which leaves the jobs' text as it was given"); return -1; }
    if (!m || !m->ran || job < 0 || job >= (int64_t)m->jobs.size() || !out) { rv_set_error("rv_many_text: no finished run, or no such job"); return -1; }
    const ManyJob &jb = m->jobs[(size_t)job];
    if (cap < jb.ranks) { rv_set_error("buffer too small"); return -1; }
    memcpy(out, m->out_text.data() + jb.text_off, (size_t)jb.ranks);
    return jb.ranks;
}

int rv_many_flagged(const rv_many *m, int64_t *out) {
    if (!m || !out) { rv_set_error("rv_many_flagged: null argument"); return -1; }
    for (int k = 0; k < 8; k++) out[k] = m->flagged[k];
    return 0;
}

int rv_many_info(const rv_many *m, int64_t *out) {
    if (!m || !out) { rv_set_error("rv_many_info: null argument"); return -1; }
    for (int k = 0; k < 5; k++) out[k] = m->info[k];
    return 0;
}

int64_t rv_many_arrays(rv_many *m, int64_t job, int which, void *out, int64_t cap) {
    if (!m || !(m->ran || m->scanned || m->chained) || job < 0 || job >= (int64_t)m->jobs.size() || !out) { rv_set_error("rv_many_arrays: no finished run or scan, or no such job"); return -1; }
    const ManyJob &jb = m->jobs[(size_t)job];
    if (jb.arr_off < 0) { rv_set_error("rv_many_arrays: job %lld did not go through the shared launches with RV_MANY_KEEP set", (long long)job); return -2; }
    if (cap < jb.ranks) { rv_set_error("buffer too small"); return -1; }
    if (which == RV_SA) memcpy(out, m->keep_sa.data() + jb.arr_off, (size_t)jb.ranks * sizeof(sa_t));
    else if (which == RV_LCP) memcpy(out, m->keep_lcp.data() + jb.arr_off, (size_t)jb.ranks * sizeof(lcp_t));
    else { rv_set_error("rv_many_arrays: RV_SA or RV_LCP"); return -1; }
    return jb.ranks;
}

}  // extern "C"
