// rv_many_large.hip -- index build for rv_many's rounds of pair jobs above RV_LEAF_N ranks (RV_MANY_LARGE, include/reveal_amd.h "many small
// alignments"): a segmented prefix doubling in HBM over every job of the round at once.
//
// k_many_build (rv_many.hip) sorts a job in LDS: 11 B per rank, 2048 ranks.  A bubble of `reveal refine` holds alleles of up to 10 kbp -- 20 000
// ranks -- so these jobs are sorted together in memory instead.  Everything works in segment coordinates: element off_j + p is local position p
// of job j's stand-alone text a_j$b_j$, and the job's ranks are [off_j, off_j + n_j) -- where rv_frontier_import expects its segment.  The
// semantics are k_many_build's: comparisons follow the job-local text, past its end a comparison reads 0 (a suffix that is a prefix of another
// sorts first, suffixes that tie through a '$' come out in the stand-alone order), nothing compares across jobs.
//   gather    the job-local texts into one buffer, and the job's number per element
//   first key job number << 35 | five text characters of 7 bits (past the end: 0), value = element; one radix sort over 55 bits.  The job
//             number on top makes the sort segmented: job j's elements end up in [off_j, off_j + n_j)
//   rank      an element's rank = 1 + the first sorted place of its run of equal keys: heads, an inclusive maximum, a scatter.  Such a rank
//             is global (off_j + 1 + local), so it keeps the segments apart in the rounds that follow
//   rounds    key = rank[e] << b2 | (rank[e + h] - off_j, or 0 when p + h >= n_j), h = 5, 10, 20 ..; b2 = bits of the largest job.  The first
//             rank always takes 31 bits -- not the bits of the round's size -- so that the radix passes, and with them the launches, do not
//             depend on how many jobs the round holds.  Device flags say whether a run longer than one is left; the host reads them once a round
//   finish    text order with Kasai's carry, a thread per 16 consecutive elements (the carry starts afresh at a job's first position): LCP with
//             the reference's stops at '$' and 'N' (interface.c:97-114), eight bytes per step; SA in shared-text positions; the BWT byte
// Every kernel is a streaming pass of a few bytes per element, plus the gather rank[e + h] inside a job's segment.
// Three forms share the passes in between (ml_build's JobT): the pair rounds (ManyDevJob), the sample-major rounds of 3 .. 64 sequences (ManyDevJobK), and
// the job-contiguous rounds of rv_many_scan (ManyDevJobC, 2 .. 64 sequences): there a job's stand-alone text IS [off_j, off_j + n_j) of the round's text, so
// nothing is gathered -- the build reads the round's text in place -- and an element is its own text position.
#include "rv_many_large.h"
#include "rv_index.h"
#include <type_traits>

namespace {

constexpr int LT = 256;                    // threads per workgroup
constexpr int FIRST_CHARS = 5;             // characters of the first key
constexpr int JOB_BITS = 20;               // (a job holds more than 2^11 ranks, a round fewer than 2^31)
constexpr int RANK_BITS = 31;
constexpr int FIN_CHUNK = 16;              // consecutive elements a thread of the finish takes
constexpr int MAX_ROUNDS = 40;
constexpr int TIE_SLOTS = 1024;            // words of the tie flag: a workgroup marks slot blockIdx % TIE_SLOTS, the host reads them all

__device__ inline u64 ml_zero_bytes(u64 v) { return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull; }

// the first rank behind a job's segment
template <class JobT>
__device__ inline int64_t ml_end(const JobT *jobs, u32 j, int64_t n) {
    if constexpr (std::is_same_v<JobT, ManyDevJobK>) {      // never behind the round's last element, whatever a descriptor the gather has refused says
        const int64_t end = jobs[j].off + jobs[j].n;
        return end < n ? end : n;
    } else if constexpr (std::is_same_v<JobT, ManyDevJobC>) {      // the same: k_mlc_jobs may have refused it
        const int64_t end = jobs[j].off + jobs[j].n;
        return end < n ? end : n;
    } else return jobs[j].off + jobs[j].la + jobs[j].lb + 2;
}

__global__ __launch_bounds__(LT) void k_ml_gather(const ManyDevJob *__restrict__ jobs, int njobs, int64_t n, const uint8_t *__restrict__ T,
                                                   uint8_t *__restrict__ txt, u32 *__restrict__ job, u32 *__restrict__ d_err) {
    const int64_t e = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (e >= n) return;
    int lo = 0, hi = njobs;                // the last job whose segment begins at or in front of e
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (jobs[mid].off <= e) lo = mid; else hi = mid; }
    const ManyDevJob J = jobs[lo];
    const int64_t p = e - J.off, la = J.la;
    if (p < 0 || p >= la + (int64_t)J.lb + 2 || J.la < 1 || J.lb < 1) { atomicOr(d_err, 1u); txt[e] = (uint8_t)'$'; job[e] = (u32)lo; return; }
    txt[e] = p <= la ? T[J.abeg + p] : T[J.bbeg + (p - la - 1)];
    job[e] = (u32)lo;
}

template <class JobT>
__global__ __launch_bounds__(LT) void k_ml_first_keys(const JobT *__restrict__ jobs, int64_t n, const uint8_t *__restrict__ txt, const u32 *__restrict__ job,
                                                       u64 *__restrict__ key, u32 *__restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (e >= n) return;
    const u32 j = job[e];
    const int64_t rem = ml_end(jobs, j, n) - e;      // characters the job has left from e on
    u64 w;
    __builtin_memcpy(&w, txt + e, 8);      // (the buffer is padded behind n)
    u64 k = 0;
#pragma unroll
    for (int b = 0; b < FIRST_CHARS; b++) k = (k << 7) | (b < rem ? (w >> (8 * b)) & 0x7Full : 0ull);
    key[e] = ((u64)j << (7 * FIRST_CHARS)) | k;
    val[e] = (u32)e;
}

// head[i] = i + 1 where a run of equal keys begins in the sorted order, else 0; d_tied[TIE_SLOTS]: some run is longer than one.  (One flag
// word for all: 177 000 wavefronts at 1.1e7 elements queued at one address, 168 us per launch against 40 us of streaming.)
__global__ __launch_bounds__(LT) void k_ml_heads(const u64 *__restrict__ key, int64_t n, u32 *__restrict__ head, u32 *__restrict__ d_tied) {
    const int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x;
    bool tie = false;
    if (i < n) {
        const bool first = i == 0 || key[i - 1] != key[i];
        head[i] = first ? (u32)i + 1u : 0u;
        tie = !first;
    }
    if (__syncthreads_or(tie ? 1 : 0) && threadIdx.x == 0) d_tied[blockIdx.x % TIE_SLOTS] = 1u;
}

__global__ __launch_bounds__(LT) void k_ml_ranks(const u32 *__restrict__ val, const u32 *__restrict__ run, int64_t n, u32 *__restrict__ rank) {
    const int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (i < n) rank[val[i]] = run[i];
}

template <class JobT>
__global__ __launch_bounds__(LT) void k_ml_pair_keys(const JobT *__restrict__ jobs, int64_t n, const u32 *__restrict__ job, const u32 *__restrict__ rank,
                                                      int64_t h, int b2, u64 *__restrict__ key, u32 *__restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (e >= n) return;
    const u32 j = job[e];
    const int64_t off = jobs[j].off, end = ml_end(jobs, j, n);
    const u64 r1 = rank[e], r2 = e + h < end ? (u64)(rank[e + h] - (u32)off) : 0ull;
    key[e] = (r1 << b2) | r2;
    val[e] = (u32)e;
}

__global__ __launch_bounds__(LT) void k_ml_finish(const ManyDevJob *__restrict__ jobs, int64_t n, const uint8_t *__restrict__ txt, const u32 *__restrict__ job,
                                                   const u32 *__restrict__ rank, const u32 *__restrict__ order, sa_t *__restrict__ SA, lcp_t *__restrict__ LCP,
                                                   uint8_t *__restrict__ BWT, u32 *__restrict__ d_maxlcp) {
    const int64_t e0 = ((int64_t)blockIdx.x * LT + threadIdx.x) * FIN_CHUNK;
    u32 lmax = 0, jcur = ~0u;
    int64_t off = 0, la = 0, abeg = 0, bbeg = 0, hh = 0;
    for (int64_t e = e0; e < e0 + FIN_CHUNK && e < n; e++) {
        const u32 j = job[e];
        if (j != jcur) { const ManyDevJob J = jobs[j]; off = J.off; la = J.la; abeg = J.abeg; bbeg = J.bbeg; jcur = j; hh = 0; }      // (a job's first position: no carry)
        const int64_t p = e - off, k = (int64_t)rank[e] - 1;
        if (k > off) {
            const int64_t q = order[k - 1];
            for (;;) {
                u64 a, b;
                __builtin_memcpy(&a, txt + e + hh, 8);
                __builtin_memcpy(&b, txt + q + hh, 8);
                const u64 x = a ^ b, z = ml_zero_bytes(a ^ 0x2424242424242424ull) | ml_zero_bytes(a ^ 0x4E4E4E4E4E4E4E4Eull);      // '$', 'N'
                const int m = x ? (int)(__builtin_ctzll(x) >> 3) : 8, s = z ? (int)(__builtin_ctzll(z) >> 3) : 8;
                const int step = m < s ? m : s;
                hh += step;
                if (step < 8) break;       // (a job's text ends with '$': no comparison runs past it)
            }
            LCP[k] = (lcp_t)hh;
            if ((u32)hh > lmax) lmax = (u32)hh;
        } else { LCP[k] = 0; hh = 0; }     // the job's first rank
        SA[k] = (sa_t)(p <= la ? abeg + p : bbeg + (p - la - 1));
        BWT[k] = (uint8_t)((p > 0 ? txt[e - 1] : (uint8_t)'$') | (p > la ? RV_BWT_SIDE : 0u));
        if (hh > 0) hh--;
    }
    lmax = (u32)rv_wave_max_u64((u64)lmax);
    if ((threadIdx.x & 63) == 0 && lmax > __atomic_load_n(d_maxlcp, __ATOMIC_RELAXED)) atomicMax(d_maxlcp, lmax);
}

// The gather of a sample-major round: element -> job by the search in the offsets, local position -> sequence by a scan of the (at most RV_MANY_WIDE_KMAX)
// prefix ends, byte from the shared text.  The thread of a job's first element checks the whole descriptor; every thread checks what it reads
// with: a malformed descriptor sets the error word and reads nothing outside T.
__global__ __launch_bounds__(LT) void k_mlk_gather(const ManyDevJobK *__restrict__ jobs, int njobs, int64_t n, const uint8_t *__restrict__ T, int64_t nT,
                                                   uint8_t *__restrict__ txt, u32 *__restrict__ job, u32 *__restrict__ d_err) {
    const int64_t e = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (e >= n) return;
    int lo = 0, hi = njobs;                // the last job whose segment begins at or in front of e
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (jobs[mid].off <= e) lo = mid; else hi = mid; }
    const ManyDevJobK *J = jobs + lo;
    const int64_t p = e - J->off;
    const int k = J->k, nj = J->n;
    job[e] = (u32)lo;
    bool bad = k < 3 || k > RV_MANY_WIDE_KMAX || p < 0 || p >= nj;
    uint8_t ch = (uint8_t)'$';
    if (!bad) {
        if (p == 0) {                      // the whole descriptor, once per job: its sequences, and its segment between its neighbours
            if (J->off + nj != (lo + 1 < njobs ? jobs[lo + 1].off : n)) bad = true;
            int prev = 0;
            for (int q = 0; q < k; q++) { const int pe = J->pend[q]; if (pe - prev < 2) bad = true; prev = pe; }      // (a sequence of at least one base and its '$')
            if (prev != nj) bad = true;
        }
        int q = 0, prev = 0;
        while (q < k - 1 && p >= J->pend[q]) prev = J->pend[q++];
        const int64_t src = J->beg[q] + (p - prev);
        if (p < prev || p >= J->pend[q] || src < 0 || src >= nT) bad = true;
        else ch = T[src];
    }
    if (bad) atomicOr(d_err, 1u);
    txt[e] = ch;
}

// The finish of a sample-major round: k_ml_finish with the position map of k sequences.  A thread walks 16 consecutive elements, so the sequence
// of the local position moves forward with it; the side bit of the BWT byte is "behind the first sequence's '$'" (p > la, la = pend[0] - 1).
// Where the gather has refused a descriptor the kernel does nothing: the host reports the error word.
__global__ __launch_bounds__(LT) void k_mlk_finish(const ManyDevJobK *__restrict__ jobs, int64_t n, const uint8_t *__restrict__ txt, const u32 *__restrict__ job,
                                                    const u32 *__restrict__ rank, const u32 *__restrict__ order, sa_t *__restrict__ SA, lcp_t *__restrict__ LCP,
                                                    uint8_t *__restrict__ BWT, u32 *__restrict__ d_maxlcp, const u32 *__restrict__ d_err) {
    if (__atomic_load_n(d_err, __ATOMIC_RELAXED)) return;      // (a text the gather did not finish need not end in '$')
    const int64_t e0 = ((int64_t)blockIdx.x * LT + threadIdx.x) * FIN_CHUNK;
    u32 lmax = 0, jcur = ~0u;
    const ManyDevJobK *J = jobs;
    int64_t off = 0, la = 0, hh = 0, sbeg = 0;      // sbeg: shared-text position of local position 0 of the current sequence, minus its local begin
    int q = 0, kk = 0, pe = 0;
    for (int64_t e = e0; e < e0 + FIN_CHUNK && e < n; e++) {
        const u32 j = job[e];
        if (j != jcur) { J = jobs + j; off = J->off; la = J->pend[0] - 1; kk = J->k < RV_MANY_WIDE_KMAX ? J->k : RV_MANY_WIDE_KMAX; jcur = j; hh = 0; q = 0; pe = J->pend[0]; sbeg = J->beg[0]; }      // (a job's first position: no carry)
        const int64_t p = e - off, k = (int64_t)rank[e] - 1;
        while (q < kk - 1 && p >= pe) { sbeg = J->beg[q + 1] - pe; pe = J->pend[++q]; }
        if (k > off) {
            const int64_t o = order[k - 1];
            for (;;) {
                u64 a, b;
                __builtin_memcpy(&a, txt + e + hh, 8);
                __builtin_memcpy(&b, txt + o + hh, 8);
                const u64 x = a ^ b, z = ml_zero_bytes(a ^ 0x2424242424242424ull) | ml_zero_bytes(a ^ 0x4E4E4E4E4E4E4E4Eull);      // '$', 'N'
                const int m = x ? (int)(__builtin_ctzll(x) >> 3) : 8, s = z ? (int)(__builtin_ctzll(z) >> 3) : 8;
                const int step = m < s ? m : s;
                hh += step;
                if (step < 8) break;       // (a job's text ends with '$': no comparison runs past it)
            }
            LCP[k] = (lcp_t)hh;
            if ((u32)hh > lmax) lmax = (u32)hh;
        } else { LCP[k] = 0; hh = 0; }     // the job's first rank
        SA[k] = (sa_t)(sbeg + p);
        BWT[k] = (uint8_t)((p > 0 ? txt[e - 1] : (uint8_t)'$') | (p > la ? RV_BWT_SIDE : 0u));
        if (hh > 0) hh--;
    }
    lmax = (u32)rv_wave_max_u64((u64)lmax);
    if ((threadIdx.x & 63) == 0 && lmax > __atomic_load_n(d_maxlcp, __ATOMIC_RELAXED)) atomicMax(d_maxlcp, lmax);
}

// The first kernel of a job-contiguous round (ManyDevJobC): the job of every element, by the search in the offsets.  Nothing is gathered -- the round's
// text is the build's text in place.  The thread of a job's first element checks the whole descriptor: its segment back to back with its neighbours'
// inside [0, n), at least s$t$ (n >= 4, 1 <= la <= n - 3), a '$' behind the first sequence and at the job's end (the finish relies on the last one: its
// comparisons stop there).  A malformed descriptor sets the error word; T is read inside [0, n) only, and only where the descriptor has passed.
__global__ __launch_bounds__(LT) void k_mlc_jobs(const ManyDevJobC *__restrict__ jobs, int njobs, int64_t n, const uint8_t *__restrict__ T,
                                                  u32 *__restrict__ job, u32 *__restrict__ d_err) {
    const int64_t e = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (e >= n) return;
    int lo = 0, hi = njobs;                // the last job whose segment begins at or in front of e
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (jobs[mid].off <= e) lo = mid; else hi = mid; }
    const ManyDevJobC J = jobs[lo];
    const int64_t p = e - J.off, nj = J.n, la = J.la;
    job[e] = (u32)lo;
    bool bad = p < 0 || p >= nj;
    if (!bad && p == 0) {                  // (off == e: inside [0, n))
        const int64_t end = J.off + nj;
        if (end > n || end != (lo + 1 < njobs ? jobs[lo + 1].off : n)) bad = true;
        if (nj < 4 || la < 1 || la > nj - 3) bad = true;
        if (!bad && (T[J.off + la] != (uint8_t)'$' || T[end - 1] != (uint8_t)'$')) bad = true;
    }
    if (bad) atomicOr(d_err, 1u);
}

// The finish of a job-contiguous round: k_ml_finish where an element IS its position of the shared text (SA[k] = e), the side bit of the BWT byte is
// "behind the first sequence's '$'" (p > la).  Kasai's carry starts afresh at a job's first position; the LCP stops at '$' and 'N'.  Where k_mlc_jobs
// has refused a descriptor the kernel does nothing (a text it did not check need not end in '$'): the host reports the error word.
__global__ __launch_bounds__(LT) void k_mlc_finish(const ManyDevJobC *__restrict__ jobs, int64_t n, const uint8_t *__restrict__ txt, const u32 *__restrict__ job,
                                                    const u32 *__restrict__ rank, const u32 *__restrict__ order, sa_t *__restrict__ SA, lcp_t *__restrict__ LCP,
                                                    uint8_t *__restrict__ BWT, u32 *__restrict__ d_maxlcp, const u32 *__restrict__ d_err) {
    if (__atomic_load_n(d_err, __ATOMIC_RELAXED)) return;
    const int64_t e0 = ((int64_t)blockIdx.x * LT + threadIdx.x) * FIN_CHUNK;
    u32 lmax = 0, jcur = ~0u;
    int64_t off = 0, la = 0, hh = 0;
    for (int64_t e = e0; e < e0 + FIN_CHUNK && e < n; e++) {
        const u32 j = job[e];
        if (j != jcur) { const ManyDevJobC J = jobs[j]; off = J.off; la = J.la; jcur = j; hh = 0; }      // (a job's first position: no carry)
        const int64_t p = e - off, k = (int64_t)rank[e] - 1;
        if (k > off) {
            const int64_t o = order[k - 1];
            for (;;) {
                u64 a, b;
                __builtin_memcpy(&a, txt + e + hh, 8);
                __builtin_memcpy(&b, txt + o + hh, 8);
                const u64 x = a ^ b, z = ml_zero_bytes(a ^ 0x2424242424242424ull) | ml_zero_bytes(a ^ 0x4E4E4E4E4E4E4E4Eull);      // '$', 'N'
                const int m = x ? (int)(__builtin_ctzll(x) >> 3) : 8, s = z ? (int)(__builtin_ctzll(z) >> 3) : 8;
                const int step = m < s ? m : s;
                hh += step;
                if (step < 8) break;       // (a job's text ends with '$': no comparison runs past it)
            }
            LCP[k] = (lcp_t)hh;
            if ((u32)hh > lmax) lmax = (u32)hh;
        } else { LCP[k] = 0; hh = 0; }     // the job's first rank
        SA[k] = (sa_t)e;
        BWT[k] = (uint8_t)((p > 0 ? txt[e - 1] : (uint8_t)'$') | (p > la ? RV_BWT_SIDE : 0u));
        if (hh > 0) hh--;
    }
    lmax = (u32)rv_wave_max_u64((u64)lmax);
    if ((threadIdx.x & 63) == 0 && lmax > __atomic_load_n(d_maxlcp, __ATOMIC_RELAXED)) atomicMax(d_maxlcp, lmax);
}

int ml_bits(int64_t v) { int b = 1; while (b < 63 && ((int64_t)1 << b) <= v) b++; return b; }      // bits that hold 0 .. v

// kernels of the primitives (rv_prims.hip), for the launch count
int ml_scan_launches(int64_t n) { const int64_t nt = ceil_div(n, 2048); return nt <= 1 ? 1 : 2 + ml_scan_launches(nt); }
int ml_sort_launches(const Workspace &ws, int64_t n, int bits) {
    const int width = ws.opt.rs_bits == 10 ? 10 : 8;
    return rv_radix_passes(ws, bits) * (2 + ml_scan_launches(((int64_t)1 << width) * ceil_div(n, 4096)));
}

// JobT: ManyDevJob (pair rounds), ManyDevJobK (sample-major rounds: their own gather and finish; nT, the bytes of T, is theirs alone) or ManyDevJobC
// (job-contiguous rounds: no gather -- the build's text is T in place, padded by the caller --, their own first kernel and finish); the kernels in
// between only need a segment's end
template <class JobT>
int ml_build(Workspace &ws, RvManyLargeBufs &B, const JobT *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T, int64_t nT,
             sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches) {
    if (njobs < 1 || njobs >= ((int64_t)1 << JOB_BITS) || n < 1 || n >= ((int64_t)1 << RANK_BITS) || maxn < 1 || maxn > n) { rv_set_error("rv_many_run: a round of large jobs of bad sizes"); return -1; }
    const int b2 = ml_bits(maxn);          // a job-local rank is 0 .. maxn
    hipStream_t q = ws.stream;
    constexpr bool in_place = std::is_same_v<JobT, ManyDevJobC>;
    if (!in_place) RV_TRY(B.txt.reserve((size_t)n + 64));
    RV_TRY(B.job.reserve((size_t)n * sizeof(u32)));
    RV_TRY(B.rank.reserve((size_t)n * sizeof(u32)));
    RV_TRY(B.head.reserve((size_t)n * sizeof(u32)));
    for (int k = 0; k < 2; k++) { RV_TRY(B.key[k].reserve((size_t)n * sizeof(u64))); RV_TRY(B.val[k].reserve((size_t)n * sizeof(u32))); }
    uint8_t *gtxt = in_place ? nullptr : B.txt.as<uint8_t>();      // what a gather writes
    const uint8_t *txt = in_place ? T : gtxt;
    u32 *job = B.job.as<u32>(), *rank = B.rank.as<u32>(), *head = B.head.as<u32>();
    u64 *key[2] = {B.key[0].as<u64>(), B.key[1].as<u64>()};
    u32 *val[2] = {B.val[0].as<u32>(), B.val[1].as<u32>()};
    RV_TRY(B.flag.reserve(TIE_SLOTS * sizeof(u32)));
    u32 *d_max = d_cnt, *d_err = d_cnt + 1, *d_tied = B.flag.as<u32>();
    std::vector<u32> slots(TIE_SLOTS);
    const dim3 grid((unsigned)ceil_div(n, LT)), block(LT);
    if (!in_place) RV_HIP(hipMemsetAsync(gtxt + n, 0, 64, q));
    if constexpr (in_place) hipLaunchKernelGGL(k_mlc_jobs, grid, block, 0, q, djobs, (int)njobs, n, T, job, d_err);
    else if constexpr (std::is_same_v<JobT, ManyDevJobK>) hipLaunchKernelGGL(k_mlk_gather, grid, block, 0, q, djobs, (int)njobs, n, T, nT, gtxt, job, d_err);
    else hipLaunchKernelGGL(k_ml_gather, grid, block, 0, q, djobs, (int)njobs, n, T, gtxt, job, d_err);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ml_first_keys<JobT>, grid, block, 0, q, djobs, n, (const uint8_t *)txt, (const u32 *)job, key[0], val[0]);
    RV_LAUNCH_CHECK();
    *launches += 2;
    int cur = 0, bits = 7 * FIRST_CHARS + JOB_BITS;
    int64_t h = FIRST_CHARS;
    for (int round = 0;; round++) {
        RV_TRY(rv_radix_sort_pairs<u32>(ws, key[0], val[0], key[1], val[1], n, 0, bits, &cur));
        *launches += ml_sort_launches(ws, n, bits);
        RV_HIP(hipMemsetAsync(d_tied, 0, TIE_SLOTS * sizeof(u32), q));
        hipLaunchKernelGGL(k_ml_heads, grid, block, 0, q, (const u64 *)key[cur], n, head, d_tied);
        RV_LAUNCH_CHECK();
        RV_TRY(rv_inclusive_max_u32(ws, head, head, n));
        hipLaunchKernelGGL(k_ml_ranks, grid, block, 0, q, (const u32 *)val[cur], (const u32 *)head, n, rank);
        RV_LAUNCH_CHECK();
        *launches += 2 + ml_scan_launches(n);
        u32 tied = 0;
        RV_TRY(rv_read_back(ws, slots.data(), d_tied, TIE_SLOTS * sizeof(u32)));
        for (u32 x : slots) tied |= x;
        if (!tied) break;
        if (round >= MAX_ROUNDS) { rv_set_error("rv_many_run: the order of a round of large jobs is not final after %d doubling rounds", round); return -1; }      // (cannot happen: h passes 2^31 first)
        hipLaunchKernelGGL(k_ml_pair_keys<JobT>, grid, block, 0, q, djobs, n, (const u32 *)job, (const u32 *)rank, h, b2, key[0], val[0]);
        RV_LAUNCH_CHECK();
        (*launches)++;
        bits = RANK_BITS + b2;
        h <<= 1;
    }
    const dim3 fgrid((unsigned)ceil_div(ceil_div(n, FIN_CHUNK), LT));
    if constexpr (in_place)
        hipLaunchKernelGGL(k_mlc_finish, fgrid, block, 0, q, djobs, n, (const uint8_t *)txt, (const u32 *)job, (const u32 *)rank, (const u32 *)val[cur], SA, LCP, BWT, d_max, (const u32 *)d_err);
    else if constexpr (std::is_same_v<JobT, ManyDevJobK>)
        hipLaunchKernelGGL(k_mlk_finish, fgrid, block, 0, q, djobs, n, (const uint8_t *)txt, (const u32 *)job, (const u32 *)rank, (const u32 *)val[cur], SA, LCP, BWT, d_max, (const u32 *)d_err);
    else
        hipLaunchKernelGGL(k_ml_finish, fgrid, block, 0, q, djobs, n, (const uint8_t *)txt, (const u32 *)job, (const u32 *)rank, (const u32 *)val[cur], SA, LCP, BWT, d_max);
    RV_LAUNCH_CHECK();
    (*launches)++;
    return 0;
}

}  // namespace

int rv_many_large_build(Workspace &ws, RvManyLargeBufs &B, const ManyDevJob *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T,
                        sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches) {
    return ml_build(ws, B, djobs, njobs, n, maxn, T, 0, SA, LCP, BWT, d_cnt, launches);
}

int rv_many_large_build_k(Workspace &ws, RvManyLargeBufs &B, const ManyDevJobK *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T, int64_t nT,
                          sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches) {
    return ml_build(ws, B, djobs, njobs, n, maxn, T, nT, SA, LCP, BWT, d_cnt, launches);
}

int rv_many_large_build_c(Workspace &ws, RvManyLargeBufs &B, const ManyDevJobC *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T,
                          sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches) {
    return ml_build(ws, B, djobs, njobs, n, maxn, T, n, SA, LCP, BWT, d_cnt, launches);
}
