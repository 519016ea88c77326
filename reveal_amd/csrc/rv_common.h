// rv_common.h -- shared declarations of the reveal_amd HIP library (gfx950 only).
//
// Index-width switch exactly like the reference's two modules
// (reveallib/reveal.h:7-13): default = reveallib (int32 SA, int32 LCP),
// -DRV_SA64 = reveallib64 (int64 SA, uint32 LCP).
#pragma once
#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>
#include <utility>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stddef.h>
#include <vector>
#include <string>

#ifdef RV_SA64
typedef int64_t  sa_t;
typedef uint32_t lcp_t;
#else
typedef int32_t  sa_t;
typedef int32_t  lcp_t;
#endif

typedef unsigned long long u64;
typedef unsigned int       u32;

void rv_set_error(const char *fmt, ...);

#define RV_HIP(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            rv_set_error("%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
            return -1;                                                                         \
        }                                                                                      \
    } while (0)
#define RV_TRY(x)                                                                              \
    do {                                                                                       \
        int r_ = (x);                                                                          \
        if (r_ != 0) return r_;                                                                \
    } while (0)
// ---- switches (test hooks, diagnostics, A/B paths).  The library never reads the process environment: a handle starts with the
// defaults below and rv_set_option() (include/reveal_amd.h) changes one; the Python layer applies RV_* environment variables
// when it makes a handle (reveal_amd/_index.py).  name = the historical environment spelling.
#define RV_OPTION_LIST(X) \
    X(bubble_par_min, "RV_BUBBLE_PAR_MIN", -1) \
    X(presel_log, "RV_PRESEL_LOG", 0) \
    X(presel_host, "RV_PRESEL_HOST", 0) \
    X(leaf_acap, "RV_LEAF_ACAP", 256) \
    X(bubble_lds_always, "RV_BUBBLE_LDS_ALWAYS", 0) \
    X(no_early_bubble, "RV_NO_EARLY_BUBBLE", 0) \
    X(early_bubble_many, "RV_EARLY_BUBBLE_MANY", 0) \
    X(no_early_split, "RV_NO_EARLY_SPLIT", 0) \
    X(keep_dead, "RV_KEEP_DEAD", 0) \
    X(bubble_no_lds, "RV_BUBBLE_NO_LDS", 0) \
    X(bubble_no_join, "RV_BUBBLE_NO_JOIN", 0) \
    X(bubble_no_merge, "RV_BUBBLE_NO_MERGE", 0) \
    X(tables_memcpy, "RV_TABLES_MEMCPY", 0) \
    X(bubble_parent_scratch, "RV_BUBBLE_PARENT_SCRATCH", 0) \
    X(level_log, "RV_LEVEL_LOG", 0) \
    X(pb_two_pass, "RV_PB_TWO_PASS", 0) \
    X(no_leaf, "RV_NO_LEAF", 0) \
    X(leaf_prof, "RV_LEAF_PROF", 0) \
    X(no_cascade, "RV_NO_CASCADE", 0) \
    X(cascade_second, "RV_CASCADE_SECOND", 0) \
    X(cascade_danger, "RV_CASCADE_DANGER", 1) \
    X(cascade_second_off, "RV_CASCADE_SECOND_OFF", 0) \
    X(sync_block, "RV_SYNC_BLOCK", 0) \
    X(pb_refresh_tmin, "RV_PB_REFRESH_TMIN", 0) \
    X(cascade_log, "RV_CASCADE_LOG", 0) \
    X(cascade_danger_min, "RV_CASCADE_DANGER_MIN", 0) \
    X(cascade_batch, "RV_CASCADE_BATCH", 8) \
    X(lcp_by_rank, "RV_LCP_BY_RANK", 0) \
    X(no_tiny_sa, "RV_NO_TINY_SA", 0) \
    X(no_short_alphabet, "RV_NO_SHORT_ALPHABET", 0) \
    X(no_fused_lcp, "RV_NO_FUSED_LCP", 0) \
    X(no_diag, "RV_NO_DIAG", 0) \
    X(no_packed_text, "RV_NO_PACKED_TEXT", 0) \
    X(no_heads_fusion, "RV_NO_HEADS_FUSION", 0) \
    X(no_twin_collapse, "RV_NO_TWIN_COLLAPSE", 0) \
    X(no_far_twins, "RV_NO_FAR_TWINS", 0) \
    X(no_lcp_list, "RV_NO_LCP_LIST", 0) \
    X(no_text_jump, "RV_NO_TEXT_JUMP", 0) \
    X(far_table, "RV_FAR_TABLE", 0) \
    X(no_slow_class, "RV_NO_SLOW_CLASS", 0) \
    X(no_dwalk_blocks, "RV_NO_DWALK_BLOCKS", 0) \
    X(no_pub_twins, "RV_NO_PUB_TWINS", 0) \
    X(sa_no_text, "RV_SA_NO_TEXT", 0) \
    X(text_mode, "RV_TEXT_MODE", -1) \
    X(carry_ch, "RV_CARRY_CH", -1) \
    X(rs_bits, "RV_RS_BITS", 8) \
    X(rs_xcd, "RV_RS_XCD", 1) \
    X(rs_cnt16, "RV_RS_CNT16", 1) \
    X(rs_no_digit_bytes, "RV_RS_NO_DIGIT_BYTES", 0) \
    X(diag_table, "RV_DIAG_TABLE", -1) \
    X(no_cascade_chain, "RV_NO_CASCADE_CHAIN", 0) \
    X(casm_rank_count, "RV_CASM_RANK_COUNT", 0) \
    X(casm_big_min, "RV_CASM_BIG_MIN", -1) \
    X(casm_no_big, "RV_CASM_NO_BIG", 0) \
    X(casm_big_root, "RV_CASM_BIG_ROOT", 1 << 22) \
    X(casm_big_total, "RV_CASM_BIG_TOTAL", 1 << 26) \
    X(lock_any, "RV_LOCK_ANY", 0) \
    X(presel_dev_min, "RV_PRESEL_DEV_MIN", 65536) \
    X(scan_v1, "RV_SCAN_V1", 0) \
    X(pick_threads, "RV_PICK_THREADS", 0) \
    X(cascade_prio, "RV_CASCADE_PRIO", 0) \
    X(cas_witness_pass, "RV_CAS_WITNESS_PASS", 0) \
    X(cap_limit, "RV_CAP_LIMIT", 0) \
    X(cap_sites, "RV_CAP_SITES", -1) \
    X(many_chain_multi, "RV_MANY_CHAIN_MULTI", 0) \
    X(pick_chain_cap, "RV_PICK_CHAIN_CAP", 1024) \
    X(decide_max_subs, "RV_DECIDE_MAX_SUBS", 65536) \
    X(pick_mchain_cap, "RV_PICK_MCHAIN_CAP", 512) \
    X(many_kchain_host, "RV_MANY_KCHAIN_HOST", 0) \
    X(kchain_cap, "RV_KCHAIN_CAP", 1024) \
    X(many_kchain_big, "RV_MANY_KCHAIN_BIG", 1) \
    X(kchain_big_min, "RV_KCHAIN_BIG_MIN", 512) \
    X(blocks_host, "RV_BLOCKS_HOST", 0) \
    X(blocks_host_below, "RV_BLOCKS_HOST_BELOW", 4096) \
    X(glocal_host, "RV_GLOCAL_HOST", 0) \
    X(glocal_host_below, "RV_GLOCAL_HOST_BELOW", (int64_t)1 << 31) \
    X(glocal_edge_budget, "RV_GLOCAL_EDGE_BUDGET", 1 << 25) \
    X(rc_host, "RV_RC_HOST", 0) \
    X(rc_host_below, "RV_RC_HOST_BELOW", 0) \
    X(merge_host, "RV_MERGE_HOST", 0) \
    X(merge_host_below, "RV_MERGE_HOST_BELOW", 8192)
struct RvOptions {
#define RV_X_(f, name, def) int64_t f = def;
    RV_OPTION_LIST(RV_X_)
#undef RV_X_
    int64_t *find(const char *name) {
#define RV_X_(f, nm, def) if (strcmp(name, nm) == 0) return &f;
        RV_OPTION_LIST(RV_X_)
#undef RV_X_
        return nullptr;
    }
};
extern int g_rv_launch_trace;      // process-wide (rv_api.hip): rv_set_launch_trace(), not a switch of a handle
// RV_LAUNCH_TRACE=1 (diagnostics): print the source line of every kernel launch and wait for it, so that a GPU memory fault
// (which aborts the process) names the kernel behind it
static inline bool rv_launch_trace_on() { return g_rv_launch_trace != 0; }
#define RV_LAUNCH_CHECK()                                                                      \
    do {                                                                                       \
        RV_HIP(hipGetLastError());                                                             \
        if (rv_launch_trace_on()) {                                                            \
            fprintf(stderr, "launch %s:%d\n", __FILE__, __LINE__);                             \
            fflush(stderr);                                                                    \
            RV_HIP(hipDeviceSynchronize());                                                    \
        }                                                                                      \
    } while (0)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// BWT level arrays: one byte per rank = the character in front of the suffix ('$' for text position 0); all of them are
// ASCII, so bit 7 is free: it says on which side of the first sample separator the suffix starts (reveal.c:73).  The pair
// scan then needs LCP and this byte only (5 B per rank instead of 9) and fetches SA for its few survivors.  The byte travels
// with its rank through split, bubble_sort and the frontier hand-off; readers of the character mask the bit.
#define RV_BWT_SIDE 0x80u
#define RV_BWT_CHAR 0x7fu

#ifdef __HIPCC__
// wave-wide minimum of a u32, broadcast to every lane, without LDS traffic: DPP row operations inside the four 16-lane rows,
// row broadcasts across them, the total read from lane 63.  (Six __shfl_xor steps are six ds_bpermute round trips through the
// LDS pipeline, ~100 cycles each and serialised by their dependence: fine once per tile, ruinous once per 64 ranks.)
__device__ inline u32 rv_wave_min_u32(u32 v) {
    const int inf = -1;      // 0xFFFFFFFF: what a lane without a source lane sees
    int x = (int)v, y;
#define RV_DPP_MIN(ctrl, rmask)                                                        \
    y = __builtin_amdgcn_update_dpp(inf, x, ctrl, rmask, 0xf, false);                  \
    x = (int)(((u32)y < (u32)x) ? (u32)y : (u32)x);
    RV_DPP_MIN(0xB1, 0xf)     // quad_perm [1,0,3,2]
    RV_DPP_MIN(0x4E, 0xf)     // quad_perm [2,3,0,1]
    RV_DPP_MIN(0x141, 0xf)    // row_half_mirror
    RV_DPP_MIN(0x140, 0xf)    // row_mirror: every lane of a row holds the row's minimum
    RV_DPP_MIN(0x142, 0xa)    // row_bcast:15 into rows 1 and 3
    RV_DPP_MIN(0x143, 0xc)    // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's minimum
#undef RV_DPP_MIN
    return (u32)__builtin_amdgcn_readlane(x, 63);
}
#endif

#ifdef __HIPCC__
// One step of a wave-wide inclusive scan by DPP: the value of the lane `shift` lanes below inside a 16-lane row (row_shr), of
// lane 15 of the previous row (row_bcast:15 into rows 1 and 3), of lane 31 (row_bcast:31 into rows 2 and 3).  `take` says
// whether this lane has such a source: Hillis-Steele inside the rows (shifts 1, 2, 4, 8), then the two broadcasts --
// six DPP moves per scanned word where __shfl_up needs six trips through the LDS crossbar.
template <int CTRL, int ROWMASK> __device__ inline u32 rv_dpp_u32(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWMASK, 0xf, false); }
#define RV_WAVE_SCAN_STEPS(STEP)                                                     \
    STEP(0x111, 0xf, (lane & 15) >= 1)                                               \
    STEP(0x112, 0xf, (lane & 15) >= 2)                                               \
    STEP(0x114, 0xf, (lane & 15) >= 4)                                               \
    STEP(0x118, 0xf, (lane & 15) >= 8)                                               \
    STEP(0x142, 0xa, (lane & 31) >= 16)                                              \
    STEP(0x143, 0xc, lane >= 32)
// maximum over the wave (every lane gets it)
__device__ inline u64 rv_wave_max_u64(u64 v) {
#define RV_STEP_(CTRL, RM, TAKE) { const u64 t = ((u64)rv_dpp_u32<CTRL, RM>((u32)(v >> 32)) << 32) | rv_dpp_u32<CTRL, RM>((u32)v); v = t > v ? t : v; }
    RV_WAVE_SCAN_STEPS(RV_STEP_)        // (a lane without a source lane sees 0: the identity)
#undef RV_STEP_
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), 63) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)v, 63);
}
// inclusive maximum over the run of equal `seg` values a lane belongs to (runs are stretches of consecutive lanes): lane i gets the maximum of the
// values of the lanes of its run at or below i.  The same six DPP steps as the scans: a lane takes its source lane's value when that lane belongs
// to the same run (then every lane in between does).  (Written with __shfl_up this was eighteen dependent trips through the LDS crossbar per call.)
__device__ inline u64 rv_wave_seg_max_u64(u32 seg, u64 v) {
    const int lane = threadIdx.x & 63;
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#define RV_STEP_(CTRL, RM, TAKE) { const u32 os = rv_dpp_u32<CTRL, RM>(seg), ol = rv_dpp_u32<CTRL, RM>(lo), oh = rv_dpp_u32<CTRL, RM>(hi); \
                                   const bool up = (TAKE) && os == seg && (oh > hi || (oh == hi && ol > lo)); lo = up ? ol : lo; hi = up ? oh : hi; }
    RV_WAVE_SCAN_STEPS(RV_STEP_)
#undef RV_STEP_
    return ((u64)hi << 32) | lo;
}
__device__ inline u32 rv_wave_seg_max_u32(u32 seg, u32 v) {
    const int lane = threadIdx.x & 63;
#define RV_STEP_(CTRL, RM, TAKE) { const u32 os = rv_dpp_u32<CTRL, RM>(seg), ov = rv_dpp_u32<CTRL, RM>(v); v = ((TAKE) && os == seg && ov > v) ? ov : v; }
    RV_WAVE_SCAN_STEPS(RV_STEP_)
#undef RV_STEP_
    return v;
}
// inclusive prefix sum over the wave
__device__ inline u32 rv_wave_incl_sum_u32(u32 v) {
    const int lane = threadIdx.x & 63;
#define RV_STEP_(CTRL, RM, TAKE) { const u32 t = rv_dpp_u32<CTRL, RM>(v); v += (TAKE) ? t : 0u; }
    RV_WAVE_SCAN_STEPS(RV_STEP_)
#undef RV_STEP_
    return v;
}
// Where ONE wavefront works on a piece of LDS by itself (a sub-index of the leaf kernels, a job of the small build class): what its lanes wrote is
// visible to its other lanes behind this -- a fence and a wave barrier, no workgroup barrier
#define RV_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)
// how many lanes below this one have their bit set in a ballot
__device__ inline u32 rv_lanes_below(u64 mask) { return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u)); }
__device__ inline int rv_iabs(int x) { return x < 0 ? -x : x; }
// sum over the KM lanes of a group: sixteen lanes by four exchanges, the whole wavefront by its scan
template <int KM>
__device__ inline int rv_group_sum(int v) {
    if constexpr (KM == 64) return __builtin_amdgcn_readlane((int)rv_wave_incl_sum_u32((u32)v), 63);
    else { v += __shfl_xor(v, 8, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 1, 16); return v; }
}
// the job whose sequence holds text position p, among the ascending begins of a round's jobs: the last begin at or in front of it
__device__ inline int rv_job_of(const int64_t *__restrict__ beg, int njobs, int64_t p) {
    int lo = 0, hi = njobs;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (beg[mid] <= p) lo = mid + 1; else hi = mid; }
    return lo > 0 ? lo - 1 : 0;
}
#endif

// When a device allocation fails: give back the SA-build scratch of every handle that is not inside a construct() right now
// (it is kept between calls so that a benchmark step does not pay for hipMalloc -- 160 GB at 2.2 x 10^9 positions in the 64-bit
// library, more than the recursion's level arrays find room beside).  true = something was released (rv_api.hip).
bool rv_oom_trim();

// Wait for an event by polling: the wake-up of a sleeping hipEventSynchronize costs tens of microseconds, and the waits on the path
// (a few counters between launches) are 5-15 us long.  The first ~20 us spin (pause instruction: the sibling hyper-thread keeps its
// issue slots), after that the thread yields between polls, and after ~200 us it sleeps in the runtime -- a host application that
// runs many handles does not burn a core per handle on a long wait (bench.py --jobs).
inline hipError_t rv_event_wait(hipEvent_t ev) {
    hipError_t e;
    for (int spins = 0; (e = hipEventQuery(ev)) == hipErrorNotReady; spins++) {
        if (spins < 64) { __builtin_ia32_pause(); continue; }
        if (spins < 640) { std::this_thread::yield(); continue; }
        return hipEventSynchronize(ev);
    }
    return e;
}

// Grow-only device buffer.
struct DBuf {
    void  *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        // (the growth margin saves re-allocations while inputs of similar size follow each other; on the arrays of a large index -- 256 MB and
        //  more -- an eighth was 8.5 bytes per text position of device memory)
        size_t want = bytes + (bytes >= ((size_t)256 << 20) ? bytes / 64 : bytes / 8) + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            if (rv_oom_trim()) e = hipMalloc(&p, want);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); want = bytes + 256; e = hipMalloc(&p, want); }      // without the growth margin
        }
        if (e != hipSuccess) { p = nullptr; rv_set_error("%s:%d hipMalloc(%zu bytes): %s", __FILE__, __LINE__, want, hipGetErrorString(e)); return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

// Pinned host staging buffer (grow-only).
// Streams and pinned host buffers outlive the handle that made them.  `reveal refine` builds an index per bubble -- a few hundred bases,
// 0.9 ms of construct + recursion -- and a handle's three streams and four pinned buffers cost 6 ms to create and destroy
// (hipStreamCreateWithFlags 0.65-2 ms, hipStreamDestroy 0.96 ms, hipHostFree 0.23 ms each: rocprofv3 --hip-trace of 30 such alignments).
// Idle ones wait here for the next handle on the same device; nothing is given back at process exit.
struct RvPools {
    std::mutex mu;
    std::vector<std::pair<int, hipStream_t>> streams;
    struct Pin { int dev; void *p; size_t cap; };
    std::vector<Pin> pinned;
    size_t pinned_bytes = 0;
};
inline RvPools &rv_pools() { static RvPools *p = new RvPools(); return *p; }
inline hipError_t rv_stream_get(hipStream_t *s) {
    int dev = 0; (void)hipGetDevice(&dev);
    {
        RvPools &P = rv_pools();
        std::lock_guard<std::mutex> g(P.mu);
        for (size_t k = P.streams.size(); k-- > 0;)
            if (P.streams[k].first == dev) { *s = P.streams[k].second; P.streams.erase(P.streams.begin() + (ptrdiff_t)k); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
inline void rv_stream_put(hipStream_t s) {      // (the caller has set the stream's device)
    if (!s) return;
    (void)hipStreamSynchronize(s);
    int dev = 0; (void)hipGetDevice(&dev);
    RvPools &P = rv_pools();
    {
        std::lock_guard<std::mutex> g(P.mu);
        if (P.streams.size() < 64) { P.streams.push_back({dev, s}); return; }
    }
    (void)hipStreamDestroy(s);
}
inline hipError_t rv_pinned_get(size_t bytes, void **p, size_t *cap) {
    int dev = 0; (void)hipGetDevice(&dev);
    {
        RvPools &P = rv_pools();
        std::lock_guard<std::mutex> g(P.mu);
        size_t best = (size_t)-1;
        for (size_t k = 0; k < P.pinned.size(); k++)
            if (P.pinned[k].dev == dev && P.pinned[k].cap >= bytes && P.pinned[k].cap <= 4 * bytes + (1u << 20) && (best == (size_t)-1 || P.pinned[k].cap < P.pinned[best].cap)) best = k;
        if (best != (size_t)-1) { *p = P.pinned[best].p; *cap = P.pinned[best].cap; P.pinned_bytes -= *cap; P.pinned.erase(P.pinned.begin() + (ptrdiff_t)best); return hipSuccess; }
    }
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) *cap = bytes;
    return e;
}
inline void rv_pinned_put(void *p, size_t cap) {
    if (!p) return;
    int dev = 0; (void)hipGetDevice(&dev);
    RvPools &P = rv_pools();
    {
        std::lock_guard<std::mutex> g(P.mu);
        if (cap <= ((size_t)64 << 20) && P.pinned_bytes + cap <= ((size_t)512 << 20) && P.pinned.size() < 256) { P.pinned.push_back({dev, p, cap}); P.pinned_bytes += cap; return; }
    }
    (void)hipHostFree(p);
}

struct HBuf {
    void  *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        // (kernels read and write pinned buffers directly -- picks, table staging: nothing may be in flight when one is replaced)
        if (p) { (void)hipDeviceSynchronize(); rv_pinned_put(p, cap); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 2 + 4096;
        RV_HIP(rv_pinned_get(want, &p, &cap));
        return 0;
    }
    void release() { if (p) rv_pinned_put(p, cap); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

// ---- capacity protocols ("Lists filled by atomics").  A list whose capacity is an estimate is filled behind a guard, counted
// beyond it, and the host goes round again with a list of the counted size.  RvCapEvent: one counter per place where the host decides that
// (rv_capacity_events, include/reveal_amd.h: host integers, nothing on the device).  RvCapSite: the estimates that no small input overflows;
// RV_CAP_LIMIT = an upper limit on what the FIRST attempt of the sites named by the bit mask RV_CAP_SITES passes to its kernels (test hook;
// the buffers are allocated as without it -- a list kept in regions is laid out with the limited stride inside its buffer --, a retry sizes
// from the count as ever).
enum RvCapEvent { RV_CE_PAIR_OVF = 0, RV_CE_PAIR_OUT, RV_CE_PAIR_PICK_OVF, RV_CE_PAIR_SECOND_COPY, RV_CE_MULTI_REC, RV_CE_MULTI_MEM, RV_CE_MULTI_CAND,
                  RV_CE_MEMS_REC, RV_CE_MEMS_MEM, RV_CE_MEMS_LONG, RV_CE_COUNT };
enum RvCapSite { RV_CS_MULTI_CAND = 1, RV_CS_CAS_WIT = 2, RV_CS_CAS_TABLES = 4, RV_CS_CASM_MATCHES = 8, RV_CS_CASM_WIT = 16, RV_CS_CASM_TABLES = 32,
                 RV_CS_MEMS_REC = 64, RV_CS_MEMS_MEM = 128, RV_CS_MEMS_LONG = 256 };
// Scratch slots used by the primitives (one set per index handle, one stream).
struct Workspace {
    hipStream_t stream = nullptr;
    RvOptions opt;         // the owning handle's switches (rv_set_option)
    int64_t cap_events[RV_CE_COUNT] = {0};
    // what the last pair scan / multi picker passed to its kernels as the overflow buffer's / candidate list's capacity: the early split's
    // decide kernels test the same header words against the same values (rv_align.hip early_split)
    u32 pair_ovf_cap = 0, multi_cand_cap = 0;
    template <class T> T cap_first(int site, T cap, T least = 1) const {
        if (opt.cap_limit <= 0 || !(opt.cap_sites & (int64_t)site)) return cap;
        const T lim = (T)std::max<int64_t>(opt.cap_limit, (int64_t)least);
        return cap < lim ? cap : lim;
    }
    DBuf scan_tmp[4];      // block sums of the multi-level scan
    DBuf rs_hist;          // radix sort: per-block digit histograms
    DBuf rs_digits;        // radix sort: the next pass' digit of every key, a byte each
    DBuf misc[20];
    DBuf blk[15];          // getblocks (rv_blocks.hip): records, ids, keys, sums and the block arrays
    DBuf glc[3];           // the glocal chain (rv_glocal.hip): the arena of a call, a tile's edges, the tables that stay for every pass
    DBuf mrg[10];          // merge_consecutive (rv_merge.hip): the uploaded and the gathered columns, keys, permutations, sums, the merged rows
    DBuf sa[32];           // SA-build scratch, kept between construct() calls
    HBuf hpin;             // pinned landing zone of rv_read_back
    hipEvent_t ev_rb = nullptr;
    // kernel-class timing of the handle that owns this workspace (RvProf, rv_index.h), for code that only sees the workspace
    void *prof_ctx = nullptr;
    int (*prof_begin_fn)(void *, hipStream_t, int, double) = nullptr;
    void (*prof_end_fn)(void *, hipStream_t, int) = nullptr;
    int prof_begin(int k, double bytes) { return prof_begin_fn ? prof_begin_fn(prof_ctx, stream, k, bytes) : -1; }
    void prof_end(int id) { if (prof_end_fn && id >= 0) prof_end_fn(prof_ctx, stream, id); }
    bool sa_in_use = false; // inside rv_build_sa / rv_build_lcp: the scratch below must stay
    size_t trim_sa() {      // releases the SA-build scratch; -> bytes given back
        size_t got = 0;
        for (auto &b : sa) { got += b.cap; b.release(); }
        return got;
    }
    void release() {
        hpin.release();
        if (ev_rb) { (void)hipEventDestroy(ev_rb); ev_rb = nullptr; }
        for (auto &b : scan_tmp) b.release();
        rs_hist.release(); rs_digits.release();
        for (auto &b : misc) b.release();
        for (auto &b : blk) b.release();
        for (auto &b : glc) b.release();
        for (auto &b : mrg) b.release();
        for (auto &b : sa) b.release();
    }
};

std::mutex &rv_trim_mutex();      // rv_api.hip: guards the list of live handles and every change of sa_in_use
struct SaScratchInUse {
    Workspace &w; bool was;
    SaScratchInUse(Workspace &x) : w(x) { std::lock_guard<std::mutex> g(rv_trim_mutex()); was = w.sa_in_use; w.sa_in_use = true; }
    ~SaScratchInUse() { std::lock_guard<std::mutex> g(rv_trim_mutex()); w.sa_in_use = was; }
};

// ---- primitives (rv_prims.hip) ---------------------------------------------
// out[i] = sum_{j<i} in[j]  (in may alias out); n up to 2^40.
int rv_exclusive_sum_u32(Workspace &ws, const u32 *in, u32 *out, int64_t n);
int rv_exclusive_sum_u64(Workspace &ws, const u64 *in, u64 *out, int64_t n);
// out[i] = max_{j<=i} in[j]
int rv_inclusive_max_u32(Workspace &ws, const u32 *in, u32 *out, int64_t n);
int rv_inclusive_max_u64(Workspace &ws, const u64 *in, u64 *out, int64_t n);

// Stable LSD radix sort of (64-bit key, 32/64-bit value) pairs on key bits
// [bit_lo, bit_hi).  Ping-pongs between (k0,v0) and (k1,v1); *result_in_1
// tells where the sorted data ended up.
// radix passes rv_radix_sort_pairs makes over `nbits` key bits (8- or 10-bit digits: ws.opt.rs_bits)
int rv_radix_passes(const Workspace &ws, int nbits);
template <class V>
int rv_radix_sort_pairs(Workspace &ws, u64 *k0, V *v0, u64 *k1, V *v1, int64_t n,
                        int bit_lo, int bit_hi, int *result_in_1, bool first_digits = false);
// Where a caller that makes the keys itself may leave the first pass' digit of every key -- (uint8_t)(key >> bit_lo), a byte per key in
// the keys' order -- so that the sort's first histogram reads a byte per key instead of the key: the pointer (n + 64 bytes), or null when
// this sort would not use them.  Nothing else may sort on this workspace in between; the sort is then called with first_digits = true.
uint8_t *rv_radix_first_digits(Workspace &ws, int64_t n, int bit_lo, int bit_hi);

// A few bytes the host needs before it can go on (counts that size the next launch): device -> pinned memory -> dst, waiting on
// an event by polling.  A pageable destination is staged by the runtime and hipStreamSynchronize sleeps: ~35 us per read
// against ~12 us this way, five reads per construct().
int rv_read_back(Workspace &ws, void *dst, const void *dsrc, size_t bytes);
// two such pieces behind one wait
int rv_read_back2(Workspace &ws, void *dst_a, const void *dsrc_a, size_t bytes_a, void *dst_b, const void *dsrc_b, size_t bytes_b);

// copy of a small table from pinned host memory by a kernel (bytes rounded up to 16: both buffers must have that room)
int rv_h2d_copy(Workspace &ws, const void *pinned_src, void *dst, size_t bytes);

// ---- construct (rv_construct.hip) ------------------------------------------
// which side of each of rv_build_sa's host decisions a build took (read-only census: rv_sa_paths hands the fields out in this order)
struct RvSaPaths {
    int tiny;                                   // the counting build ran (k_sa_tiny_rank / k_sa_tiny_emit); everything below but the fused pair stays 0
    int short_alphabet, ends_with_sep;          // "past the end" spells the separator when both are set
    int g, K, bits;                             // key layout: digits per field, symbols and bits of the first key
    int fused_asked, fused_final;               // LCP / BWT from the build itself: requested / kept to the end
    int hint_ns, nd_bits;                       // samples the diagonal hint knows / hint bits in the key
    int collapse;                               // twins of the second sample leave before the sort
    int diag_table_tried, diag_table_kept;      // piecewise diagonals
    int heads_kernel;                           // 0 k_heads + k_publish0, 1 k_heads_publish, 2 k_heads_publish_tc
    int text_round, text_mode, packed_text;     // the text round ran, the work division that ran (0 when it did not), the 2-bit text was used
    int text_big;                               // a group above MEDIUM_GROUP went through the radix path in the text round
    int far_ran, nd_table;                      // k_far_twins ran, with the table of k_far_nd
    int doubling_rounds, slow_class, text_jump; // rounds ordered by ranks (k_round_small), classes made, h jumped to TEXT_LIM
    int lcp_list_overflow;                      // k_lcp_list met a common prefix it gave up on
    int64_t defer_max, defer_cap;               // k_round_text3: largest per-region count of its work list, and reg_cap
    int lcp_by_rank;                            // rv_build_lcp ran rank by rank (k_lcp) after the build (set by rv_construct)
};
#define RV_SA_PATHS_FIELDS 27
struct RvSaStats {
    int    sigma, bits, k0;     // alphabet size, bits per symbol, symbols in the first key
    int    rounds;              // doubling rounds after the initial sort
    int64_t sorted_elems;       // sum of elements pushed through the radix sort
    int    radix_passes;
    int    diag_table;          // two samples: the hint and the twins' leaving follow piecewise diagonals from seeds (k_diag_bits_tab)
    int64_t far_pairs;          // tied pairs of partners ordered from the diagonal's marks (k_far_twins)
    int64_t lcp_list;           // ranks whose LCP / BWT came from the text after the doubling rounds (k_lcp_list)
    RvSaPaths paths;
};
// SA of T[0..n) (device pointers).  T must be readable up to n+15 (zero padded).
// LCP / BWT / d_maxlcp given: the build also leaves LCP (interface.c:97-114), the BWT bytes (side_sep as for rv_build_lcp) and
// the largest LCP whenever the first key and the text round finish the order (*fused_done = true); otherwise rv_build_lcp is due
int rv_build_sa(Workspace &ws, const uint8_t *T, int64_t n, sa_t *SA, RvSaStats *st,
                lcp_t *LCP = nullptr, uint8_t *BWT = nullptr, sa_t side_sep = 0, u32 *d_maxlcp = nullptr, bool *fused_done = nullptr,
                const int64_t *seps = nullptr, int nseps = 0);      // seps: every sample separator (nsep), for the diagonal hint
int rv_build_inverse(Workspace &ws, const sa_t *SA, sa_t *SAi, int64_t n);
// the same for an SA that came from a file: fails unless it is a permutation of 0..n-1
int rv_build_inverse_checked(Workspace &ws, const sa_t *SA, sa_t *SAi, int64_t n);
// LCP with the reference's stop characters (interface.c:97-114); also returns max LCP.
// by_rank: every rank from scratch (one thread per rank); otherwise text order with Kasai's carry (PHI scatter, no inverse needed)
// side_sep: text position of the first sample separator, nsep[0] (bit RV_BWT_SIDE of a BWT byte = the suffix starts behind
// it), or the largest sa_t for a single sample (the bit stays clear)
int rv_build_lcp(Workspace &ws, const uint8_t *T, const sa_t *SA, bool by_rank, lcp_t *LCP, int64_t n, u32 *d_maxlcp, uint8_t *BWT, sa_t side_sep);
// BWT only (when LCP came from a file)
int rv_build_bwt(Workspace &ws, const uint8_t *T, const sa_t *SA, int64_t n, uint8_t *BWT, sa_t side_sep);
