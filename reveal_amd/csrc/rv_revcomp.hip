// rv_revcomp.hip -- construct(rc=1)'s reverse complement of T[nsep[0], n) (interface.c:168-175) on the text in device memory, in place.
//
// The range [lo, hi) is cut into a head of `head` < 16 bytes that brings lo up to a 16-byte boundary, the mirror tail of as many bytes,
// `npairs` pairs of 16-byte pieces -- piece j at lo + head + 16 j and its mirror ending at hi - head - 16 j --, and the fewer than 32
// bytes left in the middle.  Thread j loads both pieces of pair j, reverses and complements them in registers and stores each where the
// other came from: a front piece is aligned, a back piece is wherever (hi - head) mod 16 puts it and is moved by a 16-byte access all the
// same (the hardware takes unaligned global addresses).  The one thread behind the last pair swaps head and tail and turns the middle
// byte by byte.  No two threads touch the same byte: no barrier and no atomic for the data, nothing outside the range read or written.
// The complement is rv_comp_of (rv_revcomp.h) through a 256-byte table in LDS that the workgroup's 256 threads fill, one entry each: 64
// words, every one in a bank of its own, so a look-up never conflicts.
// rv_comp_of is its own inverse on every byte value but U, u and 96 (U -> A -> T, 96 -> 64 -> 64): where `seen` is given, a thread that meets one
// of the three in what it READS stores `mark` there (every writer the same value, one the word did not hold before) -- the handle then knows whether
// turning the range a second time brings the first text back (rv_construct).  The test is two packed zero-byte tests a word.
#include "rv_revcomp.h"

namespace {

typedef u32 rc_u4 __attribute__((ext_vector_type(4)));
typedef rc_u4 rc_u4_any __attribute__((aligned(1)));      // a 16-byte piece at any address

// the 16 bytes of v in reverse order, complemented
__device__ __forceinline__ rc_u4 rc_turn(const rc_u4 v, const uint8_t *tab) {
    rc_u4 o;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const u32 s = v[3 - d];
        o[d] = (u32)tab[s >> 24] | ((u32)tab[(s >> 16) & 255u] << 8) | ((u32)tab[(s >> 8) & 255u] << 16) | ((u32)tab[s & 255u] << 24);
    }
    return o;
}

// nonzero iff one of the four bytes of v is U, u or 96
__device__ __forceinline__ u32 rc_odd_word(u32 v) {
    const u32 x = (v | 0x20202020u) ^ 0x75757575u, y = v ^ 0x60606060u;      // a zero byte in x: U or u; in y: 96
    return (((x - 0x01010101u) & ~x) | ((y - 0x01010101u) & ~y)) & 0x80808080u;
}
__device__ __forceinline__ bool rc_odd_byte(uint8_t c) { return c == (uint8_t)'U' || c == (uint8_t)'u' || c == 96; }

__global__ __launch_bounds__(RV_RC_THREADS) void k_text_revcomp(uint8_t *__restrict__ T, int64_t lo, int64_t hi, int64_t head, int64_t npairs, u32 *__restrict__ seen, u32 mark) {
    __shared__ uint8_t tab[256];
    static_assert(RV_RC_THREADS == 256, "one table entry per thread");
    tab[threadIdx.x] = (uint8_t)rv_comp_of((char)threadIdx.x);
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * RV_RC_THREADS + threadIdx.x;
    if (t < npairs) {
        rc_u4 *f = (rc_u4 *)__builtin_assume_aligned(T + lo + head + RV_RC_PIECE * t, 16);
        rc_u4_any *b = (rc_u4_any *)(T + hi - head - RV_RC_PIECE * t - RV_RC_PIECE);
        const rc_u4 vf = *f, vb = *b;
        *f = rc_turn(vb, tab);
        *b = rc_turn(vf, tab);
        if (seen) {
            u32 odd = 0;
#pragma unroll
            for (int d = 0; d < 4; d++) odd |= rc_odd_word(vf[d]) | rc_odd_word(vb[d]);
            if (odd) *seen = mark;
        }
    } else if (t == npairs) {
        bool odd = false;
        for (int64_t i = 0; i < head; i++) {
            const uint8_t r0 = T[lo + i], r1 = T[hi - 1 - i];
            odd = odd || rc_odd_byte(r0) || rc_odd_byte(r1);
            T[lo + i] = tab[r1]; T[hi - 1 - i] = tab[r0];
        }
        int64_t a = lo + head + RV_RC_PIECE * npairs, b = hi - head - RV_RC_PIECE * npairs - 1;
        for (; a < b; a++, b--) {
            const uint8_t r0 = T[a], r1 = T[b];
            odd = odd || rc_odd_byte(r0) || rc_odd_byte(r1);
            T[a] = tab[r1]; T[b] = tab[r0];
        }
        if (a == b) { odd = odd || rc_odd_byte(T[a]); T[a] = tab[T[a]]; }
        if (seen && odd) *seen = mark;
    }
}

}  // namespace

int rv_text_revcomp(Workspace &ws, uint8_t *d_text, int64_t lo, int64_t len, u32 *d_seen, u32 mark) {
    if (!d_text || lo < 0 || len < 0) { rv_set_error("rv_text_revcomp: bad range"); return -1; }
    if (len == 0) return 0;
    int64_t head = (int64_t)((16 - ((uintptr_t)(d_text + lo) & 15)) & 15);
    if (2 * head > len) head = 0;      // (too short to peel: the whole range is the middle)
    const int64_t npairs = (len - 2 * head) / (2 * RV_RC_PIECE);
    const unsigned grid = (unsigned)ceil_div(npairs + 1, RV_RC_THREADS);
    hipLaunchKernelGGL(k_text_revcomp, dim3(grid), dim3(RV_RC_THREADS), 0, ws.stream, d_text, lo, lo + len, head, npairs, d_seen, mark);
    RV_LAUNCH_CHECK();
    return 0;
}
