// rv_revcomp.h -- the reverse complement of construct(rc=1) (interface.c:136-158, :168-175): the rule, stated once for the host loop and
// the kernel, and the launcher of the kernel that applies it to the text in device memory (rv_revcomp.hip).
#pragma once
#include "rv_common.h"

// The complement of one byte, for all 256 values: letters through the reference's table (either case), 96 -> 64, everything else -- digits,
// '$', punctuation, bytes of 128 and above -- unchanged.  Its own inverse except on U, u (-> A, a) and 96, as in the reference.
__host__ __device__ inline char rv_comp_of(char ch) {
    constexpr char up[27] = "TVGHEFCDIJMLKNOPQYSAABWXRZ";
    const unsigned char c = (unsigned char)ch;
    if (c >= 'A' && c <= 'Z') return up[c - 'A'];
    if (c >= 'a' && c <= 'z') return (char)(up[c - 'a'] + 32);
    if (c == 96) return 64;
    return ch;
}
// T[0, n) reversed and complemented in place on the host
inline void rv_revcomp_host(char *T, int64_t n) {
    for (int64_t i = 0; i < n >> 1; ++i) {
        const char c0 = rv_comp_of(T[i]), c1 = rv_comp_of(T[n - 1 - i]);
        T[i] = c1; T[n - 1 - i] = c0;
    }
    if (n & 1) T[n >> 1] = rv_comp_of(T[n >> 1]);
}

// k_text_revcomp's shape: a thread moves one pair of RV_RC_PIECE-byte pieces, a workgroup RV_RC_THREADS pairs
#define RV_RC_PIECE 16
#define RV_RC_THREADS 256

// d_text[lo, lo + len) reversed and complemented in place, on the workspace's stream.  No byte outside the range is read or written.
// d_seen (optional, a device word that does not hold `mark`): set to `mark` when the range held U, u or 96 before the call -- the bytes on
// which two turns do not bring the text back.
int rv_text_revcomp(Workspace &ws, uint8_t *d_text, int64_t lo, int64_t len, u32 *d_seen = nullptr, u32 mark = 1);
