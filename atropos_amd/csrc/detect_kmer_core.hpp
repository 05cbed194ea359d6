// detect_kmer_core.hpp -- de-novo adapter discovery (the reference's HeuristicDetector._get_contaminants,
// commands/detect/__init__.py:568-619): the layouts, keys and per-position decisions that the kernels
// (detect_kmer_kernels.hip) and the CPU test emulation (tests/emu/emu_kmer.cpp, -DATR_HOST_EMU) share.
//
// The reads are the representatives of the distinct pass (detect_kernels.hip), one per distinct kept sequence.
// Every kept base of every representative has a SLOT; the slots of one read are consecutive, so the slot of
// (read, o + a) is the slot of (read, o) plus a.  A slot has room r = kept - o: the k-mer that starts there exists
// for k <= r.  K-mers compare as bytes.  No k-mer is ever written down or hashed: a k-mer is known by its CLASS, the
// dense rank of its text among the k-mers counted at that length, and a class is made from shorter ones:
//   pair key   (class of the a-mer at p) << 32 | (class of the b-mer at p + a)   -> the (a + b)-mers   (1-mers: the byte)
//   level key  (class of the k-mer at p) << 8 | (byte at p + k)                  -> the (k + 1)-mers
// Equal keys <=> equal texts, by induction; the caller sorts the keys and kmer ranks turn the sorted runs into
// classes.  A slot without room for the longer k-mer gets KMER_NO_KEY, which sorts last and gets no class.
#ifndef ATR_DETECT_KMER_CORE_HPP
#define ATR_DETECT_KMER_CORE_HPP

#include <stddef.h>
#include <stdint.h>

#ifdef ATR_HOST_EMU
#define KMER_HD static inline
#else
#define KMER_HD __host__ __device__ __forceinline__
#endif

namespace atr {

constexpr int KMER_MIN_K = 4, KMER_MAX_K = 32;            // kmer_size (the filter's bounds)
constexpr int KMER_MAX_READ = 320;                        // the filter's bound: no k-mer and no pattern is longer
constexpr long long KMER_MAX_SLOTS = (1ll << 31) - 1;     // classes and slots are int32
constexpr int KMER_MAX_CANDIDATES = 1 << 20;              // rows of the candidate table
constexpr int KMER_MAX_PATTERNS = 64;                     // patterns of one support call (64 x 320 bytes of LDS)
constexpr long long KMER_NO_KEY = 0x7fffffffffffffffll;
constexpr int KMER_NO_CLASS = -1;

// a representative: its first slot, where its text starts in the chunk, what it keeps, its record
struct KmerRep {
    long long start;
    uint32_t off;
    int32_t kept;
    long long rec;
};

// a row of the candidate table
enum { KMER_C_LEVEL = 0, KMER_C_COUNT = 1, KMER_C_REP = 2, KMER_C_OFFSET = 3, KMER_C_QUIRK = 4, KMER_C_WORDS = 5 };
// the words of the state block (int64): rows appended so far (may pass the capacity: nothing is written beyond it),
// the survivors the last `next` call left, then the number of over-represented classes of level k at KMER_S_OVER + k
enum { KMER_S_CANDIDATES = 0, KMER_S_SURVIVORS = 1, KMER_S_OVER = 8, KMER_S_WORDS = KMER_S_OVER + KMER_MAX_READ + 2 };

KMER_HD long long kmer_pair_key(int32_t a, int32_t b) { return ((long long)a << 32) | (long long)(uint32_t)b; }
KMER_HD long long kmer_level_key(int32_t cls, uint8_t next) { return ((long long)cls << 8) | (long long)next; }

// count_k(x) > min_count(k), the reference's test
KMER_HD bool kmer_over(long long count, long long min_count) { return count > min_count; }

// the word of the longest-match rule: smallest first index, then lowest record
KMER_HD unsigned long long kmer_support_word(int first, long long rec) {
    return ((unsigned long long)(uint32_t)first << 32) | (unsigned long long)(uint32_t)rec;
}

// the pattern at text + at?
KMER_HD bool kmer_same(const uint8_t *text, const uint8_t *pat, int len) {
    for (int j = 0; j < len; ++j)
        if (text[j] != pat[j]) return false;
    return true;
}

// ---- argument checks, the same on the device and in the twin: 0, -1 (invalid) or -2 (outside the envelope)
KMER_HD int kmer_check_slots(long long nrep, long long total, int kmer_size) {
    if (nrep < 0 || total < 0) return -1;
    if (kmer_size < KMER_MIN_K || kmer_size > KMER_MAX_K || total > KMER_MAX_SLOTS) return -2;
    return 0;
}
KMER_HD int kmer_check_len(long long n, int len) {
    if (n < 0 || len < 1) return -1;
    if (n > KMER_MAX_SLOTS || len > KMER_MAX_READ) return -2;
    return 0;
}
KMER_HD int kmer_check_level(long long n, int k, long long capacity) {
    if (n < 0 || k < 1 || capacity < 0) return -1;
    if (n > KMER_MAX_SLOTS || k > KMER_MAX_READ || capacity > KMER_MAX_CANDIDATES) return -2;
    return 0;
}
KMER_HD int kmer_check_support(long long nrep, int npat) {
    if (nrep < 0 || npat < 0) return -1;
    if (npat > KMER_MAX_PATTERNS || nrep > KMER_MAX_SLOTS) return -2;
    return 0;
}

}  // namespace atr
#endif
