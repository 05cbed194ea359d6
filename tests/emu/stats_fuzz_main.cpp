// TEST INFRASTRUCTURE: stand-alone driver of the CPU twin of the read-statistics entry points (emu_stats.cpp,
// stats_core.hpp with -DATR_HOST_EMU), built with -fsanitize=address,undefined by tests/test_stats_kernels_host.py and
// run as a subprocess: nothing sanitized is loaded into Python.
//
//   stats_fuzz <rounds> <seed>
// Every round lays 0 .. 200 records of 0 .. max_len arbitrary bytes (a fifth of them without a quality line) back to
// back in a heap block of exactly their size, the last line ending on the block's last byte, draws kept intervals
// (``end < begin`` included), masks (bounds outside the line included), destinations, ``longest`` in 0 .. max_len and
// an ``index_base`` up to 2^40, and collects them into heap blocks of exactly atr_read_stats_bytes(max_len): a load
// or a store outside either is a sanitizer report, and so is an overflow the language leaves undefined.  Two blocks
// are merged into a third of a larger capacity.  What is checked needs no model: the sums of the histograms against
// the header words, rows that shrink with the position, the merged header.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "atropos_hip.h"

extern "C" {
int64_t emu_read_stats_bytes(int);
int emu_read_stats_clear(void *, int, void *);
int emu_read_stats_batch(void *, int, int, int, const uint8_t *, const atr_fastq_record *, const int32_t *, const int32_t *,
                         const int32_t *, const int32_t *, const uint8_t *, int, int64_t, int64_t, void *);
int emu_read_stats_merge(void *, int, const void *, int, int64_t, void *);
}

typedef unsigned long long u64;
static uint64_t state;
static uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
static int upto(int n) { return (int)(rnd() % (uint32_t)(n + 1)); }           // 0 .. n
#define FAIL(...) do { fprintf(stderr, "round %d: ", round); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 3; } while (0)

static u64 sum(const u64 *p, long long n) {
    u64 s = 0;
    for (long long i = 0; i < n; ++i) s += p[i];
    return s;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: stats_fuzz <rounds> <seed>\n"); return 2; }
    const int rounds = atoi(argv[1]);
    state = (uint64_t)atoll(argv[2]) * 2654435761ull + 1;
    u64 total_reads = 0, total_skipped = 0;
    for (int round = 0; round < rounds; ++round) {
        const int L = 1 + upto(round % 5 == 0 ? 1100 : 150), longest = round % 7 == 0 ? L : upto(L);
        const int n = upto(200), qb = upto(255), which = upto(3);
        const bool intervals = round % 3 != 0, masks = intervals && round % 2 == 0, dests = round % 4 != 1;
        std::vector<atr_fastq_record> recs((size_t)n);
        std::vector<uint8_t> text;
        for (int r = 0; r < n; ++r) {
            const uint32_t len = (uint32_t)upto(L);
            atr_fastq_record rec;
            memset(&rec, 0, sizeof rec);
            rec.seq_off = (uint32_t)text.size();
            rec.seq_len = len;
            for (uint32_t i = 0; i < len; ++i) text.push_back((uint8_t)(rnd() % 3 ? "ACGTN"[rnd() % 5] : rnd() & 255));
            if (rnd() % 5) {
                rec.qual_off = (uint32_t)text.size();
                rec.qual_len = len;
                for (uint32_t i = 0; i < len; ++i) text.push_back((uint8_t)(rnd() & 255));
            }
            recs[(size_t)r] = rec;
        }
        uint8_t *bytes = (uint8_t *)malloc(text.size() ? text.size() : 1);      // exactly the lines: nothing behind them
        if (!text.empty()) memcpy(bytes, text.data(), text.size());
        std::vector<int32_t> begin((size_t)n), end((size_t)n), ub((size_t)n), ue((size_t)n);
        std::vector<uint8_t> dest((size_t)n);
        long long selected = 0;
        for (int r = 0; r < n; ++r) {
            const int len = (int)recs[(size_t)r].seq_len;
            begin[(size_t)r] = upto(len);
            end[(size_t)r] = rnd() % 4 ? begin[(size_t)r] + upto(len - begin[(size_t)r]) : upto(len);
            ub[(size_t)r] = upto(len + 4) - 2;
            ue[(size_t)r] = rnd() % 3 ? len + upto(3) : upto(len + 4) - 2;
            dest[(size_t)r] = (uint8_t)upto(3);
            selected += !dests || dest[(size_t)r] == which;
        }
        const int64_t size = emu_read_stats_bytes(L);
        if (size <= 0) FAIL("atr_read_stats_bytes(%d) = %lld", L, (long long)size);
        const long long words = size / 8;
        u64 *one = (u64 *)malloc((size_t)size), *two = (u64 *)malloc((size_t)size);
        memset(one, 0xEE, (size_t)size);
        memset(two, 0xEE, (size_t)size);
        if (emu_read_stats_clear(one, L, nullptr) || emu_read_stats_clear(two, L, nullptr)) FAIL("clear");
        const int64_t base = round % 2 ? (int64_t)((1ull << 32) - 50) : (int64_t)(rnd() % 3) << 39;
        const int rc = emu_read_stats_batch(one, L, longest, qb, bytes, recs.data(), intervals ? begin.data() : nullptr,
                                            intervals ? end.data() : nullptr, masks ? ub.data() : nullptr, masks ? ue.data() : nullptr,
                                            dests ? dest.data() : nullptr, which, n, base, nullptr);
        if (rc) FAIL("batch: %d", rc);
        const long long gc = 8 + L + 1, mq = gc + 101, seq = mq + 256, qual = seq + 256ll * L, first = qual + 256ll * L;
        if (first + L + 1 + 101 + 256 != words) FAIL("layout: %lld words", words);
        if ((long long)(one[0] + one[3]) != selected) FAIL("count %llu + skipped %llu != %lld", one[0], one[3], selected);
        if (sum(one + 8, L + 1) != one[0]) FAIL("length histogram");
        if (sum(one + 8 + longest + 1, L - longest)) FAIL("a length bin beyond longest");
        if (sum(one + gc, 101) != one[0] - one[8]) FAIL("gc histogram");
        if (sum(one + mq, 256) != one[2] || one[2] > one[0] - one[8]) FAIL("mean-quality histogram");
        if ((int)one[1] > longest) FAIL("longest");
        u64 above = one[0] - one[8], above_q = one[2];
        for (int p = 0; p < L; ++p) {
            const u64 s = sum(one + seq + 256ll * p, 256), q = sum(one + qual + 256ll * p, 256);
            if (s > above || q > above_q || q > s || (p >= (int)one[1] && (s || q))) FAIL("row %d", p);
            above = s;
            above_q = q;
        }
        // the same records again behind themselves, merged into a block of a larger capacity
        if (emu_read_stats_batch(two, L, longest, qb, bytes, recs.data(), intervals ? begin.data() : nullptr,
                                 intervals ? end.data() : nullptr, masks ? ub.data() : nullptr, masks ? ue.data() : nullptr,
                                 dests ? dest.data() : nullptr, which, n, 0, nullptr)) FAIL("batch 2");
        const int big = L + upto(40);
        const int64_t big_size = emu_read_stats_bytes(big);
        u64 *dst = (u64 *)malloc((size_t)big_size);
        if (emu_read_stats_clear(dst, big, nullptr) || emu_read_stats_merge(dst, big, one, L, 0, nullptr) ||
            emu_read_stats_merge(dst, big, two, L, base + n, nullptr)) FAIL("merge");
        if (dst[0] != 2 * one[0] || dst[1] != one[1] || dst[2] != 2 * one[2] || dst[3] != 2 * one[3]) FAIL("merged header");
        if (sum(dst, big_size / 8 - (big + 1 + 101 + 256)) - dst[1] != 2 * (sum(one, first) - one[1])) FAIL("merged sums");
        const u64 *f1 = one + first, *fd = dst + 8 + big + 1 + 101 + 256 + 512ll * big;
        for (int i = 0; i <= L; ++i)
            if (fd[i] != f1[i]) FAIL("merged first read of length %d", i);     // the earlier block's read stays the first
        total_reads += one[0];
        total_skipped += one[3];
        free(dst); free(one); free(two); free(bytes);
    }
    printf("ok: %d rounds, %llu reads collected, %llu skipped\n", rounds, total_reads, total_skipped);
    return 0;
}
