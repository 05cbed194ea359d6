// TEST INFRASTRUCTURE: stand-alone driver of the CPU twin of the unaligned BAM entry points (emu_bam.cpp, bam_core.hpp
// with -DATR_HOST_EMU), built with -fsanitize=address,undefined by tests/test_bam_host.py and run as a subprocess:
// nothing sanitized is loaded into Python.
//
//   bam_fuzz <runs> <seed>
// A run is a valid record stream with one random byte or one random field overwritten, a valid stream cut anywhere, or
// a pure byte soup, in a heap block of EXACTLY its size: the walk may read no byte behind it, so a load outside is a
// sanitizer report.  Every run must end in the record table, `consumed` and error word of the serial walk written
// here, at several tile sizes; the records are then decoded, single and paired, into a block of exactly the size
// the first call asked for, and the single-end text is compared with a decoder written here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <string>
#include <vector>

#include "atropos_hip.h"

extern "C" {
int64_t emu_bam_walk_workspace(int64_t, int64_t);
int emu_bam_walk(const uint8_t *, int64_t, int64_t, int32_t, int, int64_t, int64_t, uint32_t *, int64_t, int64_t *, void *, int64_t,
                 void *);
size_t emu_bam_to_fastq_work_bytes(int64_t);
int emu_bam_to_fastq(const uint8_t *, int64_t, const uint32_t *, int64_t, int, int64_t *, int64_t *, void *, uint8_t *, void *);
}

static uint64_t state;
static uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

static void put32(std::string &s, int32_t v) {
    for (int k = 0; k < 4; ++k) s.push_back((char)((uint32_t)v >> (8 * k)));
}
static long long get32(const uint8_t *p) { return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24); }

static std::string make_record(int n_ref) {
    const int l_name = 1 + rnd() % 12, n_cigar = rnd() % 3, l_seq = rnd() % 5 ? rnd() % 90 : rnd() % 700, tags = rnd() % 3 ? 0 : rnd() % 40;
    std::string body;
    put32(body, n_ref ? (int)(rnd() % (n_ref + 1)) - 1 : -1);
    put32(body, -1);
    body.push_back((char)l_name);
    body.push_back(0);
    body.push_back(0x48); body.push_back(0x12);
    body.push_back((char)n_cigar); body.push_back(0);
    const int flag = rnd() % 2 ? 77 : 141;
    body.push_back((char)flag); body.push_back(0);
    put32(body, l_seq);
    put32(body, -1);
    put32(body, -1);
    put32(body, 0);
    for (int k = 0; k + 1 < l_name; ++k) body.push_back((char)('a' + rnd() % 26));
    body.push_back(0);
    for (int k = 0; k < 4 * n_cigar + (l_seq + 1) / 2; ++k) body.push_back((char)rnd());
    for (int k = 0; k < l_seq; ++k) body.push_back((char)(rnd() % 100 ? rnd() % 94 : rnd()));
    for (int k = 0; k < tags; ++k) body.push_back((char)rnd());
    std::string rec;
    put32(rec, (int32_t)body.size());
    return rec + body;
}

struct Walk {
    std::vector<uint32_t> starts;
    long long consumed, error;
};

// the serial walk, field by field
static Walk serial(const uint8_t *b, long long n, long long entry, int final, long long cap) {
    Walk w;
    long long at = entry;
    int kind = 0;
    for (;;) {
        if (n - at < 4) break;
        const long long bs = get32(b + at);
        if (bs < 32) { kind = ATR_BAM_ERR_SMALL; break; }
        if (bs > cap) { kind = ATR_BAM_ERR_BIG; break; }
        if (at + 4 + bs > n) break;
        const long long l_name = b[at + 12], n_cigar = b[at + 16] | b[at + 17] << 8, l_seq = get32(b + at + 20);
        if (l_seq < 0) { kind = ATR_BAM_ERR_LSEQ; break; }
        if (bs < 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq) { kind = ATR_BAM_ERR_SMALL; break; }
        w.starts.push_back((uint32_t)at);
        at += 4 + bs;
    }
    if (!kind && final && at != n) kind = ATR_BAM_ERR_TRUNCATED;
    w.consumed = at;
    w.error = kind ? at * 8 + kind : LLONG_MAX;
    return w;
}

static std::string decode_one(const uint8_t *b, uint32_t at) {
    const uint32_t l_name = b[at + 12], n_cigar = b[at + 16] | b[at + 17] << 8, l_seq = (uint32_t)get32(b + at + 20);
    const uint8_t *name = b + at + 36, *seq = name + l_name + 4 * n_cigar, *qual = seq + (l_seq + 1) / 2;
    std::string t = "@";
    t.append((const char *)name, l_name ? l_name - 1 : 0);
    t.push_back('\n');
    for (uint32_t i = 0; i < l_seq; ++i) t.push_back("=ACMGRSVTWYHKDBN"[(seq[i / 2] >> (i % 2 ? 0 : 4)) & 15]);
    t += "\n+\n";
    for (uint32_t i = 0; i < l_seq; ++i) t.push_back((char)(qual[i] + 33));
    t.push_back('\n');
    return t;
}

static int fail(const char *what, int run) {
    printf("FAIL run %d: %s\n", run, what);
    return 1;
}

int main(int argc, char **argv) {
    const int runs = argc > 1 ? atoi(argv[1]) : 200;
    state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const long long tiles[] = {64, 256, 1000, 8192};
    long long repaired_total = 0, records_total = 0, errors_total = 0;
    for (int run = 0; run < runs; ++run) {
        const int n_ref = rnd() % 3;
        std::string text;
        const int mode = rnd() % 8;                       // 0: byte soup; 1: soup of small ints; else a stream, damaged
        long long entry = 0;
        if (mode == 0) {
            for (int k = rnd() % 3000; k > 0; --k) text.push_back((char)rnd());
        } else if (mode == 1) {
            for (int k = rnd() % 3000; k > 0; --k) text.push_back((char)(rnd() % 4 ? 0 : rnd() % 64));
        } else {
            entry = rnd() % 2 ? rnd() % 50 : 0;
            text.assign((size_t)entry, 'h');
            for (int k = rnd() % 40; k > 0; --k) text += make_record(n_ref);
            if (mode == 2 && !text.empty()) text[rnd() % text.size()] = (char)rnd();
            if (mode == 3 && text.size() > 8) {            // one field: four bytes of 0xFF, of zero, or a small number
                const size_t at = rnd() % (text.size() - 4);
                const int v = rnd() % 3 == 0 ? -1 : (rnd() % 2 ? 0 : (int)(rnd() % 300));
                for (int k = 0; k < 4; ++k) text[at + k] = (char)((uint32_t)v >> (8 * k));
            }
            if (mode == 4) text.resize(rnd() % (text.size() + 1));
            if (entry > (long long)text.size()) entry = (long long)text.size();
        }
        const long long n = (long long)text.size();
        uint8_t *b = (uint8_t *)malloc(n ? n : 1);         // exactly n bytes
        memcpy(b, text.data(), (size_t)n);
        const int final = rnd() % 2;
        const long long cap = rnd() % 4 ? (64 << 20) : 200;
        const Walk want = serial(b, n, entry, final, cap);
        for (long long tile : tiles) {
            const int64_t wb = emu_bam_walk_workspace(n, tile);
            void *work = malloc((size_t)wb);
            const long long capacity = (n - entry) / 36 + 1;
            uint32_t *starts = (uint32_t *)malloc((size_t)capacity * 4);
            int64_t result[4];
            if (emu_bam_walk(b, n, entry, n_ref, final, tile, cap, starts, capacity, result, work, wb, nullptr) != 0) return fail("walk rc", run);
            if (result[0] != (int64_t)want.starts.size() || result[1] != want.consumed || result[2] != want.error)
                return fail("count / consumed / error differ from the serial walk", run);
            if (result[0] > capacity) return fail("more records than the table holds", run);
            if (result[0] && memcmp(starts, want.starts.data(), (size_t)result[0] * 4)) return fail("record table differs", run);
            repaired_total += result[3];
            free(starts);
            free(work);
        }
        records_total += (long long)want.starts.size();
        errors_total += want.error != LLONG_MAX;
        for (int paired = 0; paired < 2; ++paired) {       // the decode of what the walk found
            const int64_t cnt = (int64_t)want.starts.size();
            std::vector<int64_t> offsets((size_t)cnt + 1);
            int64_t result[3];
            void *work = malloc(emu_bam_to_fastq_work_bytes(cnt));
            if (emu_bam_to_fastq(b, n, want.starts.data(), cnt, paired, offsets.data(), result, work, nullptr, nullptr) != 0) return fail("decode rc", run);
            const int64_t used = result[2];
            if (used != (paired ? cnt & ~(int64_t)1 : cnt) || offsets[(size_t)used] != result[0]) return fail("decode sizes", run);
            uint8_t *out = (uint8_t *)malloc(result[0] ? (size_t)result[0] : 1);
            if (emu_bam_to_fastq(b, n, want.starts.data(), cnt, paired, offsets.data(), result, work, out, nullptr) != 0) return fail("decode rc 2", run);
            if (!paired) {
                std::string mine;
                for (uint32_t at : want.starts) mine += decode_one(b, at);
                if ((int64_t)mine.size() != result[0] || memcmp(mine.data(), out, mine.size())) return fail("decoded text differs", run);
            }
            free(out);
            free(work);
        }
        free(b);
    }
    printf("ok: %d runs, %lld records, %lld error words, %lld repaired tiles\n", runs, records_total, errors_total, repaired_total);
    return 0;
}
