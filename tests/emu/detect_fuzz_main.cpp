// TEST INFRASTRUCTURE: stand-alone driver of the CPU twin of the detect passes (emu_detect.cpp, detect_core.hpp with
// -DATR_HOST_EMU), built with -fsanitize=address,undefined by tests/test_detect_kernels_host.py and run as a
// subprocess: nothing sanitized is loaded into Python.
//
//   detect_fuzz <rounds> <seed>
// Every round builds a handle of its own (1 .. 6 known sequences over ACGT, ACGTN or the IUPAC letters, 0 .. 4
// past-end bases, a complexity table of exactly (max_len + 1)^2 doubles) and 0 .. 300 reads of 0 .. max_len bases back
// to back in a heap block of exactly their size, the last read ending on the block's last byte: a load outside it is a
// sanitizer report, and so is a shift or an overflow the language leaves undefined.  The passes run as the detector
// chains them; the distinct count is checked against a std::set of the kept strings and the abundance against
// std::string::find, every third round with all hashes forced equal.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "atropos_hip.h"

extern "C" {
extern int emu_detect_force_hash;
int emu_detect_create(const uint8_t *, const int32_t *, int, int, const uint8_t *, int, const int32_t *, const double *, int, void **);
void emu_detect_destroy(void *);
int64_t emu_detect_counter_bytes(const void *);
int emu_detect_filter_batch(const void *, const uint8_t *, const atr_fastq_record *, int64_t, int, int32_t *, int64_t *, void *, void *);
int emu_detect_mark_batch(const void *, const uint8_t *, const atr_fastq_record *, const int32_t *, const int64_t *, const int64_t *,
                          int64_t, uint8_t *, void *, void *);
int emu_detect_batch(const void *, const uint8_t *, const atr_fastq_record *, const int32_t *, const int64_t *, const uint8_t *,
                     int64_t, void *, void *);
}

static uint64_t state;
static uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
static std::string soup(size_t n, const char *alphabet) {
    std::string s;
    const size_t letters = strlen(alphabet);
    for (size_t i = 0; i < n; ++i) s += alphabet[rnd() % letters];
    return s;
}
#define FAIL(...) do { fprintf(stderr, "round %d: ", round); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 3; } while (0)

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: detect_fuzz <rounds> <seed>\n"); return 2; }
    const int rounds = atoi(argv[1]);
    state = (uint64_t)atoll(argv[2]) * 2654435761ull + 1;
    static const char *alphabets[] = {"ACGT", "ACGTN", "ACGTRYSWKMBDHVN"};
    static const int max_k[] = {32, 21, 16};
    long long total_kept = 0, total_distinct = 0, total_abundance = 0;
    for (int round = 0; round < rounds; ++round) {
        const int which = (int)(rnd() % 3), k = 4 + (int)(rnd() % (uint32_t)(max_k[which] - 3));
        const int max_len = round % 4 == 0 ? 1 + (int)(rnd() % 320) : 320, nseq = 1 + (int)(rnd() % 6), npast = (int)(rnd() % 5);
        std::vector<std::string> known;
        std::string all;
        std::vector<int32_t> lens, thr;
        for (int s = 0; s < nseq; ++s) {
            known.push_back(soup((size_t)k + rnd() % (uint32_t)(131 - k), alphabets[which]));
            all += known.back();
            lens.push_back((int32_t)known.back().size());
            thr.push_back((int32_t)(rnd() % 7) - 1);
        }
        const uint8_t past[4] = {'A', 'G', 'N', 'C'};
        const size_t side = (size_t)max_len + 1;
        double *table = (double *)calloc(side * side, sizeof(double));       // exactly what the entry point may read
        for (size_t n = 1; n < side; ++n)
            for (size_t c = 1; c <= n; ++c) table[n * side + c] = ((double)c / (double)n) * log((double)c / (double)n) / log(2.0);
        void *h = nullptr;
        const int rc = emu_detect_create((const uint8_t *)all.data(), lens.data(), nseq, k, npast ? past : nullptr, npast, thr.data(),
                                         table, max_len, &h);
        free(table);
        if (rc != 0) FAIL("create returned %d (k = %d, %d sequences)", rc, k, nseq);
        // the reads
        const int n = (int)(rnd() % 301);
        std::vector<std::string> reads;
        std::string text;
        std::vector<atr_fastq_record> recs((size_t)n + 1);
        int longest = 0;
        for (int r = 0; r < n; ++r) {
            const int len = (int)(rnd() % (uint32_t)(max_len + 1));
            std::string s = r % 7 == 6 && r ? reads[rnd() % (uint32_t)r] : soup((size_t)len, rnd() % 5 ? "ACGT" : "AACCGTNacgt");
            if (r % 3 == 0 && !s.empty()) {                                           // a run of a past-end base, a known sequence
                const std::string piece = rnd() % 2 ? std::string(1 + rnd() % 12, (char)past[rnd() % 4]) : known[rnd() % (uint32_t)nseq];
                const size_t at = rnd() % (uint32_t)s.size();
                s = (s.substr(0, at) + piece + s.substr(at)).substr(0, (size_t)max_len);
                if (rnd() % 2) s = s.substr(0, std::min(s.size(), at + piece.size()));       // ... that ends the read
            }
            memset(&recs[(size_t)r], 0, sizeof(atr_fastq_record));
            recs[(size_t)r].seq_off = (uint32_t)text.size();
            recs[(size_t)r].seq_len = (uint32_t)s.size();
            longest = std::max(longest, (int)s.size());
            text += s;
            reads.push_back(s);
        }
        uint8_t *bytes = (uint8_t *)malloc(text.size() ? text.size() : 1);
        memcpy(bytes, text.data(), text.size());
        const size_t words = (size_t)emu_detect_counter_bytes(h) / 8;
        uint64_t *block = (uint64_t *)calloc(words, 8);
        int32_t *kept = (int32_t *)malloc((size_t)(n ? n : 1) * 4);
        int64_t *hashes = (int64_t *)malloc((size_t)(n ? n : 1) * 8);
        emu_detect_force_hash = round % 3 == 2;
        if (emu_detect_filter_batch(h, bytes, recs.data(), n, longest, kept, hashes, block, nullptr) != 0) FAIL("filter");
        emu_detect_force_hash = 0;
        std::vector<int64_t> order;
        std::set<std::string> distinct;
        for (int r = 0; r < n; ++r) {
            if (kept[r] < 0 || kept[r] > (int)reads[(size_t)r].size() || (kept[r] && kept[r] < k)) FAIL("read %d keeps %d of %zu", r, kept[r], reads[(size_t)r].size());
            if (kept[r]) { order.push_back(r); distinct.insert(reads[(size_t)r].substr(0, (size_t)kept[r])); }
        }
        if (block[0] != order.size() || block[3] != 0) FAIL("kept %llu, %zu expected", (unsigned long long)block[0], order.size());
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return hashes[a] < hashes[b]; });
        const int64_t m = (int64_t)order.size();
        std::vector<int64_t> head((size_t)m + 1);
        for (int64_t i = 0; i < m; ++i) head[(size_t)i] = i && hashes[order[(size_t)i]] == hashes[order[(size_t)i - 1]] ? head[(size_t)i - 1] : i;
        uint8_t *rep = (uint8_t *)malloc((size_t)(m ? m : 1));
        if (emu_detect_mark_batch(h, bytes, recs.data(), kept, order.data(), head.data(), m, rep, block, nullptr) != 0) FAIL("mark");
        if (block[1] != distinct.size()) FAIL("%llu distinct, %zu expected", (unsigned long long)block[1], distinct.size());
        if (emu_detect_batch(h, bytes, recs.data(), kept, order.data(), rep, m, block, nullptr) != 0) FAIL("match");
        long long invalid = 0;
        std::vector<uint64_t> abundance((size_t)nseq, 0);
        for (const std::string &s : distinct) {
            if (s.find_first_not_of("ACGTRYSWKMBDHVNacgtryswkmbdhvn") != std::string::npos) { ++invalid; continue; }
            for (int q = 0; q < nseq; ++q) abundance[(size_t)q] += s.find(known[(size_t)q]) != std::string::npos;
        }
        if ((long long)block[2] != invalid) FAIL("%llu invalid, %lld expected", (unsigned long long)block[2], invalid);
        for (int q = 0; q < nseq; ++q) {
            if (block[8 + 3 * (size_t)nseq + (size_t)q] != abundance[(size_t)q]) FAIL("abundance of sequence %d", q);
            if (block[8 + (size_t)nseq + (size_t)q] > distinct.size() || (thr[(size_t)q] < 0 && block[8 + (size_t)nseq + (size_t)q])) FAIL("hits of sequence %d", q);
            total_abundance += (long long)abundance[(size_t)q];
        }
        total_kept += m;
        total_distinct += (long long)distinct.size();
        free(rep); free(hashes); free(kept); free(block); free(bytes);
        emu_detect_destroy(h);
    }
    printf("ok: %d rounds, %lld reads kept, %lld distinct, %lld whole known sequences\n", rounds, total_kept, total_distinct, total_abundance);
    return 0;
}
