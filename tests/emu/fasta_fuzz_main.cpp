// TEST INFRASTRUCTURE: stand-alone driver of the CPU twin of the FASTA index and formatter (emu_fasta.cpp, fasta_core.hpp
// with -DATR_HOST_EMU), built with -fsanitize=address,undefined by tests/test_fasta_host.py and run as a subprocess:
// nothing sanitized is loaded into Python.
//
//   fasta_fuzz <soups> <seed>
// Every soup is a random run of bytes from an alphabet heavy in line ends, blanks, '>' and '#', in a heap block of
// exactly the size the entry points may read (the text padded to the next multiple of 16, and 16 more) plus the tail
// the scan asked for: a load or a store outside it is a sanitizer report.  The records are then checked against a
// reader written here line by line, and formatted, the text against the same reader's.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "atropos_hip.h"

extern "C" {
size_t emu_fasta_work_bytes(int64_t, int64_t);
int emu_fasta_scan(const uint8_t *, int64_t, uint32_t *, int64_t, void *, int64_t *, void *);
int emu_fasta_index(uint8_t *, int64_t, const uint32_t *, int64_t, const void *, int64_t, int64_t, int64_t, atr_fastq_record *,
                    uint32_t *, void *);
int emu_fasta_emit(const uint8_t *, const atr_fastq_record *, const int32_t *, const int32_t *, const int32_t *, const int32_t *,
                   const uint8_t *, int, int64_t, int, int64_t *, void *, uint8_t *, void *);
}

static uint64_t state;
static uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

static bool space(uint8_t c) { return c == 32 || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

struct Rec { std::string name, seq; };

// the reader, line by line; returns false when text stands in front of the first header
static bool read_all(const std::string &text, std::vector<Rec> &recs) {
    size_t start = 0;
    for (size_t i = 0; i < text.size(); ++i) {
        const uint8_t c = (uint8_t)text[i];
        if (!(c == '\n' || (c == '\r' && !(i + 1 < text.size() && text[i + 1] == '\n')))) continue;
        size_t lo = start, hi = i + 1;
        start = i + 1;
        while (lo < hi && space((uint8_t)text[lo])) ++lo;
        while (hi > lo && space((uint8_t)text[hi - 1])) --hi;
        if (lo == hi || text[lo] == '#') continue;
        if (text[lo] == '>') recs.push_back(Rec{text.substr(lo + 1, hi - lo - 1), ""});
        else if (recs.empty()) return false;
        else recs.back().seq += text.substr(lo, hi - lo);
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: fasta_fuzz <soups> <seed>\n"); return 2; }
    const int soups = atoi(argv[1]);
    state = (uint64_t)atoll(argv[2]) * 2654435761ull + 1;
    static const char alphabet[] = "ACGTNacgt>>##  \t\n\n\n\r\r\x0b\x1c\x1f\x80\xa0x";
    int bad_seen = 0;
    for (int s = 0; s < soups; ++s) {
        const size_t n = rnd() % (s % 10 == 0 ? 70000 : 600);
        std::string text;
        if (s % 3) text = ">first\n";
        for (size_t i = text.size(); i < n; ++i) text += alphabet[rnd() % (sizeof(alphabet) - 1)];
        if (!text.empty() && text.back() != '\n' && text.back() != '\r') text += '\n';
        const int64_t nbytes = (int64_t)text.size();
        const int64_t tail_off = (nbytes + 15) / 16 * 16 + 16;
        std::vector<Rec> want;
        const bool good = read_all(text, want);

        uint8_t *plain = (uint8_t *)calloc((size_t)tail_off, 1);
        memcpy(plain, text.data(), text.size());
        int64_t nlines = 0, info[3] = {-1, -1, -1};
        for (size_t i = 0; i < text.size(); ++i)                 // (what atr_fastq_count_lines tells the caller)
            nlines += text[i] == '\n' || (text[i] == '\r' && !(i + 1 < text.size() && text[i + 1] == '\n'));
        uint32_t *line_ends = (uint32_t *)malloc((size_t)(nlines ? nlines : 1) * 4);
        void *work = malloc(emu_fasta_work_bytes(nbytes, nlines));
        if (emu_fasta_scan(plain, nbytes, line_ends, nlines, work, info, nullptr) != 0) { fprintf(stderr, "soup %d: scan\n", s); return 3; }
        if (good != (info[2] == INT64_MAX)) { fprintf(stderr, "soup %d: error word %lld\n", s, (long long)info[2]); return 3; }
        if (!good) ++bad_seen;
        if (good) {
            const int64_t nrec = info[0], gather = info[1];
            if (nrec != (int64_t)want.size()) { fprintf(stderr, "soup %d: %lld records, %zu expected\n", s, (long long)nrec, want.size()); return 3; }
            uint8_t *data = (uint8_t *)calloc((size_t)(tail_off + gather), 1);       // exactly the text, its padding, the tail
            memcpy(data, plain, (size_t)tail_off);
            atr_fastq_record *recs = (atr_fastq_record *)malloc((size_t)(nrec ? nrec : 1) * sizeof(atr_fastq_record));
            uint32_t *ends = (uint32_t *)malloc((size_t)(nrec ? nrec : 1) * 4);
            if (emu_fasta_index(data, nbytes, line_ends, nlines, work, nrec, tail_off, gather, recs, ends, nullptr) != 0) {
                fprintf(stderr, "soup %d: index\n", s);
                return 3;
            }
            std::string expect;
            int64_t used = 0;
            for (int64_t r = 0; r < nrec; ++r) {
                const std::string name((const char *)data + recs[r].name_off, recs[r].name_len);
                const std::string seq((const char *)data + recs[r].seq_off, recs[r].seq_len);
                if (name != want[r].name || seq != want[r].seq || recs[r].qual_len || recs[r].flags || ends[r] >= (uint32_t)nbytes) {
                    fprintf(stderr, "soup %d: record %lld differs\n", s, (long long)r);
                    return 3;
                }
                if (recs[r].seq_off >= (uint32_t)tail_off) used += recs[r].seq_len;
                expect += ">" + name + "\n" + seq + "\n";
            }
            if (used != gather) { fprintf(stderr, "soup %d: tail of %lld bytes, %lld used\n", s, (long long)gather, (long long)used); return 3; }
            std::vector<int32_t> begin((size_t)nrec + 1, 0), end((size_t)nrec + 1, 0);
            for (int64_t r = 0; r < nrec; ++r) end[r] = (int32_t)recs[r].seq_len;
            std::vector<int64_t> offsets((size_t)nrec + 1, -1);
            emu_fasta_emit(data, recs, begin.data(), end.data(), nullptr, nullptr, nullptr, 0, nrec, 0, offsets.data(), nullptr, nullptr, nullptr);
            if (offsets[nrec] != (int64_t)expect.size()) { fprintf(stderr, "soup %d: %lld bytes of text\n", s, (long long)offsets[nrec]); return 3; }
            uint8_t *out = (uint8_t *)malloc(expect.size() ? expect.size() : 1);
            emu_fasta_emit(data, recs, begin.data(), end.data(), nullptr, nullptr, nullptr, 0, nrec, 0, offsets.data(), nullptr, out, nullptr);
            if (memcmp(out, expect.data(), expect.size()) != 0) { fprintf(stderr, "soup %d: text differs\n", s); return 3; }
            free(out);
            free(ends);
            free(recs);
            free(data);
        }
        free(work);
        free(line_ends);
        free(plain);
    }
    printf("ok: %d soups, %d with text in front of the first header\n", soups, bad_seen);
    return 0;
}
