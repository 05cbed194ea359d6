// TEST INFRASTRUCTURE: CPU twin of the FASTA index and formatter of atropos_amd/csrc/fasta_kernels.hip, built from
// the same per-line and per-record source (fasta_core.hpp over fastq_core.hpp) with -DATR_HOST_EMU.  One loop
// iteration here = one thread (line, record) of the kernels; the prefix sums are plain running sums.  The scratch
// between emu_fasta_scan and emu_fasta_index holds the arrays the kernels keep there, in a layout of its own.
#include <stdint.h>
#include <string.h>
#include <limits.h>

#include "emu_abi.hpp"
#include "fasta_core.hpp"

using namespace atr;

namespace {

typedef unsigned long long u64;

struct Work {
    uint8_t *cls;
    uint32_t *at, *len, *head_line;
    u64 *pre, *tail_pre;
};

size_t up(size_t x) { return (x + 15) & ~(size_t)15; }

Work carve(void *work, int64_t nlines, size_t *bytes) {
    Work w;
    char *p = (char *)work;
    size_t o = 0;
    w.pre = (u64 *)(p + o); o += up((size_t)(nlines + 1) * 8);
    w.tail_pre = (u64 *)(p + o); o += up((size_t)(nlines + 1) * 8);
    w.at = (uint32_t *)(p + o); o += up((size_t)nlines * 4);
    w.len = (uint32_t *)(p + o); o += up((size_t)nlines * 4);
    w.head_line = (uint32_t *)(p + o); o += up((size_t)nlines * 4);
    w.cls = (uint8_t *)(p + o); o += up((size_t)nlines);
    if (bytes) *bytes = o + 16;
    return w;
}

}  // namespace

extern "C" {

size_t emu_fasta_work_bytes(int64_t nbytes, int64_t nlines) {
    if (nbytes < 0 || nlines < 0) return 0;
    size_t bytes;
    carve(nullptr, nlines, &bytes);
    return bytes;
}
EMU_TWIN(fasta_work_bytes);

int emu_fasta_scan(const uint8_t *bytes, int64_t nbytes, uint32_t *line_ends, int64_t nlines, void *work, int64_t *info, void *) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || nlines < 0 || nlines > nbytes || !info) return ATR_ERR_INVALID;
    info[0] = info[1] = 0;
    info[2] = LLONG_MAX;
    if (nlines == 0) return ATR_OK;
    if (!bytes || !work || !line_ends) return ATR_ERR_INVALID;
    const Work w = carve(work, nlines, nullptr);
    int64_t k = 0;
    for (int64_t i = 0; i < nbytes && k < nlines; ++i)
        if (is_line_end(bytes[i], i + 1 < nbytes ? bytes[i + 1] : 0)) line_ends[k++] = (uint32_t)i;
    u64 run = 0;
    for (int64_t L = 0; L < nlines; ++L) {
        const int c = fasta_line_one(bytes, L ? line_ends[L - 1] + 1u : 0u, line_ends[L], w.at[L], w.len[L]);
        w.cls[L] = (uint8_t)c;
        w.pre[L] = run;
        run += fasta_line_value(c, w.len[L]);
    }
    w.pre[nlines] = run;
    for (int64_t L = 0; L < nlines; ++L) {
        if (w.cls[L] == FASTA_HEADER) w.head_line[fasta_pre_headers(w.pre[L])] = (uint32_t)L;
        else if (w.cls[L] == FASTA_SEQ && fasta_pre_headers(w.pre[L]) == 0 && info[2] == LLONG_MAX)
            info[2] = (L + 1) * 8 + ATR_FASTA_ERR_HEADER;
    }
    const FastaLines ln = {line_ends, w.cls, w.at, w.len, w.pre, w.head_line, nlines, fasta_pre_headers(run)};
    u64 tail = 0;
    for (int64_t r = 0; r <= nlines; ++r) {
        w.tail_pre[r] = tail;
        if (r < ln.nrec) tail += fasta_record_gather(ln, r);
    }
    info[0] = ln.nrec;
    info[1] = (int64_t)tail;
    return ATR_OK;
}
EMU_TWIN(fasta_scan);

int emu_fasta_index(uint8_t *bytes, int64_t nbytes, const uint32_t *line_ends, int64_t nlines, const void *work, int64_t nrec,
                    int64_t tail_off, int64_t tail_bytes, atr_fastq_record *records, uint32_t *record_ends, void *) {
    if (nbytes < 0 || nbytes >= (int64_t)0xFFFFFFF0ll || nlines < 0 || nrec < 0 || nrec > nlines || tail_bytes < 0 ||
        tail_off < nbytes || (tail_off & 15) || tail_off + tail_bytes >= (int64_t)0xFFFFFFF0ll)
        return ATR_ERR_INVALID;
    if (nrec == 0) return ATR_OK;
    if (!bytes || !work || !line_ends || !records || !record_ends) return ATR_ERR_INVALID;
    const Work w = carve(const_cast<void *>(work), nlines, nullptr);
    const FastaLines ln = {line_ends, w.cls, w.at, w.len, w.pre, w.head_line, nlines, nrec};
    for (int64_t r = 0; r < nrec; ++r) {
        FastqRecord rec;
        fasta_record_one(ln, w.tail_pre, (uint32_t)tail_off, r, rec, record_ends[r]);
        memcpy(&records[r], &rec, sizeof(rec));
    }
    for (int64_t L = 0; L < nlines && tail_bytes > 0; ++L) {
        uint32_t to;
        if (!fasta_line_target(ln, w.tail_pre, L, to)) continue;
        if ((u64)to + w.len[L] > (u64)tail_bytes) continue;
        lanes_copy(bytes + tail_off + to, bytes + w.at[L], w.len[L], 0, 1);
    }
    return ATR_OK;
}
EMU_TWIN(fasta_index);

size_t emu_fasta_emit_work_bytes(int64_t) { return 16; }
EMU_TWIN(fasta_emit_work_bytes);

int emu_fasta_emit(const uint8_t *bytes, const atr_fastq_record *records, const int32_t *begin, const int32_t *end,
                   const int32_t *ubegin, const int32_t *uend, const uint8_t *dest, int which, int64_t n, int, int64_t *offsets,
                   void *, uint8_t *out, void *) {
    if (n < 0 || !offsets || ((ubegin == nullptr) != (uend == nullptr))) return ATR_ERR_INVALID;
    if (n == 0) {
        if (!out) offsets[0] = 0;
        return ATR_OK;
    }
    if (!bytes || !records || !begin || !end) return ATR_ERR_INVALID;
    int64_t run = 0;
    for (int64_t r = 0; r < n; ++r) {
        FastqRecord rec;
        memcpy(&rec, &records[r], sizeof(rec));
        const bool keep = !dest || dest[r] == which;
        const int a = begin[r], b = end[r] > a ? end[r] : a;
        if (!out) {
            offsets[r] = run;
            if (keep) run += fasta_record_bytes(rec, b - a);
        } else if (keep) {
            fasta_format_record(out + offsets[r], bytes, rec, a, b, ubegin ? ubegin[r] : a, uend ? uend[r] : b, 0, 1);
        }
    }
    if (!out) offsets[n] = run;
    return ATR_OK;
}
EMU_TWIN(fasta_emit);

}  // extern "C"
