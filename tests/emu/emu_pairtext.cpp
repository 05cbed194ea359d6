// TEST INFRASTRUCTURE: CPU twin of the pair formatter of atropos_amd/csrc/pairtext_kernels.hip
// (atr_fastq_emit_pairs), built from the same per-pair source (pairtext_core.hpp over fastq_core.hpp) with
// -DATR_HOST_EMU.  One loop iteration here = one pair of the kernel's byte-per-lane path, with one lane.
#include <stdint.h>
#include <string.h>
#include <limits.h>

#include "emu_abi.hpp"
#include "pairtext_core.hpp"

using namespace atr;

extern "C" {

size_t emu_fastq_emit_pairs_work_bytes(int64_t) { return 16; }
EMU_TWIN(fastq_emit_pairs_work_bytes);

int emu_fastq_emit_pairs(const uint8_t *bytes1, const atr_fastq_record *records1, const int32_t *begin1, const int32_t *end1,
                         const int32_t *ubegin1, const int32_t *uend1, const uint8_t *bytes2,
                         const atr_fastq_record *records2, const int32_t *begin2, const int32_t *end2, const int32_t *ubegin2,
                         const int32_t *uend2, const uint8_t *dest, int which, int64_t n, int, int64_t *offsets, void *,
                         uint8_t *out, void *) {
    if (n < 0 || !offsets || ((ubegin1 == nullptr) != (uend1 == nullptr)) || ((ubegin2 == nullptr) != (uend2 == nullptr)))
        return ATR_ERR_INVALID;
    if (n == 0) {
        if (!out) offsets[0] = 0;
        return ATR_OK;
    }
    if (!bytes1 || !records1 || !begin1 || !end1 || !bytes2 || !records2 || !begin2 || !end2) return ATR_ERR_INVALID;
    const FastqRecord *rec1 = (const FastqRecord *)records1, *rec2 = (const FastqRecord *)records2;
    int64_t run = 0;
    for (int64_t r = 0; r < n; ++r) {
        const bool keep = !dest || dest[r] == which;
        const MateText m1 = mate_text(bytes1, rec1, begin1, end1, ubegin1, uend1, r);
        const MateText m2 = mate_text(bytes2, rec2, begin2, end2, ubegin2, uend2, r);
        if (!out) {
            offsets[r] = run;
            if (keep) run += pair_text_bytes(m1, m2);
        } else if (keep) {
            pair_format(out + offsets[r], m1, m2, 0, 1);
        }
    }
    if (!out) offsets[n] = run;
    return ATR_OK;
}
EMU_TWIN(fastq_emit_pairs);

size_t emu_overwrite_work_bytes(int64_t) { return 16; }
EMU_TWIN(overwrite_work_bytes);

int emu_overwrite_plan_batch(const uint8_t *bytes1, const atr_fastq_record *records1, const int32_t *begin1, const int32_t *end1,
                             const uint8_t *bytes2, const atr_fastq_record *records2, const int32_t *begin2,
                             const int32_t *end2, int64_t n, int lowq, int highq, int window, int base, uint8_t *which,
                             int64_t *grow1, int64_t *grow2, void *, void *) {
    if (n < 0 || window < 1 || lowq > highq || base < 0 || base > 255 || !grow1 || !grow2) return ATR_ERR_INVALID;
    int64_t at1 = 0, at2 = 0;
    for (int64_t r = 0; r < n; ++r) {
        const MateText m1 = mate_text(bytes1, (const FastqRecord *)records1, begin1, end1, nullptr, nullptr, r);
        const MateText m2 = mate_text(bytes2, (const FastqRecord *)records2, begin2, end2, nullptr, nullptr, r);
        const int len1 = m1.b - m1.a, len2 = m2.b - m2.a;
        const int w = overwrite_which(bytes1 + m1.rec.qual_off + m1.a, len1, bytes2 + m2.rec.qual_off + m2.a, len2, base,
                                      lowq, highq, window);
        which[r] = (uint8_t)w;
        grow1[r] = at1;
        grow2[r] = at2;
        if (w == 1) at1 += overwrite_clone_bytes(m2.rec, len2);
        if (w == 2) at2 += overwrite_clone_bytes(m1.rec, len1);
    }
    grow1[n] = at1;
    grow2[n] = at2;
    return ATR_OK;
}
EMU_TWIN(overwrite_plan_batch);

int emu_overwrite_apply_batch(uint8_t *bytes1, atr_fastq_record *records1, int32_t *begin1, int32_t *end1, uint8_t *bytes2,
                              atr_fastq_record *records2, int32_t *begin2, int32_t *end2, int64_t n, const uint8_t *which,
                              const int64_t *grow1, const int64_t *grow2, int64_t tail1, int64_t tail2, const uint8_t *comp,
                              int64_t *error, void *) {
    if (n < 0 || !comp || !error || tail1 < 0 || tail2 < 0) return ATR_ERR_INVALID;
    *error = LLONG_MAX;
    for (int64_t r = 0; r < n; ++r) {
        const int w = which[r];
        if (!w) continue;
        const MateText src = w == 1 ? mate_text(bytes2, (const FastqRecord *)records2, begin2, end2, nullptr, nullptr, r)
                                    : mate_text(bytes1, (const FastqRecord *)records1, begin1, end1, nullptr, nullptr, r);
        const uint32_t at = (uint32_t)(w == 1 ? tail1 + grow1[r] : tail2 + grow2[r]);
        if (!overwrite_clone_write((w == 1 ? bytes1 : bytes2) + at, src, comp, 0, 1) && r * 8 + 1 < *error) *error = r * 8 + 1;
        const int kept = src.b - src.a;
        const FastqRecord rec = overwrite_clone_record(src.rec, kept, at);
        memcpy(&(w == 1 ? records1 : records2)[r], &rec, sizeof(rec));
        (w == 1 ? begin1 : begin2)[r] = 0;
        (w == 1 ? end1 : end2)[r] = kept;
    }
    return ATR_OK;
}
EMU_TWIN(overwrite_apply_batch);

}  // extern "C"
