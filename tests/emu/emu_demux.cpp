// TEST INFRASTRUCTURE: CPU twin of the grouped formatter and the group codes of
// atropos_amd/csrc/fastq_emit_kernels.hip (atr_fastq_emit_grouped, atr_demux_groups), built from the same
// per-record source (demux_core.hpp, fastq_core.hpp) with -DATR_HOST_EMU.  A harness for the pipeline's
// CPU tests, not parity evidence for the kernels: the positions are made with plain running sums here.
#include <stdint.h>
#include <vector>

#include "emu_abi.hpp"
#include "demux_core.hpp"

using namespace atr;

extern "C" {

size_t emu_fastq_emit_grouped_work_bytes(int64_t, int) { return 16; }
EMU_TWIN(fastq_emit_grouped_work_bytes);

int emu_fastq_emit_grouped(const uint8_t *bytes, const atr_fastq_record *records, const int32_t *begin, const int32_t *end,
                           const int32_t *ubegin, const int32_t *uend, const int32_t *group, int n_groups, int64_t n,
                           int, int64_t *offsets, int64_t *group_offsets, void *, uint8_t *out, void *) {
    if (n_groups > ATR_EMIT_MAX_GROUPS) return ATR_ERR_UNSUPPORTED;
    if (n < 0 || n_groups < 1 || !group_offsets || ((ubegin == nullptr) != (uend == nullptr))) return ATR_ERR_INVALID;
    const FastqRecord *recs = (const FastqRecord *)records;
    if (!out) {
        std::vector<int64_t> total((size_t)n_groups + 1, 0);
        for (int64_t r = 0; r < n; ++r) {
            int g = group[r];
            const uint32_t s = demux_record_bytes(recs[r], begin[r], end[r], g, n_groups);
            if (g >= 0) total[(size_t)g + 1] += s;
        }
        group_offsets[0] = 0;
        for (int g = 0; g < n_groups; ++g) group_offsets[g + 1] = group_offsets[g] + total[(size_t)g + 1];
        std::vector<int64_t> run(group_offsets, group_offsets + n_groups);
        for (int64_t r = 0; r < n; ++r) {
            int g = group[r];
            const uint32_t s = demux_record_bytes(recs[r], begin[r], end[r], g, n_groups);
            offsets[r] = g < 0 ? -1 : run[(size_t)g];
            if (g >= 0) run[(size_t)g] += s;
        }
        return ATR_OK;
    }
    for (int64_t r = 0; r < n; ++r) {
        if (group[r] < 0 || group[r] >= n_groups) continue;
        const int a = begin[r], b = end[r] > a ? end[r] : a;
        fastq_format_record(out + offsets[r], bytes, recs[r], a, b, ubegin ? ubegin[r] : a, uend ? uend[r] : b, 0, 1);
    }
    return ATR_OK;
}
EMU_TWIN(fastq_emit_grouped);

int emu_demux_groups(const uint8_t *dest, const uint8_t *matched, const int64_t *last_which, const int32_t *adapter_group,
                     int n_adapters, int untrimmed_group, int64_t n, int32_t *group, void *) {
    if (n < 0 || n_adapters < 0) return ATR_ERR_INVALID;
    for (int64_t r = 0; r < n; ++r)
        group[r] = demux_group_one(dest[r], matched[r] != 0, last_which[r], adapter_group, n_adapters, untrimmed_group);
    return ATR_OK;
}
EMU_TWIN(demux_groups);

}  // extern "C"
