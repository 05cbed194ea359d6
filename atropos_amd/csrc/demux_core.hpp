// demux_core.hpp -- per-record arithmetic of demultiplexing (`{name}` in the output path): which output
// a read goes to (commands/trim/writers.py:138-154 with the formatters trim/__init__.py:605-630 installs).
//
// Compiled for gfx950 and, with -DATR_HOST_EMU, for the CPU test emulation (tests/emu).
#ifndef ATR_DEMUX_CORE_HPP
#define ATR_DEMUX_CORE_HPP

#include "fastq_core.hpp"

namespace atr {

// Formatters.format: a read the filters let through (NoFilter) that carries a match goes to the output of the
// adapter of its LAST match; one without a match, and -- when that filter is on and has an output -- one the
// UntrimmedFilter took, go to the untrimmed output; every other read is not written here.
// which: the adapter of the last match; adapter_group: the output of every adapter (NULL: its own index);
// untrimmed_group: the untrimmed output, or -1 without one (--discard-untrimmed).
ATR_DEV int32_t demux_group_one(int dest, bool matched, long long which, const int32_t *adapter_group, int n_adapters,
                                int untrimmed_group) {
    if (dest == ATR_DEST_KEEP && matched)
        return (which >= 0 && which < n_adapters) ? (adapter_group ? adapter_group[which] : (int32_t)which) : -1;
    if (dest == ATR_DEST_KEEP || dest == ATR_DEST_UNTRIMMED) return untrimmed_group;
    return -1;
}

// What a record adds to its output: its formatted size, or nothing when it is not written.  g: its group code,
// normalised to -1 for every value outside 0 .. n_groups-1.
ATR_DEV uint32_t demux_record_bytes(const FastqRecord &rec, int begin, int end, int &g, int n_groups) {
    if (g < 0 || g >= n_groups) { g = -1; return 0u; }
    return fastq_record_bytes(rec, end > begin ? end - begin : 0);
}

}  // namespace atr
#endif
